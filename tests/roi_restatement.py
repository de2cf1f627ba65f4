"""The element-wise reference of tests/test_gpu_roi.py: RoIAlign forward and backward (csrc/roi.hip) against float64 sums over the taps that
oracle.roi_align._samples yields -- the tap positions and fp32 weights in the kernel's expression order (roi.hip is built with
-ffp-contract=off, so the geometry is exact; what is left is the order and rounding of the sums).  Not a test module (pytest does not collect
it); tests/test_roi_restatement_cpu.py pins it without a GPU.

  * forward, per output element: ref = sum over the bin's taps of w * f / count in float64, f = the STORED feature values (fp32 or bf16);
    limit = sum_limit(4 * taps + 4, sum|w f| / count): one chain of 4 additions per tap, and 4 for the roundings of the products and of
    `* (1 / count)`.
  * backward, per gradient element: ref = the float64 sum of its contributions g * w / count; limit = sum_limit(m + 3, sum|contribution|),
    m = the number of contributions to that element (atomic additions in any order), 3 for g * (1 / count) * w; bf16 features get half a
    bf16 ulp of the reference on top, because the gradient is rounded to the features' type on return.
  * a box whose image index is not in [0, B) -- NaN included -- pools nothing: an all-zero output row (limit 0) and no contribution.
An element without taps has limit 0: it must be exactly zero.
"""
import numpy as np
import torch

import streaming_measure as sm
from oracle import roi_align as R

f = np.float32


def has_image(index, B):
    return bool(index >= 0 and index < B)            # False for NaN


def forward_reference(feat, boxes, output_size, spatial_scale, sampling_ratio):
    """feat [B, C, H, W] (fp32 or bf16 tensor), boxes [K, 5] float32 array -> (ref [K, C, PH, PW], limit), float64 tensors"""
    fm_all = feat.double().numpy()
    B, C, H, W = fm_all.shape
    PH, PW = output_size
    ref = np.zeros((len(boxes), C, PH, PW))
    sab = np.zeros_like(ref)
    n = np.zeros((len(boxes), 1, PH, PW))
    for k, box in enumerate(boxes):
        if not has_image(box[0], B):
            continue
        fm = fm_all[int(box[0])]
        for ph, pw, taps, count in R._samples(box[1:], (PH, PW), H, W, spatial_scale, sampling_ratio):
            for yl, xl, yh, xh, w1, w2, w3, w4 in taps:
                for w, y, x in ((w1, yl, xl), (w2, yl, xh), (w3, yh, xl), (w4, yh, xh)):
                    t = float(w) * fm[:, y, x] / count
                    ref[k, :, ph, pw] += t
                    sab[k, :, ph, pw] += np.abs(t)
            n[k, 0, ph, pw] = 4 * len(taps) + 4
    return torch.from_numpy(ref), sm.sum_limit(torch.from_numpy(n), torch.from_numpy(sab))


def backward_reference(grad_out, boxes, feature_shape, spatial_scale, sampling_ratio):
    """grad_out [K, C, PH, PW] fp32 tensor -> (ref [B, C, H, W], limit), float64 tensors"""
    g = grad_out.double().numpy()
    B, C, H, W = feature_shape
    PH, PW = g.shape[2:]
    ref = np.zeros(feature_shape)
    sab = np.zeros(feature_shape)
    m = np.zeros((B, 1, H, W))
    for k, box in enumerate(boxes):
        if not has_image(box[0], B):
            continue
        b = int(box[0])
        for ph, pw, taps, count in R._samples(box[1:], (PH, PW), H, W, spatial_scale, sampling_ratio):
            go = g[k, :, ph, pw] / count
            for yl, xl, yh, xh, w1, w2, w3, w4 in taps:
                for w, y, x in ((w1, yl, xl), (w2, yl, xh), (w3, yh, xl), (w4, yh, xh)):
                    t = go * float(w)
                    ref[b, :, y, x] += t
                    sab[b, :, y, x] += np.abs(t)
                    m[b, 0, y, x] += 1
    return torch.from_numpy(ref), sm.sum_limit(torch.from_numpy(m) + 3, torch.from_numpy(sab))


def first_sample(lo, hi, bins, spatial_scale, sampling_ratio):
    """the coordinate of the first sample along one axis of a box [lo, hi], in the kernel's fp32 expression"""
    s1, s2 = f(f(lo) * f(spatial_scale)), f(f(hi) * f(spatial_scale))
    roi = max(f(s2 - s1), f(1.0))
    b = f(roi / f(bins))
    grid = sampling_ratio if sampling_ratio > 0 else int(np.ceil(float(b)))
    return f(s1 + f(0) * b + f(f(f(0) + f(0.5)) * b) / f(grid))


def edge_boxes(B, H, W, output_size, spatial_scale, sampling_ratio, seed=0):
    """[K, 5] float32 boxes in input coordinates, and the list of (row, axis, bins, target) whose first sample along that axis falls exactly
    on target = -1, 0, size - 1 and size (the bin is 2 * grid cells long, so the first sample lies one cell -- half a cell when the grid is
    adaptive, 2 per bin -- behind the box's start).  Then: a box of zero size, a box entirely outside, two identical boxes, random ones."""
    PH, PW = output_size
    rng = np.random.default_rng(100 + seed)
    rows, exact = [], []
    for axis, size, bins in ((0, H, PH), (1, W, PW)):
        g = sampling_ratio if sampling_ratio > 0 else 2
        step = 1.0 if sampling_ratio > 0 else 0.5
        length = (2.0 * g if sampling_ratio > 0 else 2.0) * bins
        other = (1.0, 1.0 + min((W if axis == 0 else H) - 2, 3))
        for target in (-1.0, 0.0, size - 1.0, float(size)):
            lo = target - step
            span = (lo, lo + length)
            y, x = (span, other) if axis == 0 else (other, span)
            exact.append((len(rows), axis, bins, target))
            rows.append([len(rows) % B, x[0], y[0], x[1], y[1]])
    rows.append([0, 2.0, 2.0, 2.0, 2.0])
    rows.append([B - 1, W + 2.0, H + 2.0, W + 5.0, H + 4.0])
    twin = [B - 1, 0.75, 1.25, W - 1.5, H - 0.75]
    rows += [twin, list(twin)]
    for _ in range(4):
        x1, y1 = rng.uniform(-2, W - 1), rng.uniform(-2, H - 1)
        rows.append([int(rng.integers(0, B)), x1, y1, x1 + rng.uniform(0.3, W), y1 + rng.uniform(0.3, H)])
    boxes = np.asarray(rows, dtype=np.float64)
    boxes[:, 1:] /= spatial_scale
    return boxes.astype(np.float32), exact


# (spatial_scale, sampling_ratio, output_size, C, (H, W), bf16 features): every value the kernel branches on -- the scale, a fixed and the
# adaptive grid, one bin, the 7 x 7 of the model, and PW = 50 and 99 for the second 49-bin pass; C below, at and above the 64-channel slice
CASES = [
    (1.0, -1, (7, 7), 65, (5, 9), False),
    (0.25, 2, (2, 50), 64, (13, 7), False),
    (0.0625, 3, (3, 99), 1, (5, 9), False),
    (1.0, 1, (1, 1), 130, (13, 7), True),
    (0.25, -1, (3, 99), 63, (5, 9), True),
    (0.0625, 2, (7, 7), 63, (13, 7), False),
]
BATCH = 2
