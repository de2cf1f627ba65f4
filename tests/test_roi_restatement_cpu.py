"""tests/roi_restatement.py pinned without a GPU: the oracle's fp32 RoIAlign passes the element limits on the cases of the GPU test, the edge
boxes put a sample exactly on -1, 0, size - 1 and size, and the wrong kernels the GPU test is there to catch are rejected."""
import numpy as np
import pytest
import torch

import roi_restatement as rr
import streaming_measure as sm
from oracle import roi_align as R


def make(case, seed=0):
    scale, sampling, osz, C, (H, W), bf16 = case
    g = torch.Generator().manual_seed(31 + C)
    feat = torch.randn(rr.BATCH, C, H, W, generator=g)
    feat = feat.bfloat16() if bf16 else feat
    boxes, exact = rr.edge_boxes(rr.BATCH, H, W, osz, scale, sampling)
    return feat, boxes, exact, g


@pytest.mark.parametrize('case', rr.CASES, ids=[f'case{i}' for i in range(len(rr.CASES))])
def test_edge_boxes_put_samples_exactly_on_the_borders(case):
    scale, sampling, osz, C, (H, W), _ = case
    boxes, exact = rr.edge_boxes(rr.BATCH, H, W, osz, scale, sampling)
    assert len(exact) == 8
    for row, axis, bins, target in exact:
        lo, hi = (boxes[row, 2], boxes[row, 4]) if axis == 0 else (boxes[row, 1], boxes[row, 3])
        assert rr.first_sample(lo, hi, bins, scale, sampling) == np.float32(target)
    assert set(t for _, a, _, t in exact if a == 0) == {-1.0, 0.0, H - 1.0, float(H)}
    assert set(t for _, a, _, t in exact if a == 1) == {-1.0, 0.0, W - 1.0, float(W)}
    assert (boxes[8, 1:3] == boxes[8, 3:5]).all() and (boxes[10] == boxes[11]).all()


@pytest.mark.parametrize('case', [rr.CASES[0], rr.CASES[1], rr.CASES[3]], ids=['adaptive_7x7', 'fixed_2x50', 'bf16_1x1'])
def test_oracle_fp32_passes_and_wrong_kernels_do_not(case):
    scale, sampling, osz, C, (H, W), bf16 = case
    feat, boxes, exact, g = make(case)
    ref, lim = rr.forward_reference(feat, boxes, osz, scale, sampling)
    got = torch.from_numpy(R.roi_align(feat.float().numpy(), boxes, osz, scale, sampling))
    w = sm.worst_f32(got, ref, lim)
    print(f'oracle fp32 forward: {w:.3f} of the limit')
    assert w <= 1.0
    assert (lim[9] == 0).all() and (ref[9] == 0).all(), 'the box outside the map pools nothing'
    if osz[1] > 49:                                                    # the second 49-bin pass left out
        bad = got.clone()
        bad[..., 49:] = 0
        assert sm.worst_f32(bad, ref, lim) > 100
    bad = torch.from_numpy(R.roi_align(feat.float().numpy(), boxes, osz, scale, sampling if sampling > 0 else 1))
    if sampling <= 0:                                                  # a fixed grid where the adaptive one is asked for
        assert sm.worst_f32(bad, ref, lim) > 100
    one_tap = got.clone()                                               # one wrong tap on a small element
    k, c = 12, C - 1
    i = ref[k, c].abs().argmin()
    one_tap[k, c].view(-1)[i] += 1.5e-5                                # inside allclose(rtol=1e-5, atol=2e-5), outside the element's limit
    assert sm.worst_f32(one_tap, ref, lim) > 5 and np.allclose(one_tap.numpy(), got.numpy(), rtol=1e-5, atol=2e-5)
    # backward: float64 accumulation rounded once passes; two identical boxes add; a contribution left out does not pass
    go = torch.randn(ref.shape, generator=g)
    dref, dlim = rr.backward_reference(go, boxes, feat.shape, scale, sampling)
    dgot = torch.from_numpy(R.roi_align_backward(go.numpy(), boxes, tuple(feat.shape), scale, sampling))
    assert sm.worst_f32(dgot, dref, dlim) <= 1.0
    less = torch.from_numpy(R.roi_align_backward(go.numpy(), boxes[:11], tuple(feat.shape), scale, sampling))
    assert sm.worst_f32(less, dref, dlim) > 100
    # an image index outside [0, B) -- NaN included -- pools nothing and adds nothing
    for idx in (-1.0, float(rr.BATCH), 1e9, float('nan')):
        b2 = boxes.copy()
        b2[12, 0] = idx
        r2, l2 = rr.forward_reference(feat, b2, osz, scale, sampling)
        assert (r2[12] == 0).all() and (l2[12] == 0).all() and torch.equal(r2[:12], ref[:12]) and torch.equal(r2[13:], ref[13:])
        d2, _ = rr.backward_reference(go, b2, feat.shape, scale, sampling)
        keep = [i for i in range(len(boxes)) if i != 12]
        d3, _ = rr.backward_reference(go[keep], boxes[keep], feat.shape, scale, sampling)
        assert torch.equal(d2, d3)
