"""The references and the edge inputs of tests/test_gpu_detect_edges.py: eval decode, RPN row decode, candidate selection, rank and NMS, and the
two matchers (csrc/detect.hip).  Not a test module (pytest does not collect it); tests/test_detect_restatement_cpu.py pins it without a GPU:
the restatements equal the oracle's functions at the oracle's fixed parameters, and every constructed input has the property it is there for.

  * Decode (both variants of fva_yolo_decode, and fva_rpn_decode) is arithmetic: written once with a dtype parameter, float64 is the
    reference and fp32 gives the e32 of streaming_measure.limit_of; rows stay aligned with the kernel's output (the demo variant keeps every
    row and stores -1 as objectness where the reference drops the box).  mag of an element = the largest term of its last operation:
        sigmoid outputs, exp(t) * anchor, (2 sigmoid)^2 * anchor * stride:   the value itself (last operation: a product / a quotient)
        library centre (sigmoid + cell) * stride:                            the value itself
        demo centre (2 sigmoid - 0.5 + cell) * stride:                       max(2 sigmoid, 0.5, cell) * stride (the terms of the sum)
        letterboxed corner  clamp(ctr -+ half):                              max(centre, half), the centre taken before the pad is
                                                                             subtracted, max(|c|, |pad|) / ratio: that subtraction cancels
        RPN corner clamp(xc -+ w / 2), xc = d * anchor + cell:               max(|d * anchor|, cell, w / 2)
    The factor is streaming_measure.FACTOR for all of them; the strides are powers of two as the model's are (exact products).
  * The only discontinuity of decode is the demo variant's min_wh drop: a row whose float64 width or height lies within its own limit of
    min_wh may be excused from the objectness comparison, at most MAX_EXCUSED of a case's rows; MIN_SHARE of them must be dropped and
    MIN_SHARE kept.
  * Candidates, rank, NMS and the matchers are index and compare work: exact.  nms_restatement is built on oracle.detect.nms (stable
    descending order, IoU in fp32 in torchvision's expression order) with the kernels' parameters; class arg-max = first maximum.
"""
import numpy as np
import torch

import streaming_measure as sm
from oracle import detect as D
from oracle import rpn as R

F64, F32 = torch.float64, torch.float32
MAX_EXCUSED = 0.01
MIN_SHARE = 0.10


def f32(v):
    """a Python float as the C ABI receives it (c_float)"""
    return float(np.float32(v))


def below(v):
    """the next fp32 below v"""
    return float(np.nextafter(np.float32(v), np.float32(-np.inf)))


# ---- decode ------------------------------------------------------------------------------------------------------------------------------
def decode_rows(heads, anchors, strides, variant, letterbox, dt):
    """heads: per level [B, A, H, W, K] fp32; anchors: per level A pairs (w, h); letterbox: None or (resize_ratio, pad_left, pad_top, ori_w,
    ori_h, min_wh).  -> (rows [B, sum A*H*W, K], mag, extent): library rows in (a, y, x) order, demo rows in (y, x, a) order; extent
    [B, rows, 2] = the letterboxed width and height the min_wh test reads (None without a letterbox)."""
    outs, mags = [], []
    for h, anc, stride in zip(heads, anchors, strides):
        B, A, H, W, K = h.shape
        t = h.to(dt)
        anc = torch.tensor([[f32(a[0]), f32(a[1])] for a in anc], dtype=F64).to(dt).view(A, 1, 1, 2)
        stride = f32(stride)
        ys = torch.arange(H).view(H, 1).expand(H, W)
        xs = torch.arange(W).view(1, W).expand(H, W)
        cell = torch.stack([xs, ys], dim=2).to(dt)
        # the slices and the memory order are the oracle's: torch's fp32 sigmoid is not the same function on every code path (vector body
        # or scalar tail), and the fp32 instance of the library variant is pinned to the oracle bit for bit
        if variant == 0:
            o = torch.empty_like(t)
            o[..., 0:2] = (t[..., 0:2].sigmoid() + cell) * stride
            o[..., 2:4] = torch.exp(t[..., 2:4]) * anc
            o[..., 4:] = t[..., 4:].sigmoid()
            m = o.abs()
        else:
            t = t.permute(0, 1, 4, 2, 3).contiguous().permute(0, 3, 4, 1, 2)    # [B, H, W, A, K] over NCHW memory, as the demo's model emits it
            anc, cell = anc.view(1, 1, 1, A, 2), cell.view(1, H, W, 1, 2)
            o = torch.empty_like(t)
            s2 = torch.sigmoid(t[..., 0:2]) * 2
            o[..., 0:2] = (s2 - 0.5 + cell) * stride
            o[..., 2:4] = (torch.sigmoid(t[..., 2:4]) * 2) ** 2 * anc * stride
            o[..., 4:] = torch.sigmoid(t[..., 4:])
            m = o.abs()
            m[..., 0:2] = torch.maximum(torch.maximum(s2, torch.full_like(s2, 0.5)), cell.expand_as(s2)) * stride
        outs.append(o.reshape(B, -1, K))
        mags.append(m.reshape(B, -1, K))
    out, mag = torch.cat(outs, 1), torch.cat(mags, 1)
    if letterbox is None:
        return out, mag, None
    assert variant == 1
    rr, pl, pt, ow, oh, mn = (f32(v) for v in letterbox)
    pad, lim = torch.tensor([pl, pt], dtype=dt), torch.tensor([ow, oh], dtype=dt)
    ctr = torch.minimum(((out[..., 0:2] - pad) / rr).clamp_min(0), lim - 1)
    ext = torch.minimum((out[..., 2:4] / rr).clamp_min(0), lim)
    keep = (ext[..., 0] > mn) & (ext[..., 1] > mn)
    half = ext / 2
    res = out.clone()
    res[..., 0:2] = torch.minimum((ctr - half).clamp_min(0), lim - 1)
    res[..., 2:4] = torch.minimum((ctr + half).clamp_min(0), lim - 1)
    res[..., 4] = torch.where(keep, out[..., 4], torch.full_like(out[..., 4], -1.0))
    mg = torch.maximum(torch.maximum(out[..., 0:2].abs(), pad.abs().expand_as(half)) / rr, half.abs())
    mag = mag.clone()
    mag[..., 0:2] = mg
    mag[..., 2:4] = mg
    mag[..., 4] = torch.ones_like(mag[..., 4])
    return res, mag, ext


def decode_excused(ext64, ext32, min_wh):
    """rows whose float64 width or height lies within its limit of min_wh: which side of the drop they land on is not decided"""
    lim = sm.limit_of(ext64, ext32, ext64.abs())
    return ((ext64 - f32(min_wh)).abs() <= lim).any(dim=-1)


# name: (B, K, [(A, H, W, stride)]): nlevels 1, 2 and 4, A in {1, 5, 8} mixed, K in {6, 7, 85}; maps 3x7, 1x5, 5x1, 4x4: per_image is no
# multiple of 256, and the divisors A = 1 and W = 1 occur
DECODE_CASES = {
    'one_level_k6': (1, 6, [(1, 3, 7, 32)]),
    'two_levels_k7': (3, 7, [(5, 1, 5, 16), (8, 5, 1, 8)]),
    'four_levels_k85': (3, 85, [(1, 3, 7, 64), (5, 1, 5, 32), (8, 5, 1, 16), (5, 4, 4, 8)]),
    'four_levels_k6': (1, 6, [(8, 4, 4, 8), (1, 5, 1, 16), (5, 3, 7, 32), (8, 1, 5, 64)]),
}


def decode_case(name):
    """-> (heads, anchors, strides, letterbox): logits randn * 3 with a few rows planted at +-30 (both sigmoid tails, the largest extents)"""
    B, K, levels = DECODE_CASES[name]
    g = torch.Generator().manual_seed(sorted(DECODE_CASES).index(name) + 20250101)
    heads, anchors, strides = [], [], []
    for A, H, W, stride in levels:
        h = torch.randn(B, A, H, W, K, generator=g) * 3
        flat = h.view(-1, K)
        idx = torch.randperm(flat.size(0), generator=g)[:4]
        flat[idx[0::2]] = 30.0
        flat[idx[1::2]] = -30.0
        heads.append(h)
        anchors.append([(1.25 + 0.75 * a, 1.5 + 0.625 * ((3 * a) % 5)) for a in range(A)])
        strides.append(stride)
    in_w, in_h = max(W * s for _, _, W, s in levels), max(H * s for _, H, _, s in levels)
    rr, pl, pt = 0.8125, 4.0, 10.0
    letterbox = (rr, pl, pt, float(int((in_w - 2 * pl) / rr)), float(int((in_h - 2 * pt) / rr)), 5.0)
    return heads, anchors, strides, letterbox


def nhwc_view(h):
    """the [B, A, H, W, K] view of an NHWC buffer [B, H, W, A*K]: what the head kernels hand to decode"""
    B, A, H, W, K = h.shape
    buf = h.permute(0, 2, 3, 1, 4).reshape(B, H, W, A * K).contiguous()
    return buf.view(B, H, W, A, K).permute(0, 3, 1, 2, 4)


# ---- RPN row decode ----------------------------------------------------------------------------------------------------------------------
def rpn_rows(cls, d, base_wh, dt):
    """cls [B,H,W,A,2], d [B,H,W,A,4], base_wh [A,2] -> (rows [B, H*W*A, 6] = clamped xyxy, foreground score, 1; mag).  Both extents use
    exp(d[2]) as rpn.py:118-119 does."""
    B, H, W, A = cls.shape[:4]
    an = R.make_anchors_xywh(torch.as_tensor(base_wh, dtype=F32), H, W).to(dt)
    t, c = d.to(dt), cls.to(dt)
    px, py = t[..., 0] * an[..., 2], t[..., 1] * an[..., 3]
    xc, yc = px + an[..., 0], py + an[..., 1]
    e = torch.exp(t[..., 2])
    w, h = e * an[..., 2], e * an[..., 3]
    score = torch.softmax(c, dim=4)[..., 1]
    one = torch.ones_like(score)
    rows = torch.stack([(xc - w / 2).clamp(0, W - 1), (yc - h / 2).clamp(0, H - 1), (xc + w / 2).clamp(0, W - 1), (yc + h / 2).clamp(0, H - 1),
                        score, one], dim=-1)
    mx = torch.maximum(torch.maximum(px.abs(), an[..., 0].expand_as(px)), (w / 2).abs())
    my = torch.maximum(torch.maximum(py.abs(), an[..., 1].expand_as(py)), (h / 2).abs())
    mag = torch.stack([mx, my, mx, my, score, one], dim=-1)
    return rows.reshape(B, -1, 6), mag.reshape(B, -1, 6)


def rpn_case(H, W, A, B=2, seed=0):
    g = torch.Generator().manual_seed(7000 + seed + A)
    cls = torch.randn(B, H, W, A, 2, generator=g) * 3
    d = torch.randn(B, H, W, A, 4, generator=g) * 0.7
    cls.view(-1, 2)[0] = torch.tensor([30.0, -30.0])
    cls.view(-1, 2)[1] = torch.tensor([-30.0, 30.0])
    base = torch.tensor([[1.5 + 0.75 * a, 1.0 + 0.5 * ((2 * a) % 7)] for a in range(A)])
    return cls, d, base


def rpn_tie_case():
    """130 rows (5 x 13 cells, 2 anchors); ten rows share one pair of logits, and 60 rows score above them: the tie lies across places 61..70
    of the ranking, so pre_nms_top_n = 64 and 65 both cut through it.  -> (cls, d, base, tied rows)"""
    H, W, A = 5, 13, 2
    g = torch.Generator().manual_seed(7130)
    n = H * W * A
    perm = torch.randperm(n, generator=g)
    logit = torch.empty(n)
    logit[perm[:60]] = 1.0 + torch.rand(60, generator=g) * 3
    logit[perm[60:70]] = 0.5
    logit[perm[70:]] = -3.0 + torch.rand(n - 70, generator=g) * 3
    cls = torch.stack([torch.zeros(n), logit], 1).view(1, H, W, A, 2)
    d = (torch.randn(1, H, W, A, 4, generator=g) * 0.5)
    base = torch.tensor([[2.5, 1.5], [1.5, 3.0]])
    return cls, d, base, torch.sort(perm[60:70])[0]


def proposals_from_rows(rows, pre_nms_top_n, post_nms_top_n, nms_thresh):
    """filter_proposals from the decoded rows of ONE image [n, 6] on: the pre_nms_top_n best in stable order (lower row first), NMS, the first
    post_nms_top_n, xyxy -> xywh.  -> (xywh [m, 4], source rows [m])"""
    n = rows.size(0)
    det, src = nms_restatement(rows, -1.0, nms_thresh, min(post_nms_top_n, n), box_mode=1, score_mode=1, rethreshold=0, class_gap=0.0,
                               max_nms=min(pre_nms_top_n, n))
    x = det[:, :4]
    return torch.stack([(x[:, 0] + x[:, 2]) / 2, (x[:, 1] + x[:, 3]) / 2, x[:, 2] - x[:, 0], x[:, 3] - x[:, 1]], dim=1), src


# ---- candidates, rank, NMS ---------------------------------------------------------------------------------------------------------------
def nms_restatement(pred, conf_thres, iou_thres, max_det, box_mode, score_mode, rethreshold, class_gap, max_nms):
    """One image's rows [R, K] fp32 -> (detections [n, 6] = xyxy, score, category; source rows [n]), as fva_nms_candidates + fva_nms_select
    define them: candidates are the rows with objectness > conf_thres in row order; category = FIRST maximum of cls * obj; score = that
    maximum (score_mode 0) or the objectness (1); rethreshold drops candidates whose best product is not > conf_thres; of more than max_nms
    (> 0) candidates the max_nms best stay, stable; boxes are offset by category * class_gap for the suppression only."""
    pred = pred.detach().float().cpu()
    conf = np.float32(conf_thres)
    obj = pred[:, 4].numpy()
    rows = np.nonzero(obj > conf)[0]
    p = pred[rows]
    prod = (p[:, 5:] * p[:, 4:5]).numpy()
    cat = prod.argmax(axis=1) if len(rows) else np.zeros(0, np.int64)              # numpy: the first occurrence of the maximum
    best = prod[np.arange(len(rows)), cat] if len(rows) else np.zeros(0, np.float32)
    if rethreshold:
        ok = best > conf
        rows, p, cat, best = rows[ok], p[torch.from_numpy(ok)], cat[ok], best[ok]
    score = torch.from_numpy(best.astype(np.float32)) if score_mode == 0 else p[:, 4].clone()
    boxes = D.xywh2xyxy(p[:, :4]) if box_mode == 0 else p[:, :4].clone()
    catf = torch.from_numpy(cat.astype(np.float32))
    rows = torch.from_numpy(rows.astype(np.int64))
    if max_nms > 0 and rows.numel() > max_nms:
        order = torch.from_numpy(np.argsort(-score.numpy(), kind='stable')[:max_nms].copy())
        rows, boxes, score, catf = rows[order], boxes[order], score[order], catf[order]
    keep = D.nms(boxes + catf[:, None] * np.float32(class_gap), score, iou_thres)[:max_det]
    return torch.cat([boxes[keep], score[keep, None], catf[keep, None]], dim=1).view(-1, 6), rows[keep]


def apart_xywh(n):
    """n boxes of 4 x 4 on a 10-pixel grid: no two overlap"""
    i = torch.arange(n)
    return torch.stack([10.0 * (i % 100) + 5, 10.0 * (i // 100) + 5, torch.full((n,), 4.0), torch.full((n,), 4.0)], 1)


def apart_xyxy(n, x0=1000.0):
    b = apart_xywh(n)
    return torch.stack([b[:, 0] - 2 + x0, b[:, 1] - 2, b[:, 0] + 2 + x0, b[:, 1] + 2], 1)


CONF = 0.25
CLASS_TIES = ((3, 4), (2, 66), (63, 64))          # neighbouring lanes; one lane, two rounds of its class loop; last lane against lane 0 of the next round


def class_ties_for(C):
    return [t for t in CLASS_TIES if t[1] < C] + ([(0, 1)] if C == 2 else [])


def candidate_case(R, C, seed=0):
    """[3, R, 5 + C]: boxes that overlap nothing; image 1 has no candidate (every objectness <= CONF, some exactly CONF) between two images
    that have some.  Candidates are about half of the rows and always the rows at the seams of a 64-row wave and a 1024-row round that exist.
    Planted in images 0 and 2: class ties (two bit-equal products that are the row's maximum), objectness exactly CONF (no candidate), and
    best product exactly CONF with objectness 0.5 (a candidate that rethreshold = 1 drops).
    -> (pred, info) with info = dict(ties=[(image, row, c_low, c_high)], at_conf=[(image, row)], best_at_conf=[(image, row)])"""
    g = torch.Generator().manual_seed(1000 * C + R + seed)
    pred = torch.empty(3, R, 5 + C)
    pred[..., 0:4] = apart_xywh(R)
    pred[..., 5:] = 0.3 + 0.6 * torch.rand(3, R, C, generator=g)
    cand = torch.rand(3, R, generator=g) < 0.5
    for r in (0, 62, 63, 64, 65, 1023, 1024, 1025, R - 1):
        if r < R:
            cand[:, r] = True
    obj = torch.where(cand, 0.45 + 0.5 * torch.rand(3, R, generator=g), CONF * torch.rand(3, R, generator=g))
    obj[1] = CONF * torch.rand(R, generator=g)
    obj[1, ::3] = CONF
    pred[..., 4] = obj
    info = dict(ties=[], at_conf=[], best_at_conf=[])
    free = [r for r in range(R) if r not in (0, 63, 64, R - 1)] or [0]
    picks = iter(free[::max(1, len(free) // 12)] + free)
    for b in (0, 2):
        if R == 1:
            if C >= 2 and b == 0:
                lo, hi = class_ties_for(C)[0]
                pred[b, 0, 4] = 0.75
                pred[b, 0, 5 + lo] = pred[b, 0, 5 + hi] = 0.96875
                info['ties'].append((b, 0, lo, hi))
            continue
        for lo, hi in class_ties_for(C):
            r = next(picks)
            pred[b, r, 4] = 0.75
            pred[b, r, 5 + lo] = pred[b, r, 5 + hi] = 0.96875
            info['ties'].append((b, r, lo, hi))
        r = next(picks)
        pred[b, r, 4] = CONF
        info['at_conf'].append((b, r))
        r = next(picks)
        pred[b, r, 4] = 0.5
        pred[b, r, 5:] = 0.25 + 0.2 * torch.rand(C, generator=g)
        pred[b, r, 5 + (C - 1) // 2] = 0.5
        info['best_at_conf'].append((b, r))
    return pred, info


def score_rows(scores, boxes_xyxy, cats=None, C=1):
    """[n, 5 + C] rows for box_mode = 1, score_mode = 1: the NMS score is the objectness, every row a candidate at conf_thres = 0 (scores
    must be > 0), candidate index = row; cats: the category of each row (its class score is 1, the others 0.5)"""
    n = scores.numel()
    p = torch.full((n, 5 + C), 0.5)
    p[:, 0:4] = boxes_xyxy
    p[:, 4] = scores
    cats = torch.zeros(n, dtype=torch.int64) if cats is None else cats
    p[torch.arange(n), 5 + cats] = 1.0
    return p


def distinct_scores(n, seed):
    """n different scores in (0.1, 0.9) in a shuffled order"""
    g = torch.Generator().manual_seed(seed)
    return (0.1 + 0.8 * (torch.arange(n, dtype=F32) + 0.5) / n)[torch.randperm(n, generator=g)]


RANK_TIES = ((0, 255, 256, 257), (63, 64))        # across the 256-entry tile of rank_kernel and inside it; across a 64-row wave


def rank_case(n, tied=True):
    """n candidates that overlap nothing, different scores, except (tied) one score shared by the indices RANK_TIES[0] that exist -- the highest
    -- and another, the lowest, by RANK_TIES[1]; -> (rows [n, 6], groups of tied indices with at least two members)"""
    s = distinct_scores(n, 300 + n)
    groups = []
    if tied:
        for grp, val in zip(RANK_TIES, (0.95, 0.05)):
            idx = [i for i in grp if i < n]
            if len(idx) >= 2:
                s[idx] = val
                groups.append(idx)
    return score_rows(s, apart_xyxy(n)), groups


def all_equal_case(n=300):
    return score_rows(torch.full((n,), 0.625), apart_xyxy(n))


# pairs whose fp32 IoU is exactly the value: inter / (area_a + area_b - inter) = 2 / (4 + 2 - 2), 12 / (16 + 12 - 12)
IOU_PAIRS = ((0.5, (0.0, 0.0, 2.0, 2.0), (0.0, 0.0, 2.0, 1.0)), (0.75, (8.0, 8.0, 12.0, 12.0), (8.0, 8.0, 12.0, 11.0)))


def iou_f32(a, b):
    """torchvision's expression in fp32 (what overlaps() compares with the threshold)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    w = max(np.float32(0), min(a[2], b[2]) - max(a[0], b[0]))
    h = max(np.float32(0), min(a[3], b[3]) - max(a[1], b[1]))
    inter = np.float32(w * h)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.float32(inter / np.float32(np.float32((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1])) - inter))


def pair_case(pair, with_gap, n=70):
    """the pair at the candidate indices 3 and 66 with the two best scores: ranks 0 and 1, neighbours in one diagonal block of the mask; a
    second copy of the pair, shifted by 100 pixels, gets the ranks 2 and n - 1 (column block 1 against row block 0).  The rest overlaps
    nothing.  with_gap: three classes, both boxes of a pair in class 1, so class_gap = 4096 is added to every coordinate of theirs.
    -> (rows, dict of the four indices)"""
    _, a, b = pair
    s = distinct_scores(n, 17)
    boxes = apart_xyxy(n)
    order = torch.argsort(s, descending=True)
    hi = s.max().item()
    idx = dict(a1=3, b1=66, a2=40, b2=int(order[-1]))
    s[idx['a1']], s[idx['b1']], s[idx['a2']] = hi + 0.03, hi + 0.02, hi + 0.01
    off = torch.tensor([100.0, 0.0, 100.0, 0.0])
    boxes[idx['a1']], boxes[idx['b1']] = torch.tensor(a), torch.tensor(b)
    boxes[idx['a2']], boxes[idx['b2']] = torch.tensor(a) + off, torch.tensor(b) + off
    cats = None
    if with_gap:
        cats = torch.arange(n) % 3
        for k in idx.values():
            cats[k] = 1
    return score_rows(s, boxes, cats, C=3 if with_gap else 1), idx


def zero_area_case(n=140):
    """zero-area boxes: a point twice (IoU 0 / 0), a point inside a large box, a flat line over a box, with scores above, between and below
    their partners: none is suppressed, none suppresses.  -> (rows, indices of everything that must be kept = all)"""
    s = distinct_scores(n, 23)
    boxes = apart_xyxy(n)
    big = torch.tensor([0.0, 0.0, 20.0, 20.0])
    boxes[1] = torch.tensor([5.0, 5.0, 5.0, 5.0])
    boxes[70] = torch.tensor([5.0, 5.0, 5.0, 5.0])
    boxes[2] = big
    boxes[130] = torch.tensor([0.0, 10.0, 20.0, 10.0])
    boxes[65] = torch.tensor([50.0, 50.0, 50.0, 60.0])
    boxes[66] = torch.tensor([50.0, 50.0, 50.0, 60.0])
    s[1], s[2], s[70], s[130] = 0.99, 0.98, 0.05, 0.04
    return score_rows(s, boxes)


CHAIN_A, CHAIN_B, CHAIN_C = (0.0, 0.0, 10.0, 10.0), (0.0, 2.0, 10.0, 12.0), (0.0, 4.0, 10.0, 14.0)


def chain_case(n=200):
    """a suppresses b (IoU 2/3), b would suppress c (2/3), a does not (3/7): with a, b, c at ranks 0, 70 and 140 -- three 64-blocks -- c
    survives.  -> (rows, (ia, ib, ic))"""
    s = distinct_scores(n, 29)
    order = torch.argsort(s, descending=True)
    ia, ib, ic = int(order[0]), int(order[70]), int(order[140])
    boxes = apart_xyxy(n)
    boxes[ia], boxes[ib], boxes[ic] = torch.tensor(CHAIN_A), torch.tensor(CHAIN_B), torch.tensor(CHAIN_C)
    return score_rows(s, boxes), (ia, ib, ic)


def clusters_case(n, seed):
    """overlapping boxes in a few clusters, different scores: suppression across every pair of 64-blocks"""
    g = torch.Generator().manual_seed(seed)
    centre = torch.rand(8, 2, generator=g) * 200
    which = torch.randint(0, 8, (n,), generator=g)
    c = centre[which] + torch.randn(n, 2, generator=g) * 4
    wh = 20 + torch.rand(n, 2, generator=g) * 10
    boxes = torch.cat([c - wh / 2, c + wh / 2], 1)
    return score_rows(distinct_scores(n, seed + 1), boxes)


def max_nms_case(n=130):
    """130 candidates; the scores at places 63..66 of the ranking are one value and those at places 99..101 another, their indices scattered:
    max_nms = 64, 65 and 100 all cut through a tie.  Clustered boxes, so NMS has work to do -- but the tied boxes stand apart, so which of
    them passed the cut shows in the result.  -> rows"""
    p = clusters_case(n, 41)
    s = p[:, 4].clone()
    order = torch.argsort(s, descending=True)
    s[order[62:66]] = s[order[62]].item()
    s[order[98:101]] = s[order[98]].item()
    p[:, 4] = s
    tied = torch.cat([order[62:66], order[98:101]])
    p[tied, 0:4] = apart_xyxy(n)[tied]
    return p


# ---- matchers ----------------------------------------------------------------------------------------------------------------------------
FH, FW = 8, 16                                    # powers of two: the scaling of the normalised boxes is exact
MATCH_TIES = ((5, 69), (0, 256))                  # identical anchors: across a wave, and across the 256-thread stride of the arg-max


def match_case(Na, T, seed=0):
    """anchors [Na, 4] xywh in the left 12 cells of an 8 x 16 map and T boxes of image 0 (normalised xywh, [T, 6]).  Where the indices exist,
    box 0 lies inside the identical anchors MATCH_TIES[0] and box 1 inside MATCH_TIES[1], far from everything else, IoU 0.25: below any
    neg_thr, so only the claim of the best anchor shows which of the two won.  The last box of T = 5 repeats box 2.
    -> (anchors, targets, [(box, first anchor, second anchor)])"""
    g = torch.Generator().manual_seed(500 + 10 * Na + T + seed)
    q = 0.0625
    cxy = torch.round(torch.rand(Na, 2, generator=g) * torch.tensor([9.0, 6.0]) / q) * q + 1
    wh = torch.round((0.5 + torch.rand(Na, 2, generator=g) * 2.5) / q) * q
    anchors = torch.cat([cxy, wh], 1)
    txy = torch.round(torch.rand(T, 2, generator=g) * torch.tensor([9.0, 6.0]) / q) * q + 1
    twh = torch.round((0.5 + torch.rand(T, 2, generator=g) * 2.5) / q) * q
    ties = []
    spots = ((14.0, 2.0), (14.0, 6.0))
    for t, ((i, j), (sx, sy)) in enumerate(zip(MATCH_TIES, spots)):
        if j < Na and t < T:
            anchors[i] = anchors[j] = torch.tensor([sx, sy, 2.0, 2.0])
            txy[t], twh[t] = torch.tensor([sx + 0.5, sy + 0.5]), torch.tensor([1.0, 1.0])
            ties.append((t, i, j))
    if Na == 1:                                   # the only anchor overlaps box 0, so there is an IoU to put the thresholds on
        txy[0], twh[0] = anchors[0, :2] + 0.25, anchors[0, 2:]
    if T == 5:
        txy[4], twh[4] = txy[2], twh[2]
    targets = torch.cat([torch.zeros(T, 2), txy / torch.tensor([float(FW), float(FH)]), twh / torch.tensor([float(FW), float(FH)])], 1)
    return anchors, targets, ties


def match_iou(anchors, targets):
    """the fp32 IoU matrix [Na, T] the RPN matcher compares (boxes scaled by the map size)"""
    return R.batch_iou(anchors, targets[:, 2:] * torch.tensor([FW, FH, FW, FH], dtype=F32))


def pick_threshold(best, lo, hi):
    """an fp32 value that occurs in best, the one nearest the middle of (lo, hi) among those strictly inside (0, 1)"""
    b = best[(best > 0) & (best < 1)]
    return float(b[(b - (lo + hi) / 2).abs().argmin()])


def match_thresholds(anchors, targets):
    """thresholds that ARE the best IoU of some anchor no box claims (of any anchor where every one is claimed): pos near 0.65, neg near
    0.45, floor near 0.15 as far as the case has such values; the tests put the other thresholds out of the way of the one on trial"""
    iou = match_iou(anchors, targets)
    best = iou.max(dim=1).values
    free = torch.ones_like(best, dtype=torch.bool)
    free[iou.argmax(dim=0)] = False
    if not ((best > 0) & (best < 1) & free).any():
        free[:] = True
    best = best[free]
    return dict(pos=pick_threshold(best, 0.35, 0.95), neg=pick_threshold(best, 0.3, 0.6), floor=pick_threshold(best, 0.02, 0.3))


def fast_targets(targets):
    """the same boxes as the Fast head gets them: xywh in feature cells"""
    t = targets.clone()
    t[:, 2:] = targets[:, 2:] * torch.tensor([FW, FH, FW, FH], dtype=F32)
    return t
