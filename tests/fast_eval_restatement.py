"""The reference of tests/test_gpu_fast_eval.py: what fva_fast_decode (csrc/detect.hip) computes, written in float64 torch from the reference's
own lines -- the eval branch of Fast.forward after the heads (demos/faster_rcnn/models/fast.py:93-101,265-286) and postProcess up to its NMS
call (demos/faster_rcnn/inference.py:87-118 = inference_voc_test.py:61-80).  Not a test module (pytest does not collect it);
tests/test_fast_eval_restatement_cpu.py pins it without a GPU.

Per live row, in this order (the constants are the fp32 ones the kernel multiplies by, the arithmetic is float64):
  1. m = first index of the maximum LOGIT (torch.max(predict_cls), fast.py:266); d = box[m*4 .. m*4+3] with the multi-reg head, else box[0..3]
  2. d *= (0.1, 0.1, 0.2, 0.2)
  3. x = d0*pw + px, y = d1*ph + py, w = exp(d2)*pw, h = exp(d2)*ph            (d2 for BOTH sizes: fast.py:98-99)
  4. p = softmax(logits); score = max p, cat = FIRST index of the maximum; cat == 0 (background, ties with it included) drops the row
  5. xywh *= stride
  6. x = clamp((x - pad_left) / ratio, 0, bound_w - 1), y likewise, w = clamp(w / ratio, 0, bound_w), h likewise (inference.py:92-101); without a
     letterbox ratio 1, pads 0 and the bounds are the network input's
  7. dropped unless w > min_wh and h > min_wh (:103)
  8. x1, x2 = clamp(x -+ w/2, 0, bound_w - 1), y1, y2 likewise (:106-110)
  9. row = x1, y1, x2, y2, score, one-hot(cat - 1); a dropped row -- and every padding row r >= n_b -- is 0, 0, 0, 0, -1, 0, ...

The limits, U = 2^-24 (half an ulp of fp32, the relative error of one rounding); they come from the fp32 operation chain alone, nothing is
fitted to an output.  s = stride / ratio, a = d0 * pw (x axis; d1 * ph on y):
  centre   six roundings -- d0*0.1f, *pw, +px, *stride, -pad, /ratio -- each at most U times the magnitude of its result carried into the
           final frame, and every one of those magnitudes is at most Mc = s * (|a| + |px|) + |pad| / ratio:          lim_c = 6 U Mc
           (clamps are exact and 1-Lipschitz: they never enlarge an error)
  size     d2*0.2f is rounded (U |t2| in the argument = U |t2| relative after exp), expf is documented at 1 ulp = 2 U relative, then three
           products / quotients (*pw, *stride, /ratio):                                                      lim_w = (5 + |t2|) U w
  corner   x -+ w/2 (the halving is exact) adds one rounding of a result of at most |x| + w/2:   lim_x1 = lim_c + lim_w / 2 + U (|x| + w/2)
  prob.    e_c = expf(z_c - max z): the subtraction's rounding U |z_c - max| becomes U |z_c - max| e_c <= U / e (t exp(-t) <= 1/e), expf adds
           2 U e_c; the sum S >= 1 of n = C + 1 terms, in ANY order, carries at most (n - 1) U S on top of its terms' errors n U / e + 2 U S;
           the quotient one more U.  With S >= 1:                                           lim_p(p) = U (1/e + p (n (1 + 1/e) + 4))
  score    lim_p(score); the decision between the two largest probabilities: lim_gap = lim_p(p1) + lim_p(p2).
A row's drop / category decision is compared exactly unless one of its margins -- p1 - p2, |w - min_wh|, |h - min_wh| -- is inside its limit;
the case generator redraws every row with a margin under MARGIN_FACTOR x its limit, so for its inputs the number of rows left out is ZERO.
"""
import math

import numpy as np
import torch

F64 = torch.float64
U = 2.0 ** -24
MARGIN_FACTOR = 64.0
STD = tuple(float(np.float32(v)) for v in (0.1, 0.1, 0.2, 0.2))        # the kernel's fp32 constants


def f32(v):
    """a Python float as the C ABI receives it (c_float)"""
    return float(np.float32(v))


def lim_p(p, n):
    return U * (1.0 / math.e + p * (n * (1.0 + 1.0 / math.e) + 4.0))


def restate(cls, box, proposals, counts, R, multi_reg, stride, input_hw, min_wh=5.0, letterboxes=None, mutant=None):
    """cls [K, C+1], box [K, 4 or (C+1)*4], proposals [K, 4] fp32 (CPU), image after image; counts: rows per image (host list); letterboxes: None
    or per image (resize_ratio, pad_left, pad_top, ori_w, ori_h).  -> dict of float64 / bool tensors over the padded [B, R] grid:
      rows [B,R,5+C]; live (a source row exists); drop; cat (1-based, 0 = background); gap, wm, hm (the margins: p1 - p2, w - min_wh,
      h - min_wh); lim_box [B,R,4], lim_score, lim_gap, lim_w, lim_h.
    mutant: None | 'h_uses_d3' (h = exp(d3) * ph) | 'cat_excludes_bg' (category = arg-max of the foreground logits, never background)."""
    K, C1 = cls.shape
    C, B = C1 - 1, len(counts)
    assert sum(counts) == K and max(counts) <= R
    z = cls.to(F64)
    m = z.argmax(dim=1)                                                   # first maximum
    d = box.to(F64).view(K, -1, 4)[torch.arange(K), m] if multi_reg else box.to(F64)
    d = d * torch.tensor(STD, dtype=F64)
    p = proposals.to(F64)
    px, py, pw, ph = p[:, 0], p[:, 1], p[:, 2], p[:, 3]
    ax, ay = d[:, 0] * pw, d[:, 1] * ph
    ew = torch.exp(d[:, 2])
    eh = torch.exp(d[:, 3]) if mutant == 'h_uses_d3' else ew
    t2w, t2h = d[:, 2].abs(), (d[:, 3] if mutant == 'h_uses_d3' else d[:, 2]).abs()
    zmax = z.max(dim=1, keepdim=True).values
    e = torch.exp(z - zmax)
    prob = e / e.sum(dim=1, keepdim=True)
    score, cat = prob.max(dim=1)                                          # first maximum
    if mutant == 'cat_excludes_bg':
        cat = 1 + z[:, 1:].argmax(dim=1)
        score = prob[torch.arange(K), cat]
    top2 = prob.topk(2, dim=1).values
    gap = top2[:, 0] - top2[:, 1]
    img = torch.repeat_interleave(torch.arange(B), torch.tensor(counts))
    if letterboxes is None:
        frame = torch.tensor([[1.0, 0.0, 0.0, f32(input_hw[1]), f32(input_hw[0])]] * B, dtype=F64)
    else:
        frame = torch.tensor([[f32(v) for v in one[:5]] for one in letterboxes], dtype=F64)
    ratio, pl, pt, bw, bh = (frame[img, q] for q in range(5))
    st, mn = f32(stride), f32(min_wh)
    x = torch.minimum((((ax + px) * st - pl) / ratio).clamp_min(0), bw - 1)
    y = torch.minimum((((ay + py) * st - pt) / ratio).clamp_min(0), bh - 1)
    w_raw, h_raw = ew * pw * st / ratio, eh * ph * st / ratio
    w, h = torch.minimum(w_raw.clamp_min(0), bw), torch.minimum(h_raw.clamp_min(0), bh)
    drop = (cat == 0) | ~((w > mn) & (h > mn))
    x1 = torch.minimum((x - w / 2).clamp_min(0), bw - 1)
    y1 = torch.minimum((y - h / 2).clamp_min(0), bh - 1)
    x2 = torch.minimum((x + w / 2).clamp_min(0), bw - 1)
    y2 = torch.minimum((y + h / 2).clamp_min(0), bh - 1)
    rows = torch.zeros(K, 5 + C, dtype=F64)
    rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3], rows[:, 4] = x1, y1, x2, y2, score
    rows[torch.arange(K), 5 + (cat - 1).clamp_min(0)] = 1.0
    rows[drop] = 0.0
    rows[drop, 4] = -1.0
    # limits
    s = st / ratio
    lim_cx = 6 * U * (s * (ax.abs() + px.abs()) + pl.abs() / ratio)
    lim_cy = 6 * U * (s * (ay.abs() + py.abs()) + pt.abs() / ratio)
    lim_w, lim_h = (5 + t2w) * U * w_raw.abs(), (5 + t2h) * U * h_raw.abs()
    lim_x = lim_cx + lim_w / 2 + U * (x.abs() + w / 2)
    lim_y = lim_cy + lim_h / 2 + U * (y.abs() + h / 2)
    lim_box = torch.stack([lim_x, lim_y, lim_x, lim_y], dim=1)
    lim_score = lim_p(score, C1)
    lim_gap = lim_p(top2[:, 0], C1) + lim_p(top2[:, 1], C1)

    def pad(v, fill):
        out = torch.full((B, R) + tuple(v.shape[1:]), fill, dtype=v.dtype)
        start = 0
        for b, n in enumerate(counts):
            out[b, :n] = v[start:start + n]
            start += n
        return out
    res = dict(rows=pad(rows, 0.0), live=pad(torch.ones(K, dtype=torch.bool), False), drop=pad(drop, True), cat=pad(cat, 0),
               gap=pad(gap, math.inf), wm=pad(w - mn, math.inf), hm=pad(h - mn, math.inf), lim_box=pad(lim_box, 0.0),
               lim_score=pad(lim_score, 0.0), lim_gap=pad(lim_gap, 0.0), lim_w=pad(lim_w, 0.0), lim_h=pad(lim_h, 0.0),
               src=pad(torch.arange(K), -1))
    res['rows'][~res['live'], 4] = -1.0
    return res


def undecided(ref, factor=1.0):
    """live rows with a margin inside factor x its limit: which side of the drop / which category they land on is not decided.  The size
    margins count only where the category test lets the row through."""
    size = ((ref['wm'].abs() <= factor * ref['lim_w']) | (ref['hm'].abs() <= factor * ref['lim_h'])) & (ref['cat'] > 0)
    return ref['live'] & ((ref['gap'] <= factor * ref['lim_gap']) | size)


def compare(got, ref, exact=None):
    """got [B, R, 5+C] fp32 against restate()'s dict.  Every row outside ``undecided`` -- and every row of ``exact`` ([B,R] bool: hand-built
    rows whose arithmetic is exact) -- must agree in its drop decision and its category bit for bit; a dropped row must be exactly
    0, 0, 0, 0, -1, 0, ...; the four corners and the score of a kept row must lie within their limits.
    -> dict(excused, decisions (rows whose decision differs), worst_box, worst_score (largest err / limit), pattern (dropped rows not in the
    dropped pattern))."""
    got = got.detach().cpu().to(F64)
    want = ref['rows']
    assert got.shape == want.shape, (got.shape, want.shape)
    excused = undecided(ref)
    if exact is not None:
        excused = excused & ~exact
    got_drop = got[..., 4] == -1.0
    dropped_pattern = torch.zeros_like(got[0, 0])
    dropped_pattern[4] = -1.0
    pattern = int((got_drop & (got != dropped_pattern).any(dim=-1)).sum())
    finite = torch.isfinite(got).all(dim=-1)
    checked = ~excused
    wrong = checked & ((got_drop != ref['drop']) | (~ref['drop'] & (got[..., 5:] != want[..., 5:]).any(dim=-1)) | ~finite)
    both = checked & ~ref['drop'] & ~got_drop & finite
    ratio_box = (got[..., :4] - want[..., :4]).abs() / ref['lim_box'].clamp_min(1e-300)
    ratio_score = (got[..., 4] - want[..., 4]).abs() / ref['lim_score'].clamp_min(1e-300)
    return dict(excused=int(excused.sum()), decisions=int(wrong.sum()), pattern=pattern,
                worst_box=float(ratio_box[both].max()) if both.any() else 0.0,
                worst_score=float(ratio_score[both].max()) if both.any() else 0.0, kept=int(both.sum()))


def check(got, ref, exact=None, what=''):
    rep = compare(got, ref, exact)
    print(what, rep)
    assert rep['excused'] == 0, (what, rep)
    assert rep['decisions'] == 0 and rep['pattern'] == 0, (what, rep)
    assert rep['worst_box'] <= 1.0 and rep['worst_score'] <= 1.0, (what, rep)
    return rep


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
# per-image letterboxes of the three-image cases: distinct ratios and pads, the second image wider than tall, the third taller than wide
LETTERBOXES = [(0.8, 0.0, 24.0, 160.0, 100.0), (0.5, 0.0, 32.0, 256.0, 128.0), (1.25, 19.0, 0.0, 72.0, 102.0)]
INPUT_HW = (128, 128)
STRIDE = 16.0


def _draw(g, K, C, multi_reg, fw, fh):
    z = torch.randn(K, C + 1, generator=g) * 3
    big = torch.rand(K, generator=g) < 0.15                               # logits up to +-80: exp(z - max) must not overflow
    z[big] = torch.rand(K, C + 1, generator=g)[big] * 160.0 - 80.0
    bg = torch.rand(K, generator=g) < 0.3                                 # a background share at every C
    z[bg, 0] += 12.0
    d = torch.randn(K, (C + 1) * 4 if multi_reg else 4, generator=g) * 1.5
    xy = torch.rand(K, 2, generator=g) * torch.tensor([float(fw), float(fh)])
    wh = torch.exp(torch.rand(K, 2, generator=g) * math.log(40.0)) * 0.15  # 0.15 .. 6 cells: both sides of min_wh = 5 px at stride 16
    return z, d, torch.cat([xy, wh], 1)


def make_case(seed, C, multi_reg, counts, R, letterboxes=None, stride=STRIDE, input_hw=INPUT_HW, min_wh=5.0):
    """Random head outputs for ``counts`` rows per image; every row whose margin is under MARGIN_FACTOR x its limit is redrawn, so that
    ``undecided`` is empty by construction.  -> (cls, box, proposals, ref)."""
    g = torch.Generator().manual_seed(seed)
    K = sum(counts)
    fw, fh = input_hw[1] / stride, input_hw[0] / stride
    z, d, p = _draw(g, K, C, multi_reg, fw, fh)
    for _ in range(100):
        ref = restate(z, d, p, counts, R, multi_reg, stride, input_hw, min_wh, letterboxes)
        close = undecided(ref, MARGIN_FACTOR)
        if not close.any():
            return z, d, p, ref
        idx = ref['src'][close]
        nz, nd, np_ = _draw(g, idx.numel(), C, multi_reg, fw, fh)
        z[idx], d[idx], p[idx] = nz, nd, np_
    raise AssertionError('make_case: rows kept landing next to a decision boundary')


def hand_rows():
    """Hand-worked rows in exact arithmetic: C = 3, single-reg head, ONE image with letterbox ratio 0.5 (a power of two), stride 16, no pads,
    original image 4096 x 4096 (no clamp is active), min_wh 5.  With d2 = 0: w = pw * 32, h = ph * 32, exactly.
    -> (cls, box, proposals, counts, letterboxes, expected) with expected = list of (dropped, category or None, what)."""
    up = float(np.nextafter(np.float32(5.0), np.float32(6.0)))
    rows = [
        # logits (bg, c1, c2, c3)      box deltas             proposal xywh
        ([0.0, 2.0, 1.0, 0.0], [0.0, 0.0, 1.5, -2.0], [10.0, 20.0, 2.0, 3.0], (False, 0, 'exp(d2) twice: d3 = -2 is ignored, w / h = 2 / 3')),
        ([3.0, 3.0, 1.0, 0.0], [0.0, 0.0, 0.0, 0.0], [10.0, 20.0, 2.0, 3.0], (True, None, 'background ties with class 1: dropped')),
        ([0.0, 1.0, 4.0, 4.0], [0.0, 0.0, 0.0, 0.0], [10.0, 20.0, 2.0, 3.0], (False, 1, 'classes 2 and 3 tie: the lower one')),
        ([0.0, 5.0, 1.0, 0.0], [0.0, 0.0, 0.0, 0.0], [10.0, 20.0, 5.0 / 32, 1.0], (True, None, 'w == 5.0 exactly: dropped')),
        ([0.0, 5.0, 1.0, 0.0], [0.0, 0.0, 0.0, 0.0], [10.0, 20.0, up / 32, 1.0], (False, 0, 'w == nextafter(5, 6): kept')),
        ([0.0, 5.0, 1.0, 0.0], [0.0, 0.0, 0.0, 0.0], [10.0, 20.0, 1.0, 5.0 / 32], (True, None, 'h == 5.0 exactly: dropped')),
        ([0.0, 5.0, 1.0, 0.0], [0.0, 0.0, 0.0, 0.0], [10.0, 20.0, 1.0, up / 32], (False, 0, 'h == nextafter(5, 6): kept')),
    ]
    cls = torch.tensor([r[0] for r in rows], dtype=torch.float32)
    box = torch.tensor([r[1] for r in rows], dtype=torch.float32)
    prop = torch.tensor([r[2] for r in rows], dtype=torch.float32)
    return cls, box, prop, [len(rows)], [(0.5, 0.0, 0.0, 4096.0, 4096.0)], [r[3] for r in rows]


# the GPU cases: name -> (seed, C, multi_reg, counts, R, letterboxed)
CASES = {}
for _C in (1, 20, 80):
    for _mr in (False, True):
        for _lb in (False, True):
            CASES[f'c{_C}_{"multi" if _mr else "single"}_{"lb" if _lb else "input"}'] = (20260000 + len(CASES), _C, _mr, (0, 1, 70), 80, _lb)
CASES['k1'] = (20260100, 20, False, (1,), 1, False)


def case(name):
    seed, C, multi_reg, counts, R, lb = CASES[name]
    lbs = LETTERBOXES[:len(counts)] if lb else None
    z, d, p, ref = make_case(seed, C, multi_reg, list(counts), R, lbs)
    return dict(cls=z, box=d, proposals=p, counts=list(counts), R=R, C=C, multi_reg=multi_reg, letterboxes=lbs, ref=ref)
