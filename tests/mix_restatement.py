"""Float64 / numpy restatements of label smoothing, MixUp and CutMix as include/fastvision_amd.h states them: the mix plan (Philox words
from tests/vgg_restatement.py, the uniform, Johnk's method, torchvision's box), the apply pass and the three target forms of the soft
cross-entropy, with the limits the GPU tests hold the kernels to.  Not a test module (pytest does not collect it);
tests/test_mix_restatement_cpu.py pins it without a GPU, tests/test_gpu_mix.py and tests/test_gpu_soft_ce.py compare the device with it.

Limits.  Every limit comes from the formula evaluated in fp32 on the CPU against float64 on the same inputs (e32), times FACTOR = 4
because device libm is not host libm, plus a floor of FACTOR * 2^-24 * magnitude so that an element where the CPU's fp32 happens to be
exact does not make the limit zero (tests/streaming_measure.py).  None is taken from a kernel's output.  The table:

  lam_raw        FACTOR * (|johnk32 - johnk64| + 2^-24 * lam_raw)                                   lam_raw_limit()
  acceptance     a pair whose X + Y lies within FACTOR * (|XpY32 - XpY64| + 2^-24) of 1 is undecidable         plan()
  box            r * W (and r * H) in float64 +- [FACTOR * (|rW32 - rW64| + 2^-24 * rW) + 2^-25 * 0.25 * W / sqrt(1 - lam_raw)]: the second
                 term is what rounding lam_raw to fp32 (half an ulp below 1 = 2^-25) moves r * W by; a draw is undecidable when that
                 interval, cut off at 0 (r >= 0), holds an integer boundary; then either neighbour is accepted             plan()
  CE row value   FACTOR * |row32 - row64| + (C + 6) * 2^-24 * max(|sum q (z - m)|, sum(q) |log den|, 1, eps * max|z|) per row, the rule of
                 tests/test_gpu_losses.py::check_rows for its cross-entropy ((C + 6) * 2^-24: the kernel's softmax denominator is one chain
                 of C fp32 additions); the new last entry covers the smoothing term (eps / C) * (sum z - C m), whose sum of C logits is
                 another such chain: its error is below (C + 6) * 2^-24 * max|z| * eps.                                   soft_ce_limits()
  CE gradient    FACTOR * |g32 - g64| + (C + 6) * 2^-24 * scale * w * max(q, softmax * sum(q))                            soft_ce_limits()
  MixUp          streaming_measure's rule: FACTOR * (e32 + 2^-24 * max(|lam x|, |(1 - lam) x'|)), + half a bf16 ulp for bf16 outputs
"""
import math

import numpy as np
import torch

import streaming_measure as sm
from vgg_restatement import philox4x32_10

F64, F32 = torch.float64, torch.float32
FACTOR = sm.FACTOR
EPS32 = sm.EPS32
PLAN_WORDS = 9
JOHNK_MAX_PAIRS = 512


# ---------------------------------------------------------------------------------------------------------------- the plan
def tick_words(seed, counters, block):
    """Words 4 * block ... 4 * block + 3 of the ticks ``counters`` (uint64 array): philox(counter = (block, 0, call counter lo, hi), key = seed)."""
    counters = np.asarray(counters, dtype=np.uint64)
    blk = np.zeros_like(counters) + np.uint64(block)
    return philox4x32_10(blk, np.zeros_like(counters), counters & np.uint64(0xFFFFFFFF), counters >> np.uint64(32), seed & 0xFFFFFFFF, seed >> 32)


def uniform(word):
    """u = ((word >> 8) + 0.5f) * 2^-24 AS FP32 ARITHMETIC FORMS IT: v = word >> 8 is exact, v + 0.5f is exact below 2^23 and rounded to
    even above (fp32 has no half there: an even v stays, an odd v becomes v + 1), the product with 2^-24 is exact.  So u lies in (0, 1];
    1 is reached by v = 2^24 - 1 alone.  Returned as float64 (every fp32 value is one)."""
    v = (np.asarray(word, dtype=np.uint64) >> np.uint64(8)).astype(np.float32)
    return ((v + np.float32(0.5)) * np.float32(2.0 ** -24)).astype(np.float64)


def johnk_pair(U, V, alpha, dt=np.float64):
    """One pair of Johnk's method in ``dt``: (X + Y, the value returned if the pair is accepted)."""
    U, V, inv = U.astype(dt), V.astype(dt), dt(1.0) / np.asarray(alpha, dtype=dt)
    with np.errstate(under='ignore', divide='ignore', invalid='ignore'):
        X, Y = np.power(U, inv), np.power(V, inv)
        XpY = X + Y
        lx, ly = np.log(U) * inv, np.log(V) * inv
        lm = np.maximum(lx, ly)
        lx, ly = lx - lm, ly - lm
        logform = np.exp(lx - np.log(np.exp(lx) + np.exp(ly)))
        val = np.where(XpY > 0, X / np.where(XpY > 0, XpY, 1), logform)
    return XpY, val


def johnk(seed, counters, alpha):
    """lam_raw ~ Beta(alpha, alpha) for every tick: the first pair (words 4 + 2 i, 5 + 2 i) with X + Y <= 1.  Returns (lam_raw float64, the fp32
    evaluation on the same pair, undecidable: some pair up to the accepted one had X + Y within the fp32 limit of 1)."""
    counters = np.asarray(counters, dtype=np.uint64)
    n = counters.shape[0]
    lam, lam32 = np.full(n, 0.5), np.full(n, 0.5, dtype=np.float32)
    und, open_ = np.zeros(n, dtype=bool), np.ones(n, dtype=bool)
    alpha = np.asarray(alpha, dtype=np.float64) + np.zeros(n)
    for pair in range(JOHNK_MAX_PAIRS):
        if not open_.any():
            break
        if pair % 2 == 0:
            w = tick_words(seed, counters, 1 + pair // 2)
        U, V = uniform(w[2 * (pair % 2)]), uniform(w[2 * (pair % 2) + 1])
        XpY, val = johnk_pair(U, V, alpha)
        XpY32, val32 = johnk_pair(U, V, alpha.astype(np.float32), np.float32)
        close = np.abs(XpY - 1.0) <= FACTOR * (np.abs(XpY32.astype(np.float64) - XpY) + EPS32)
        und |= open_ & close
        take = open_ & (XpY <= 1.0)
        lam[take], lam32[take] = val[take], val32[take]
        open_ &= ~take
    return lam, lam32, und


def lam_raw_limit(lam64, lam32):
    return FACTOR * (np.abs(lam32.astype(np.float64) - lam64) + EPS32 * np.abs(lam64))


def _half_extent(lam64, size):
    """(floor of r * size in float64, undecidable) with r = 0.5 * sqrt(1 - lam_raw)."""
    one = np.maximum(1.0 - lam64, 0.0)
    rs = 0.5 * np.sqrt(one) * size
    lam32 = lam64.astype(np.float32)
    rs32 = (np.float32(0.5) * np.sqrt(np.float32(1.0) - lam32) * np.float32(size)).astype(np.float64)
    delta = FACTOR * (np.abs(rs32 - rs) + EPS32 * rs) + 2.0 ** -25 * 0.25 * size / np.sqrt(np.maximum(one, 2.0 ** -25))
    lo, hi = np.floor(np.maximum(rs - delta, 0.0)), np.floor(rs + delta)
    return np.floor(rs).astype(np.int64), lo != hi


def box_of(rx, ry, hw, hh, H, W):
    x1, x2 = np.maximum(rx - hw, 0), np.minimum(rx + hw, W)
    y1, y2 = np.maximum(ry - hh, 0), np.minimum(ry + hh, H)
    return x1, y1, x2, y2


def lam_of_box(x1, y1, x2, y2, H, W):
    """lam = 1.f - (float)((x2 - x1) * (y2 - y1)) / (float)(W * H), in fp32 as the kernel forms it."""
    area = ((x2 - x1) * (y2 - y1)).astype(np.float32)
    return np.float32(1.0) - area / np.float32(W * H)


def plan(seed, counter0, n, mixup_alpha, cutmix_alpha, prob, switch_prob, H, W):
    """The plans of ticks counter0 ... counter0 + n - 1 as a dict of arrays: mode, lam_raw (float64), lam_raw32 (the fp32 evaluation, for
    the limit), lam (fp32, from the box / = lam_raw for MixUp / 1), rx, ry, hw, hh, x1, y1, x2, y2, und_accept, und_w, und_h."""
    counters = np.arange(counter0, counter0 + n, dtype=np.uint64)
    head = tick_words(seed, counters, 0)
    u0, u1 = uniform(head[0]), uniform(head[1])
    prob, switch_prob = float(np.float32(prob)), float(np.float32(switch_prob))          # the C ABI takes floats
    ma, ca = float(np.float32(mixup_alpha)), float(np.float32(cutmix_alpha))
    cut = (u1 < switch_prob) if (ma > 0 and ca > 0) else np.full(n, ca > 0)
    alpha = np.where(cut, ca, ma)
    applied = (u0 < prob) & (alpha > 0)
    mode = np.where(applied, np.where(cut, 2, 1), 0)
    lam_raw, lam_raw32, und = johnk(seed, counters, np.where(alpha > 0, alpha, 1.0))
    lam_raw = np.where(applied, lam_raw, 1.0)
    lam_raw32 = np.where(applied, lam_raw32, np.float32(1.0)).astype(np.float32)
    is_cut = mode == 2
    rx = np.where(is_cut, (head[2] * np.uint64(W)) >> np.uint64(32), 0).astype(np.int64)
    ry = np.where(is_cut, (head[3] * np.uint64(H)) >> np.uint64(32), 0).astype(np.int64)
    hw, und_w = _half_extent(lam_raw, W)
    hh, und_h = _half_extent(lam_raw, H)
    x1, y1, x2, y2 = box_of(rx, ry, hw, hh, H, W)
    z = np.zeros(n, dtype=np.int64)
    x1, y1, x2, y2, hw, hh = (np.where(is_cut, v, z) for v in (x1, y1, x2, y2, hw, hh))
    lam = np.where(is_cut, lam_of_box(x1, y1, x2, y2, H, W), lam_raw.astype(np.float32)).astype(np.float32)
    return dict(mode=mode, lam_raw=lam_raw, lam_raw32=lam_raw32, lam=lam, rx=rx, ry=ry, hw=hw, hh=hh, x1=x1, y1=y1, x2=x2, y2=y2,
                und_accept=und & applied, und_w=und_w & is_cut, und_h=und_h & is_cut)


def beta_moments(alpha):
    """Mean, variance and fourth central moment of Beta(alpha, alpha): 1/2, 1 / (4 (2 alpha + 1)), var^2 * (3 - 6 / (2 alpha + 3))."""
    var = 1.0 / (4.0 * (2.0 * alpha + 1.0))
    return 0.5, var, var * var * (3.0 - 6.0 / (2.0 * alpha + 3.0))


# (seed, (mixup_alpha, cutmix_alpha, prob, switch_prob, H, W)) of the 4096-tick plan tests.  The seeds are chosen so that the float64
# restatement has no undecidable draw (tests/test_mix_restatement_cpu.py checks that).  alpha = 0.2 runs at ODD sizes: Beta(0.2, 0.2) piles
# up at lam_raw -> 0, where r * W -> W / 2, and at an even W that is an integer boundary which fp32 (1.f - lam_raw == 1 below 2^-25) and
# float64 put on different sides -- about 3 % of such draws are genuinely undecidable there, whatever the seed.
PLAN_SETTINGS = [(3, (0.2, 0.2, 0.7, 0.5, 37, 53)), (5, (1.0, 1.0, 1.0, 0.3, 32, 48)), (7, (0.2, 1.0, 1.0, 0.5, 224, 224))]
PLAN_TICKS = 4096


def plan_words(mode, lam_raw, lam, rx=0, ry=0, x1=0, y1=0, x2=0, y2=0):
    """A plan as the int32[9] tensor the kernels read (the tests write their own plans with this)."""
    t = torch.zeros(PLAN_WORDS, dtype=torch.int32)
    t[0] = mode
    t[1:3] = torch.tensor([lam_raw, lam], dtype=torch.float32).view(torch.int32)
    t[3:] = torch.tensor([rx, ry, x1, y1, x2, y2], dtype=torch.int32)
    return t


# ---------------------------------------------------------------------------------------------------------------- the apply pass
def apply(x, mode, lam, box, dt):
    """out [B, C, H, W] in ``dt`` from x (values the storage dtype holds): partner = x.roll(1, 0).  Returns (out, mag, inside) with mag = the
    larger of the two MixUp terms and inside = the CutMix box as a [H, W] mask (None for the other modes).  B == 1 is the identity."""
    xx = x.to(dt)
    if mode == 0 or x.shape[0] == 1:
        return xx, xx.abs(), None
    partner = xx.roll(1, 0)
    if mode == 1:
        lam_t = torch.tensor(lam, dtype=F32).to(dt)                     # lam and 1.f - lam as the kernel holds them: fp32 values
        oml = (torch.tensor(1.0, dtype=F32) - torch.tensor(lam, dtype=F32)).to(dt)
        a, b = lam_t * xx, oml * partner
        return a + b, torch.maximum(a.abs(), b.abs()), None
    x1, y1, x2, y2 = box
    inside = torch.zeros(x.shape[2], x.shape[3], dtype=torch.bool)
    inside[max(y1, 0):max(y2, 0), max(x1, 0):max(x2, 0)] = True
    return torch.where(inside, partner, xx), xx.abs(), inside


# ---------------------------------------------------------------------------------------------------------------- soft cross-entropy
def soft_targets(R, C, dt, labels=None, lam=None, dense=None, eps=0.0):
    """q = (1 - eps) t + eps / C with t = onehot(y) | lam onehot(y_r) + (1 - lam) onehot(y_(r-1)) | dense."""
    if dense is not None:
        t = dense.to(dt)
    else:
        t = torch.zeros(R, C, dtype=dt).scatter_(1, labels.reshape(-1, 1).long(), 1.0)
        if lam is not None:
            lam_t = torch.tensor(lam, dtype=F32).to(dt)
            oml = (torch.tensor(1.0, dtype=F32) - torch.tensor(lam, dtype=F32)).to(dt)
            t = lam_t * t + oml * t.roll(1, 0)
    e = torch.tensor(eps, dtype=F32).to(dt)
    return (1 - e) * t + e / C


def soft_ce(z, dt, labels=None, lam=None, dense=None, eps=0.0, weights=None, mean=True):
    """Rows, value and gradient in ``dt``: rows = -w sum_k q_k log_softmax(z)_k, grad = scale w (softmax sum(q) - q).  Returns a dict."""
    z = z.to(dt)
    R, C = z.shape
    q = soft_targets(R, C, dt, labels, lam, dense, eps)
    w = torch.ones(R, dtype=dt) if weights is None else weights.to(dt)
    m = z.max(1, keepdim=True)[0]
    den = torch.exp(z - m).sum(1, keepdim=True)
    lsm = (z - m) - torch.log(den)
    soft = torch.exp(lsm)
    sq = q.sum(1, keepdim=True)
    rows = -(q * lsm).sum(1) * w
    scale = 1.0 / R if mean else 1.0
    grad = scale * w[:, None] * (soft * sq - q)
    return dict(rows=rows, value=rows.sum() * scale, grad=grad, q=q, sq=sq, soft=soft, logden=torch.log(den), qzm=(q * (z - m)).sum(1), w=w, scale=scale)


def soft_ce_limits(z, **kw):
    """(float64 result dict, value limit, gradient limit [R, C]) by the table in the module docstring."""
    r64, r32 = soft_ce(z, F64, **kw), soft_ce(z, F32, **kw)
    R, C = z.shape
    eps = kw.get('eps', 0.0)
    unit = (C + 6) * EPS32
    rmag = torch.stack([r64['qzm'].abs(), (r64['sq'] * r64['logden']).abs().squeeze(1), torch.ones(R, dtype=F64),
                        eps * z.double().abs().amax(1)]).amax(0)
    w = r64['w'].abs()
    vlim = (FACTOR * (r32['rows'].double() - r64['rows']).abs() + unit * rmag * w).sum() * r64['scale'] + EPS32 * r64['value'].abs()
    glim = FACTOR * (r32['grad'].double() - r64['grad']).abs() + unit * r64['scale'] * w[:, None] * torch.maximum(r64['q'], r64['soft'] * r64['sq'])
    return r64, vlim, glim


# ---------------------------------------------------------------------------------------------------------------- top-k
def topk_hits(z, y, k):
    """hit[r] = #{j : z_j beats z_y} < k, with the argmax order: a NaN is largest, among equals the smaller index wins.  Plain loops."""
    z = z.float()
    R, C = z.shape
    hits = []
    for r in range(R):
        yy = float(y[r])
        if not (0 <= yy < C and yy == math.floor(yy)):
            hits.append(False)
            continue
        yi, zy = int(yy), z[r, int(yy)].item()
        cnt = 0
        for j in range(C):
            if j == yi:
                continue
            v = z[r, j].item()
            vn, bn = math.isnan(v), math.isnan(zy)
            if vn != bn:
                better = vn
            elif vn or v == zy:
                better = j < yi
            else:
                better = v > zy
            cnt += better
        hits.append(cnt < k)
    return torch.tensor(hits)
