"""The reference formulas and limits of tests/test_gpu_stem.py: conv0 (3x3, stride 1, pad 1, Cin <= 3, Cout = 32) alone and recomputed inside
its BatchNorm / SiLU passes (csrc/stem.hip), and its two weight gradients, element by element against float64 on the operands the kernel
reads.  Not a test module (pytest does not collect it); tests/test_stem_restatement_cpu.py pins it without a GPU.  The element measure, the
sum rule and the constants (FACTOR_SIGMOID, BIAS_MAX, BIAS_MIN_N) are those of tests/streaming_measure.py; what is added here is derived, and
nothing is taken from a device result.

  * y64 = the float64 convolution of the operands as the kernel reads them (the MFMA paths read bf16(image) and bf16(weights); the host
    rounds them once and feeds the rounded tensors to both sides).  The kernel's y is one chain of n fp32 fmas (VALU), or two MFMAs, which
    are k-ordered fp32 fma chains without wider accumulation: any order of n fp32 additions of rounded products stays inside
    ylim = sum_limit(n, sum|term|) = (n + 2) * 2^-24 * conv(|x|, |w|), per element.  n = the k slots that can hold a non-zero product:
    9 * Cin in the direct kernel, 36 (3 x 3 taps x 4 packed channels) in the MFMA kernels; the slots 36..63 multiply zeros exactly.
  * y stored (forward kernels): |got - y64| <= ylim (+ half a bf16 ulp of y64 for a bf16 store).
  * The fused passes never store y.  Their outputs get the streaming element measure evaluated AT y64 (e32 = plain fp32 torch ops on
    fp32(y64)) plus what an error of ylim in y does to the output, first order with the derivative bounded on the whole axis:
        APPLY   z = SiLU(u), u = y * scale + shift:          |SiLU'| <= 1.1            ->  + 1.1 * |scale| * ylim
        DGRAD   dY = a * dz * SiLU'(u) + k1 * y + k2:        |SiLU''| <= 0.5           ->  + |a| * |dz| * 0.5 * |scale| * ylim + |k1| * ylim
        REDUCE  sum dU, dU = dz * SiLU'(u):                                            ->  + sum |dz| * 0.5 * |scale| * ylim
                sum dU * xhat, xhat = (y - mean) * rstd:     product rule              ->  + sum (|dz| * 0.5 * |scale| * ylim * |xhat| + |dU| * rstd * ylim)
        STATS   sum y, sum y^2 (also the MFMA forward's):                              ->  + sum ylim,  + sum (2 |y64| ylim + ylim^2)
    (the second-order remainders are 2^-24 of these and sit inside the slack between the (n - 1) of the any-order bound and the (n + 2) of
    the rule).  Sums follow sum_limit(n, sum|term|, sum e32) with n = the longest chain of fp32 additions behind one entry, read off the
    launch geometry by the functions below, and are compared PER BLOCK ROW: the pixels a block owns are known.
  * The direct forward kernel's statistics are sums of the STORED values: against float64 sums of the downloaded y, by the sum rule alone.
  * Weight gradients: per element of dW, sum_limit(n, sum|dy * x|); accumulate = 1 adds one more rounding of the result.
"""
import torch
import torch.nn.functional as F

import streaming_measure as sm

CO = 32
N_MFMA = 36                 # 3 x 3 taps x 4 packed channels: the k slots of the two MFMAs that are not zero by construction
F64, F32, BF = torch.float64, torch.float32, torch.bfloat16


def cdiv(a, b):
    return -(-a // b)


def n_direct(Cin):
    """stem_fwd_kernel: acc[c] += v * w over ci, kh, kw -- one chain of 9 * Cin fmas"""
    return 9 * Cin


# ---- launch geometry: who owns a pixel, and the longest chain of fp32 additions behind one table entry --------------------------------------
def direct_stats_geometry(M):
    """stem_fwd_kernel: block = 256 consecutive pixels; a thread adds 32 of them (p = grp, grp + 8, ...), then one thread adds the 8 groups."""
    return torch.arange(M) // 256, cdiv(M, 256), 32 + 8


def mfma_stats_geometry(M):
    """stem_fwd_mfma_kernel: block = 1024 consecutive pixels = 4 waves x 16 tiles; a lane adds one value per tile (16), four xor-shuffles
    fold the 16 pixels of a tile, (w0 + w1) + (w2 + w3) folds the waves (2)."""
    return torch.arange(M) // 1024, cdiv(M, 1024), 16 + 4 + 2


def fused_geometry(M, blocks):
    """stem_fused_kernel: chunk = 256 consecutive pixels (16 tiles); chunk c belongs to wave slot c mod (4 * blocks), block = slot // 4.
    A lane adds 16 values per chunk it visits, rounds = ceil(chunks / (4 * blocks)) chunks at most, then 4 shuffles and 2 for the waves."""
    nchunks = cdiv(M // 16, 16)
    rounds = cdiv(nchunks, 4 * blocks)
    owner = ((torch.arange(M) // 256) % (4 * blocks)) // 4
    return owner, rounds, 16 * rounds + 4 + 2


def wgrad_chain(M):
    """stem_wgrad_kernel + stem_wgrad_reduce_kernel: tiles of 128 pixels strided over min(tiles, 1024) blocks; a worker lane adds 32 products
    per tile, the 4 pixel groups fold in 2; the reduce adds ceil(blocks / 256) partials per lane and folds 256 lanes in 8."""
    ntiles = cdiv(M, 128)
    grid = min(ntiles, 1024)
    tiles_per_block = cdiv(ntiles, grid)
    return 32 * tiles_per_block + 2 + cdiv(grid, 256) + 8, ntiles, grid


def wgrad_mfma_chain(M):
    """fva_stem_wgrad_mfma: split-K blocks of mchunk pixels (one MFMA chain over them: mchunk additions), then wgrad_reduce_kernel adds at
    most ceil(ksplit / 4) slabs per group and folds the 4 groups in 2."""
    mchunk = cdiv(cdiv(M, 512), 64) * 64
    ksplit = cdiv(M, mchunk)
    return mchunk + cdiv(ksplit, 4) + 2, mchunk, ksplit


# ---- the convolution in float64, whole or band by band ---------------------------------------------------------------------------------------
def conv_rows(x, w, b, r0, r1):
    """rows r0 .. r1-1 of image b: (y64, sum|term|) as [(r1 - r0) * W, 32] float64 (NHWC order: the kernels' pixel index m)"""
    H = x.shape[2]
    lo, hi = max(r0 - 1, 0), min(r1 + 1, H)
    xs = x[b:b + 1, :, lo:hi].double()
    xs = F.pad(xs, (0, 0, 1 if r0 == 0 else 0, 1 if r1 == H else 0))
    w64 = w.double()
    y = F.conv2d(xs, w64, padding=(0, 1))
    a = F.conv2d(xs.abs(), w64.abs(), padding=(0, 1))
    return y[0].permute(1, 2, 0).reshape(-1, CO), a[0].permute(1, 2, 0).reshape(-1, CO)


def bands(B, H, W, max_pixels=1 << 17):
    """(b, r0, r1, m0, m1): bands of whole image rows that cover the batch in pixel order, at most max_pixels each (one row at least)"""
    R = max(1, max_pixels // W)
    for b in range(B):
        for r0 in range(0, H, R):
            r1 = min(r0 + R, H)
            yield b, r0, r1, (b * H + r0) * W, (b * H + r1) * W


def conv64(x, w):
    """the whole batch at once: (y64, sum|term|) as [B * H * W, 32]"""
    B, _, H, W = x.shape
    parts = [conv_rows(x, w, b, r0, r1) for b, r0, r1, _, _ in bands(B, H, W)]
    return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])


def conv_fma32(x, w):
    """An honest device evaluation on the CPU: one chain of fp32 fmas in the MFMA's k order (kh, kw, ci), [B * H * W, 32] fp32.  The product
    of two fp32 numbers is exact in float64, so rounding acc + a * b from float64 to fp32 is the fma up to a double rounding."""
    B, Cin, H, W = x.shape
    xp = F.pad(x.float(), (1, 1, 1, 1)).double()
    acc = torch.zeros(B, H, W, CO, dtype=F32)
    for kh in range(3):
        for kw in range(3):
            for ci in range(Cin):
                acc = (acc.double() + xp[:, ci, kh:kh + H, kw:kw + W, None] * w[:, ci, kh, kw].double()).float()
    return acc.reshape(-1, CO)


def y_limit(n, sabs):
    return sm.sum_limit(n, sabs)


def out_limit(ref64, limit, bf16):
    """what a stored element may be off by: the limit, plus half a bf16 ulp of the reference where the store rounds to bf16"""
    return 0.5 * sm.bf16_ulp(ref64) + limit if bf16 else limit


def worst(got, ref64, limit, bf16):
    return sm.worst_f32(got, ref64, out_limit(ref64, limit, bf16))


# ---- the packed image: zero-bordered NHWC4 bf16, 8 bytes per pixel, 64 bytes of slack -----------------------------------------------------
def pack_host(img_bf16, slack=0):
    """[B * (H + 2) * (W + 2) * 4 + 32] bf16: the buffer fva_stem_pack writes, made with torch's own cast; the 32 slack elements get the
    16-bit pattern `slack`"""
    B, Cin, H, W = img_bf16.shape
    buf = torch.zeros(B, H + 2, W + 2, 4, dtype=BF)
    buf[:, 1:-1, 1:-1, :Cin] = img_bf16.permute(0, 2, 3, 1)
    tail = torch.full((32,), slack, dtype=torch.int16).view(BF)
    return torch.cat([buf.reshape(-1), tail])


# ---- BatchNorm tables, made on the host from float64 statistics and rounded to fp32 once -------------------------------------------------
class Tables:
    """scale, shift, mean, rstd and the backward coefficients a, cb, cc ([32] fp32 each) as the fused passes read them"""

    def __init__(self, s1, s2, M, gamma, beta, dbeta_mean, dgamma_mean, eps=1e-5):
        mean = s1 / M
        var = (s2 / M - mean * mean).clamp_min(0)
        rstd = 1 / torch.sqrt(var + eps)
        g64, b64 = gamma.double(), beta.double()
        self.mean, self.rstd = mean.float(), rstd.float()
        self.scale, self.shift = (g64 * rstd).float(), (b64 - mean * g64 * rstd).float()
        a = g64 * rstd
        self.a, self.cb, self.cc = a.float(), (-a * dgamma_mean).float(), (-a * dbeta_mean).float()

    def coef(self):
        return torch.stack([self.a, self.cb, self.cc]).contiguous()


def draw_gamma_beta(g):
    """realistic BatchNorm weights of both signs; two channels at +-3 so that u = gamma * xhat + beta reaches both sigmoid tails"""
    gamma = (torch.rand(CO, generator=g) * 2.5 + 0.5) * torch.where(torch.rand(CO, generator=g) < 0.5, -1.0, 1.0)
    gamma[3], gamma[20] = 3.0, -3.0
    return gamma, torch.rand(CO, generator=g) * 2 - 1


# ---- the fused passes at y64, with the share of ylim ------------------------------------------------------------------------------------------
def apply_ref(y64, yl, t):
    z64, s64 = sm.silu_apply(y64, t.scale, t.shift, None, F64)
    z32, _ = sm.silu_apply(y64.float(), t.scale, t.shift, None, F32)
    lim = sm.limit_of(z64, z32, s64.abs(), sm.FACTOR_SIGMOID) + 1.1 * t.scale.double().abs() * yl
    return z64, lim


def dgrad_ref(dz, y64, yl, t):
    r64, mag = sm.bwd_apply(dz, y64, t.scale, t.shift, t.mean, t.rstd, t.a, t.cb, t.cc, F64)
    r32, _ = sm.bwd_apply(dz, y64.float(), t.scale, t.shift, t.mean, t.rstd, t.a, t.cb, t.cc, F32)
    k1 = t.cb.double() * t.rstd.double()
    extra = t.a.double().abs() * dz.double().abs() * 0.5 * t.scale.double().abs() * yl + k1.abs() * yl
    return r64, sm.limit_of(r64, r32, mag, sm.FACTOR_SIGMOID) + extra


def reduce_terms(dz, y64, yl, t):
    """per element: the two float64 terms, their e32, and what ylim may move them by"""
    t64 = sm.bwd_terms(dz, y64, t.scale, t.shift, t.mean, t.rstd, F64)
    t32 = sm.bwd_terms(dz, y64.float(), t.scale, t.shift, t.mean, t.rstd, F32)
    ddu = dz.double().abs() * 0.5 * t.scale.double().abs() * yl
    xhat = (y64 - t.mean.double()) * t.rstd.double()
    extra = (ddu, ddu * xhat.abs() + t64[0].abs() * t.rstd.double() * yl)
    return t64, tuple((b.double() - a).abs() for a, b in zip(t64, t32)), extra


def stats_terms(y64, yl):
    return (y64, y64 * y64), (yl, 2 * y64.abs() * yl + yl * yl)


class RowSums:
    """float64 sums per (block row, table, channel) of terms, |terms|, e32 and extras, added up band by band"""

    def __init__(self, rows, owner):
        self.owner = owner
        self.ref, self.abs, self.e32, self.extra = (torch.zeros(rows, 2, CO, dtype=F64) for _ in range(4))

    def add(self, m0, m1, terms, e32=None, extra=None):
        idx = self.owner[m0:m1]
        for k in range(2):
            self.ref[:, k].index_add_(0, idx, terms[k])
            self.abs[:, k].index_add_(0, idx, terms[k].abs())
            if e32 is not None:
                self.e32[:, k].index_add_(0, idx, e32[k])
            if extra is not None:
                self.extra[:, k].index_add_(0, idx, extra[k])

    def worst(self, got, n):
        """largest err / limit over the rows of a downloaded [rows][2][32] table; inf where an entry is not finite"""
        lim = sm.sum_limit(n, self.abs, self.e32) + self.extra
        return sm.worst_f32(got, self.ref, lim)


# ---- weight gradient -------------------------------------------------------------------------------------------------------------------------
def wgrad64(x, dy):
    """dW[co][ci][kh][kw] = sum_m dy[m][co] * x[b][ci][y + kh - 1][x + kw - 1] in float64, and the sum of the |products|; dy is [B, H, W, 32]"""
    B, Cin, H, W = x.shape
    cols = F.unfold(x.double(), 3, padding=1)                       # [B, Cin * 9, H * W], j = ci * 9 + kh * 3 + kw
    d = dy.double().reshape(B, H * W, CO)
    ref = torch.einsum('bjm,bmc->cj', cols, d).reshape(CO, Cin, 3, 3)
    sabs = torch.einsum('bjm,bmc->cj', cols.abs(), d.abs()).reshape(CO, Cin, 3, 3)
    return ref, sabs


def wgrad_worst(got, ref, sabs, n, pre=None):
    lim = sm.sum_limit(n, sabs)
    if pre is not None:                                             # dw = dw + sum: one more rounding, of the result
        ref = ref + pre.double()
        lim = lim + sm.EPS32 * (ref.abs() + lim)
    return sm.worst_f32(got, ref, lim)
