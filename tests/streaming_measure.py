"""The measure of tests/test_gpu_streaming.py: every element of a streaming kernel's output against the float64 result of the same formula
on the same operands.  Not a test module (pytest does not collect it); tests/test_streaming_measure_cpu.py pins it without a GPU.

  * e32: the formula evaluated with plain torch ops in fp32 on the CPU, and its element-wise distance from the float64 result -- what an
    honest fp32 implementation costs, taken from the reference and never from the kernel.  The kernels use __expf and the hardware
    reciprocal where torch uses accurately rounded routines, so they get FACTOR x that, plus FACTOR * 2^-24 * mag (mag = the largest
    magnitude among the terms of the element's last addition) so that an element where torch's fp32 happens to be exact does not make the
    limit zero.  FACTOR = 4; the kernels with a sigmoid get FACTOR_SIGMOID, derived below.
  * fp32 outputs:  |got - ref64| <= limit, every element.
  * bf16 outputs:  |got - ref64| <= 0.5 * bf16_ulp(ref64) + limit, every element (ONE rounding to nearest, where the kernel stores), and
    the mean of sign(ref64) * (got - ref64) / bf16_ulp(ref64) within +-0.02: rounding to nearest gives 0 +- 0.29 / sqrt(n), a truncating
    store gives -0.5.  The bias is only meaningful from 1e5 smooth random elements on.
  * sums: added up on the host in float64 against the float64 sum of the float64 terms, per channel:
    |err| <= (n + 2) * 2^-24 * sum|term| + 4 * sum(e32 of the terms), n = the longest chain of fp32 additions behind one entry (any order
    of n fp32 additions stays inside (n - 1) * 2^-24 * sum|x|).
"""
import torch

EPS32 = 2.0 ** -24          # half an ulp of fp32 relative to the value: one rounding to nearest
FACTOR = 4.0
# The kernels that evaluate a sigmoid (forward and backward apply) need more than 4 x, explained, not measured: __expf(-u) is
# v_exp_f32(-u * log2(e)), and the product -u * log2(e) is ROUNDED TO FP32 before the exponential.  Half an ulp of an argument in [16, 32)
# (11.1 <= |u| < 22.2, the tails these tests reach) is 2^-20, i.e. a relative error of ln(2) * 2^-20 = 11.1 * 2^-24 in e^-u and, at the
# negative tail where SiLU(u) ~ u e^u and SiLU'(u) ~ (1 + u) e^u, in the result; v_exp_f32 (1 ulp = 2 * 2^-24), v_rcp_f32 (1 ulp = 2 * 2^-24)
# and the final multiply (2^-24) come on top: 16 * 2^-24 of the result where torch's accurately rounded exp leaves an e32 that can be
# next to nothing on the same element.  That is four times the 4 * 2^-24 * mag floor: a need of 16, so the factor is 32.  (At |u| = 6.57
# the argument 9.48 lies in [8, 16): ln(2) * 2^-21 = 5.5 * 2^-24; modelling ONLY that rounding on the CPU reproduces the first GPU run's
# worst forward element, err / limit 1.2215 at factor 4, to four digits.)  bf16 outputs hardly notice: half a bf16 ulp is 2^-9.
FACTOR_SIGMOID = 32.0
BIAS_MAX = 0.02
BIAS_MIN_N = 100000


def bf16_ulp(ref):
    """Spacing of bf16 (8 significant bits) around |ref|: |ref| = m * 2^e with m in [0.5, 1) -> 2^(e - 8); floored at the spacing of the
    smallest normal number (2^-126 = 0.5 * 2^-125 -> 2^-133)."""
    a = ref.detach().double().abs()
    _, e = torch.frexp(a)
    e = torch.where(a < 2.0 ** -126, torch.full_like(e, -125), e)
    return torch.ldexp(torch.ones_like(a), e - 8)


def limit_of(ref64, ref32, mag, factor=FACTOR):
    """limit = factor * (e32 + 2^-24 * mag), element-wise (float64)."""
    e32 = (ref32.double() - ref64).abs()
    return factor * (e32 + EPS32 * mag.double().abs())


def worst_f32(got, ref64, limit):
    """Largest err / limit over all elements of an fp32 output (<= 1 passes); inf if anything is not finite where the reference is."""
    err = (got.double() - ref64).abs()
    ratio = err / limit.clamp_min(1e-300)
    ratio = torch.where(err == 0, torch.zeros_like(ratio), ratio)
    ratio = torch.where(torch.isfinite(err), ratio, torch.full_like(ratio, float('inf')))
    return ratio.max().item() if ratio.numel() else 0.0


def worst_bf16(got, ref64, limit):
    """Largest err / (0.5 * bf16_ulp(ref64) + limit) over all elements of a bf16 output."""
    return worst_f32(got, ref64, 0.5 * bf16_ulp(ref64) + limit)


def rounding_bias(got, ref64):
    """Mean over ALL elements of sign(ref64) * (got - ref64) / bf16_ulp(ref64): 0 for rounding to nearest, -0.5 for truncation."""
    return (torch.sign(ref64) * (got.double() - ref64) / bf16_ulp(ref64)).mean().item()


def check(got, ref64, ref32, mag, bf16, bias=False, factor=FACTOR, what=''):
    """Assert the element-wise measure (and the bias when asked for); returns the worst err / limit for the test to print."""
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    lim = limit_of(ref64, ref32, mag, factor)
    w = worst_bf16(got, ref64, lim) if bf16 else worst_f32(got, ref64, lim)
    assert w <= 1.0, f'{what}: worst err / limit = {w:.3f}'
    if bias:
        assert bf16 and got.numel() >= BIAS_MIN_N, (what, got.numel())
        b = rounding_bias(got, ref64)
        assert abs(b) <= BIAS_MAX, f'{what}: rounding bias {b:+.4f} ulp'
    return w


def sum_limit(n, abs_terms_sum, e32_terms_sum=None):
    """Per-channel limit of a sum whose longest chain of fp32 additions is n."""
    lim = (n + 2) * EPS32 * abs_terms_sum.double()
    if e32_terms_sum is not None:
        lim = lim + 4.0 * e32_terms_sum.double()
    return lim


# ---- the formulas, written once for float64 (the reference) and fp32 (e32): dt = torch.float64 / torch.float32 -------------------------------
def silu_apply(y, scale, shift, res, dt):
    """z = SiLU(y * scale + shift) (+ res) over channels-last tensors; returns (z, silu)."""
    u = y.to(dt) * scale.to(dt) + shift.to(dt)
    s = u * torch.sigmoid(u)
    return (s + res.to(dt) if res is not None else s), s


def silu_grad(u):
    s = torch.sigmoid(u)
    return s * (1 + u * (1 - s))


def bwd_terms(dz, y, scale, shift, mean, rstd, dt):
    """dU = dz * SiLU'(y * scale + shift) and dU * xhat, xhat = (y - mean) * rstd."""
    yy = y.to(dt)
    du = dz.to(dt) * silu_grad(yy * scale.to(dt) + shift.to(dt))
    return du, du * (yy - mean.to(dt)) * rstd.to(dt)


def bwd_apply(dz, y, scale, shift, mean, rstd, a, cb, cc, dt):
    """dY = a * dU + k1 * y + k2,  k1 = cb * rstd,  k2 = cc - k1 * mean  (a, cb, cc: the [3][C] table of the backward finalize:
    a = gamma * rstd, cb = -a * dgamma / n, cc = -a * dbeta / n, i.e. dY = gamma * rstd * (dU - dbeta / n - xhat * dgamma / n)).
    Returns (dY, mag) with mag = max(|a dU|, |k1 y|, |k2|)."""
    yy = y.to(dt)
    du = dz.to(dt) * silu_grad(yy * scale.to(dt) + shift.to(dt))
    k1 = cb.to(dt) * rstd.to(dt)
    k2 = cc.to(dt) - k1 * mean.to(dt)
    t1, t2 = a.to(dt) * du, k1 * yy
    mag = torch.maximum(torch.maximum(t1.abs(), t2.abs()), k2.abs().expand_as(t1))
    return t1 + t2 + k2, mag
