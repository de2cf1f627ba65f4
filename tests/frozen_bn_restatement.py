"""BatchNorm backward with FROZEN statistics (the module in eval mode, convolution and affine parameters training), restated with plain
torch ops -- the reference of tests/test_gpu_frozen_bn.py.  Not a test module (pytest does not collect it);
tests/test_frozen_bn_restatement_cpu.py pins it against float64 torch autograd without a GPU.

With fixed statistics
    u  = (y + b - rm) * r * gamma + beta = y * scale + shift,   r = 1 / sqrt(rv + eps), scale = gamma * r, shift = beta + (b - rm) * scale
    z  = act(u),  dU = dz * act'(u)
    dY = scale * dU                                   no batch sum: ONE pass over dz and y
    dbeta = sum dU,  dgamma = sum dU * (y - m) * r,  m = rm - b,   dbias = scale * sum dU
(b: a convolution bias in front of the BatchNorm, the VGG block; 0 elsewhere.)  ``dt`` = torch.float64 gives the reference, torch.float32
the plain fp32 evaluation whose distance from it (e32) scales the limits of tests/streaming_measure.py.
"""
import torch

import streaming_measure as sm

KINK = 2.0 ** -22           # ReLU: |u64| <= KINK * (|y scale| + |shift|) cannot be decided by an fp32 evaluation of u (two roundings of 2^-24 each, doubled)
KINK_SHARE_MAX = 1e-3       # the project's cap on decisions left out of an element-wise check


def act_grad(u, act):
    """act'(u) for 'silu' and 'relu' (the kink itself has gradient 0, as torch.relu)."""
    return sm.silu_grad(u) if act == 'silu' else (u > 0).to(u.dtype)


def terms(dz, y, scale, shift, m, r, act, dt):
    """(u, dU, dU * (y - m) * r, dY) over channels-last tensors, every operand taken to ``dt`` first."""
    yy, sc = y.to(dt), scale.to(dt)
    u = yy * sc + shift.to(dt)
    du = dz.to(dt) * act_grad(u, act)
    return u, du, du * (yy - m.to(dt)) * r.to(dt), sc * du


def param_grads(du, t2, scale):
    """(dgamma, dbeta, dbias) from the two term tensors [..., C] (summed in their own dtype)."""
    flat1, flat2 = du.reshape(-1, du.shape[-1]), t2.reshape(-1, t2.shape[-1])
    s1 = flat1.sum(0)
    return flat2.sum(0), s1, scale.to(du.dtype) * s1


def kink_mask(y, scale, shift):
    """ReLU elements whose float64 pre-activation is closer to zero than fp32 can resolve: left out of the element-wise check."""
    t = y.double() * scale.double()
    return (t + shift.double()).abs() <= KINK * (t.abs() + shift.double().abs())


def eval_coeffs(gamma, beta, rm, rv, eps, bias=None):
    """(scale, shift, m, r) of a BatchNorm in eval mode, in the dtype of gamma."""
    r = 1.0 / torch.sqrt(rv + eps)
    scale = gamma * r
    m = rm if bias is None else rm - bias
    return scale, beta - m * scale, m, r


def make_inputs(B, H, W, Cc, dt, seed):
    """The operands of one kernel launch, on the CPU: y ~ 1.5 N(0, 1) and dz ~ N(0, 1) in ``dt`` (rounded ONCE here: the same tensors are
    uploaded and fed to the reference), scale in +-[0.5, 1.5] with about 20 % negative channels and one channel exactly zero, shift ~ 0.5 N,
    m ~ 0.3 N, r in [0.7, 1.4]."""
    g = torch.Generator().manual_seed(seed)
    y = (torch.randn(B, H, W, Cc, generator=g) * 1.5).to(dt)
    dz = torch.randn(B, H, W, Cc, generator=g).to(dt)
    scale = (torch.rand(Cc, generator=g) + 0.5) * torch.where(torch.rand(Cc, generator=g) < 0.2, -1.0, 1.0)
    scale[Cc // 2] = 0.0
    shift = 0.5 * torch.randn(Cc, generator=g)
    m = 0.3 * torch.randn(Cc, generator=g)
    r = 0.7 + 0.7 * torch.rand(Cc, generator=g)
    return y, dz, scale, shift, m, r


def chain_length(nblocks, B, H, W, Cc, pad, epc):
    """The longest chain of fp32 additions behind one entry of the partial table of a launch of ``nblocks`` blocks (the kernel's own
    query): a block walks ceil(rows / nblocks) padded rows, a lane meets ceil(row_chunks / 256) chunks of its channel chunk per row, and
    the 256 / cpp lanes that share a channel chunk are folded through LDS."""
    cpp = Cc // epc
    rows, row_chunks = B * (H + 2 * pad), (W + 2 * pad) * cpp
    return -(-rows // nblocks) * -(-row_chunks // 256) + 256 // cpp


def finalize_chain(nblocks):
    """fp32 additions of the table fold on top (two interleaved accumulators per thread over every 64th row; doubles from there on)."""
    return -(-nblocks // 128) + 1
