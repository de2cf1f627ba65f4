"""The measure of tests/test_gpu_streaming.py (tests/streaming_measure.py), pinned without a GPU on the forward apply formula
z = SiLU(y * scale + shift) + residual: the honest implementation -- plain fp32 torch ops, rounded to bf16 ONCE -- must be accepted, and
four wrong ones must be rejected: a store that truncates, a SiLU rounded to bf16 before the residual is added, a residual read one pixel
off (wrong pad) and the second chunk of every step dropped (chunks 256..511 of every row zero)."""
import pytest
import torch

import streaming_measure as sm

B, H, W, C = 8, 112, 112, 64          # 6.4M elements; a row is 112 * 8 = 896 sixteen-byte chunks


@pytest.fixture(scope='module')
def data():
    g = torch.Generator().manual_seed(20240607)
    y = (torch.randn(B, H, W, C, generator=g) * 1.5 + 0.3).to(torch.bfloat16)
    res = torch.randn(B, H, W, C, generator=g).to(torch.bfloat16)
    scale = (torch.rand(C, generator=g) * 1.7 + 0.3) * torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    scale[5] = 0.0
    shift = torch.rand(C, generator=g) * 2 - 1
    z64, s64 = sm.silu_apply(y, scale, shift, res, torch.float64)
    z32, s32 = sm.silu_apply(y, scale, shift, res, torch.float32)
    mag = torch.maximum(s64.abs(), res.double().abs())
    return dict(y=y, res=res, scale=scale, shift=shift, z64=z64, z32=z32, s32=s32, lim=sm.limit_of(z64, z32, mag))


def truncate_to_bf16(x32):
    return (x32.contiguous().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)


def test_inputs_reach_both_tails_of_the_sigmoid(data):
    u = data['y'].double() * data['scale'].double() + data['shift'].double()
    assert u.min() < -12 and u.max() > 12
    assert data['z64'].numel() >= 6_000_000


def test_bf16_ulp():
    x = torch.tensor([1.0, 1.5, 1.9999, 2.0, -3.0, 0.75, 0.0, 1e-45, 2.0 ** -126, 300.0], dtype=torch.float64)
    want = torch.tensor([2.0 ** -7, 2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -6, 2.0 ** -8, 2.0 ** -133, 2.0 ** -133, 2.0 ** -133, 2.0], dtype=torch.float64)
    assert torch.equal(sm.bf16_ulp(x), want)
    # the spacing is what torch's own bf16 has: the next bf16 number above a bf16 value is one ulp away
    v = torch.tensor([1.0, 2.5, 100.0, 0.013], dtype=torch.float32).to(torch.bfloat16)
    nxt = (v.view(torch.int16) + 1).view(torch.bfloat16)
    assert torch.equal((nxt.double() - v.double()), sm.bf16_ulp(v.double()))


def test_honest_fp32_evaluation_rounded_once_is_accepted(data):
    got = data['z32'].to(torch.bfloat16)
    w = sm.worst_bf16(got, data['z64'], data['lim'])
    b = sm.rounding_bias(got, data['z64'])
    print(f'honest fp32 -> bf16: worst err / limit {w:.3f}, bias {b:+.5f} ulp')
    assert w <= 1.0
    assert abs(b) <= sm.BIAS_MAX
    # and as an fp32 output it is inside its own limit by construction (4 x its own error)
    assert sm.worst_f32(data['z32'], data['z64'], data['lim']) <= 1.0


def test_truncating_store_is_rejected(data):
    got = truncate_to_bf16(data['z32'])
    w = sm.worst_bf16(got, data['z64'], data['lim'])
    b = sm.rounding_bias(got, data['z64'])
    print(f'truncating store: worst err / limit {w:.3f}, bias {b:+.5f} ulp')
    assert w > 1.0                      # up to one ulp off: twice the allowance
    assert b < -0.4                     # -0.5 in expectation
    assert abs(b) > sm.BIAS_MAX


def test_silu_rounded_before_the_residual_add_is_rejected(data):
    got = (data['s32'].to(torch.bfloat16).float() + data['res'].float()).to(torch.bfloat16)
    w = sm.worst_bf16(got, data['z64'], data['lim'])
    print(f'SiLU rounded before the add: worst err / limit {w:.3f}')
    assert w > 1.0


def test_residual_one_pixel_off_is_rejected(data):
    res = torch.roll(data['res'], 1, dims=2)
    got = sm.silu_apply(data['y'], data['scale'], data['shift'], res, torch.float32)[0].to(torch.bfloat16)
    w = sm.worst_bf16(got, data['z64'], data['lim'])
    assert w > 100.0


def test_dropped_second_chunk_is_rejected(data):
    got = data['z32'].to(torch.bfloat16).clone()
    cpp = C // 8
    got.view(B, H, W * cpp, 8)[:, :, 256:512] = 0
    w = sm.worst_bf16(got, data['z64'], data['lim'])
    assert w > 100.0


def test_sum_limit_holds_for_any_order_of_fp32_additions():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(4096, 16, generator=g)
    exact = x.double().sum(0)
    lim = sm.sum_limit(4096, x.double().abs().sum(0))
    seq = torch.zeros(16)
    for i in range(4096):               # the worst order: one long chain
        seq = seq + x[i]
    assert ((seq.double() - exact).abs() <= lim).all()
    assert ((x.sum(0).double() - exact).abs() <= lim).all()
    # a dropped term is far outside
    assert ((x[1:].sum(0).double() - exact).abs() > lim).any()
