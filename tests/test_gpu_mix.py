"""MixUp and CutMix on the GPU (fva_mix_plan, fva_mix_apply, BatchMix): the apply pass with plans written by the test (copies bit for
bit, MixUp within half an ulp of float64 by tests/streaming_measure.py's rule, boxes at every edge); 4096 sequential ticks of the plan
kernel per setting against the float64 restatement (tests/mix_restatement.py) and against the moments of Beta(alpha, alpha); and a whole
train step of a tiny classifier head with BatchMix and label smoothing: no host synchronisation, no ATen mixing or loss, a captured step
bit-identical with the eager one, a new plan on every replay."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import mix_restatement as mr
import streaming_measure as sm

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16


def _apply(x, plan):
    """fva_mix_apply through the C ABI into a buffer pre-filled with NaN."""
    from fastvision_amd import _lib
    from fastvision_amd.ops import _code, _p, _stream
    xd, pd = x.to(DEV).contiguous(), plan.to(DEV)
    out = torch.full_like(xd, float('nan'))
    B, C_, H, W = x.shape
    _lib.call('fva_mix_apply', _code(x.dtype), _p(xd), _p(out), _p(pd), B, C_, H, W, _stream())
    return out.cpu()


def _bits(t):
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


def _boxes(H, W):
    """(x1, y1, x2, y2): clipped at the left, right, top and bottom edge, empty, the whole image, one in the middle off the 16-byte grid"""
    return [(0, H // 4, W // 3 + 1, H - 1), (W - W // 3 - 1, 1, W, H - 1), (W // 5, 0, W - W // 5 - 1, H // 3 + 1), (1, H - H // 3 - 1, W - 2, H),
            (W // 2, H // 2, W // 2, H // 2), (0, 0, W, H), (W // 3, H // 3, W // 3 + 3, H // 3 + 2)]


@pytest.mark.parametrize('dtype', [F32, BF16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('H,W', [(5, 7), (64, 64)])
@pytest.mark.parametrize('B', [1, 2, 3])
def test_apply_modes_against_float64(B, H, W, dtype):
    gen = torch.Generator().manual_seed(B * 100 + H)
    x = (torch.randn(B, 3, H, W, generator=gen) * 3).to(dtype)
    special = x.clone()                                             # the copies must keep every bit: NaN, -0.0, inf, a denormal
    special[0, 0, 0, 0], special[0, 1, 1, 1], special[-1, 2, 2, 2], special[-1, 0, 3, 3] = float('nan'), -0.0, float('inf'), 1e-40
    # mode 0, and B == 1 in every mode: the input
    assert torch.equal(_bits(_apply(special, mr.plan_words(0, 1.0, 1.0))), _bits(special))
    if B == 1:
        for plan in (mr.plan_words(1, 0.3, 0.3), mr.plan_words(2, 0.3, 0.5, 1, 1, 0, 0, W, H)):
            assert torch.equal(_bits(_apply(special, plan)), _bits(special))
        return
    # MixUp: fmaf(lam, x, (1 - lam) * partner) rounded once
    worst = {}
    for lam in (0.3, 0.0, 1.0, 0.9999999):
        lam = float(np.float32(lam))
        got = _apply(x, mr.plan_words(1, lam, lam))
        ref64, mag, _ = mr.apply(x, 1, lam, None, F64)
        ref32, _, _ = mr.apply(x, 1, lam, None, F32)
        worst[lam] = sm.check(got, ref64, ref32, mag, dtype == BF16, what=f'MixUp lam {lam}')
    print(f'apply B {B} {H}x{W} {dtype}: MixUp worst err / limit {worst}')
    # CutMix: the partner's bits inside the box, the image's own outside; lam and lam_raw are not read
    for box in _boxes(H, W):
        x1, y1, x2, y2 = box
        got = _apply(special, mr.plan_words(2, 0.123, 0.456, 0, 0, x1, y1, x2, y2))
        want, _, inside = mr.apply(special, 2, None, box, special.dtype)
        assert inside.sum().item() == (x2 - x1) * (y2 - y1)
        assert torch.equal(_bits(got), _bits(want)), box


def test_apply_at_an_unaligned_address_and_odd_width():
    """a view that starts 4 bytes into an allocation, and W = 12 (bf16: not a multiple of the 8-element chunk): the element path"""
    gen = torch.Generator().manual_seed(3)
    from fastvision_amd import _lib
    from fastvision_amd.ops import _code, _p, _stream
    for dtype, W in ((F32, 8), (BF16, 12)):
        n, off = 2 * 3 * 4 * W, 2 if dtype == BF16 else 1
        base = (torch.randn(n + off, generator=gen) * 2).to(dtype).to(DEV)
        x = base[off:].view(2, 3, 4, W)
        assert (x.data_ptr() % 16 != 0) or W % 8
        out = torch.full((n + off,), float('nan'), dtype=dtype, device=DEV)
        o = out[off:].view(2, 3, 4, W)
        plan = mr.plan_words(2, 0.5, 0.5, 0, 0, 3, 1, 7, 3).to(DEV)
        _lib.call('fva_mix_apply', _code(dtype), _p(x), _p(o), _p(plan), 2, 3, 4, W, _stream())
        want, _, _ = mr.apply(x.cpu(), 2, None, (3, 1, 7, 3), dtype)
        assert torch.equal(_bits(o.cpu()), _bits(want))
        assert torch.isnan(out[:off]).all().item()                                   # nothing in front of the view was written


# ---------------------------------------------------------------------------------------------------------------- the plan
def _ticks(seed, args, n):
    """n sequential launches of fva_mix_plan into the rows of one [n, 9] buffer: read back once.  Returns (plans int32 [n, 9], state)."""
    from fastvision_amd import _lib
    from fastvision_amd.ops import _p, _stream
    import ctypes as C
    state = torch.tensor([seed, 0, 0, 0], dtype=torch.int64, device=DEV)
    plans = torch.full((n, mr.PLAN_WORDS), -1, dtype=torch.int32, device=DEV)
    ma, ca, prob, sw, H, W = args
    base, stream, sp = plans.data_ptr(), _stream(), _p(state)
    for i in range(n):
        _lib.call('fva_mix_plan', sp, ma, ca, prob, sw, H, W, C.c_void_p(base + 4 * mr.PLAN_WORDS * i), stream)
    return plans.cpu(), state.cpu()


@pytest.fixture(scope='module')
def ticked():
    return {seed: (_ticks(seed, args, mr.PLAN_TICKS), mr.plan(seed, 0, mr.PLAN_TICKS, *args), args) for seed, args in mr.PLAN_SETTINGS}


def _within(got, want, sigma, what):
    assert abs(got - want) <= 5 * sigma + 1e-12, f'{what}: {got} against {want}, 5 sigma = {5 * sigma}'
    return (got - want) / sigma if sigma > 0 else 0.0


@pytest.mark.parametrize('seed', [s for s, _ in mr.PLAN_SETTINGS])
def test_plan_ticks_against_the_restatement(ticked, seed):
    (plans, state), p, args = ticked[seed]
    ma, ca, prob, sw, H, W = args
    n = mr.PLAN_TICKS
    assert state.tolist() == [seed, n, 0, 0]                                       # the launches advanced the counter themselves
    w = plans.numpy()
    mode, rx, ry, x1, y1, x2, y2 = (w[:, i].astype(np.int64) for i in (0, 3, 4, 5, 6, 7, 8))
    lam_raw, lam = (np.ascontiguousarray(w[:, i]).view(np.float32) for i in (1, 2))
    und_accept = p['und_accept']
    ok = ~und_accept                                                               # an undecidable acceptance changes every later word of its tick
    assert (mode[ok] == p['mode'][ok]).all() and (rx[ok] == p['rx'][ok]).all() and (ry[ok] == p['ry'][ok]).all()
    lim = mr.lam_raw_limit(p['lam_raw'], p['lam_raw32'])
    err = np.abs(lam_raw.astype(np.float64) - p['lam_raw'])
    assert (err[ok] <= lim[ok]).all(), (err[ok] / lim[ok]).max()
    cut, mix, none = mode == 2, mode == 1, mode == 0
    # lam: exact from the device's own box in fp32; MixUp: lam_raw's bits; none: 1
    assert (lam[cut] == mr.lam_of_box(x1, y1, x2, y2, H, W)[cut]).all()
    assert (lam[mix].view(np.int32) == lam_raw[mix].view(np.int32)).all() and (lam[none] == 1).all() and (lam_raw[none] == 1).all()
    assert not (w[~cut, 3:] != 0).any()
    # the box: the restatement's; where r * W or r * H is within the fp32 limit of an integer, either neighbour
    sel = cut & ok
    match = np.zeros(n, dtype=bool)
    for dw in (0, -1, 1):
        for dh in (0, -1, 1):
            bx = mr.box_of(p['rx'], p['ry'], p['hw'] + dw, p['hh'] + dh, H, W)
            same = (bx[0] == x1) & (bx[1] == y1) & (bx[2] == x2) & (bx[3] == y2)
            match |= same & ((dw == 0) | p['und_w']) & ((dh == 0) | p['und_h'])
    assert match[sel].all(), np.nonzero(sel & ~match)[0][:8]
    und = und_accept | p['und_w'] | p['und_h']
    assert und.mean() <= 0.001
    # shares and moments within 5 sigma (the rule of the dropout test)
    report = {}
    applied = mode > 0
    report['applied'] = _within(applied.mean(), prob, np.sqrt(prob * (1 - prob) / n), 'applied share')
    na = int(applied.sum())
    report['cutmix'] = _within(cut.sum() / na, sw, np.sqrt(sw * (1 - sw) / na), 'CutMix share')
    for name, which, alpha in (('mixup', mix, ma), ('cutmix', cut, ca)):
        mean, var, mu4 = mr.beta_moments(alpha)
        v = lam_raw[which].astype(np.float64)
        report[f'{name} mean'] = _within(v.mean(), mean, np.sqrt(var / v.size), f'mean of lam_raw, alpha {alpha}')
        report[f'{name} var'] = _within(v.var(), var, np.sqrt((mu4 - var * var) / v.size), f'variance of lam_raw, alpha {alpha}')
    print(f'plan seed {seed} {args}: worst lam_raw err / limit {(err[ok] / lim[ok]).max():.3f}, deviations in sigma {report}')


def test_plan_same_seed_same_bits_another_seed_differs(ticked):
    seed, args = mr.PLAN_SETTINGS[0]
    (plans, _), _, _ = ticked[seed]
    again, state = _ticks(seed, args, 256)
    other, _ = _ticks(seed + 1, args, 256)
    assert state.tolist() == [seed, 256, 0, 0]
    assert torch.equal(again, plans[:256]) and not torch.equal(other, plans[:256])


def test_plan_single_modes_and_off():
    for args, modes in (((0.0, 1.0, 1.0, 0.5, 16, 16), {2}), ((0.4, 0.0, 1.0, 0.5, 16, 16), {1}), ((0.0, 0.0, 1.0, 0.5, 16, 16), {0}),
                        ((0.2, 1.0, 0.0, 0.5, 16, 16), {0})):
        plans, state = _ticks(9, args, 64)
        assert set(plans[:, 0].tolist()) == modes and state[1].item() == 64, args
        want = mr.plan(9, 0, 64, *args)
        assert (plans[:, 0].numpy() == want['mode']).all()


# ---------------------------------------------------------------------------------------------------------------- the whole step
class _Head(nn.Module):
    """global average pooling and one Linear, both on the library's kernels: the smallest classifier"""

    def __init__(self, channels=64, num_classes=16):
        super().__init__()
        self.fc = nn.Linear(channels, num_classes)

    def forward(self, x):
        from fastvision_amd import fc_ops, ops
        return fc_ops.linear(ops.global_avg_pool(x), self.fc)


def _parts(seed=3, mix_seed=5):
    from fastvision_amd import BatchMix, FusedSGD
    from fastvision_amd.loss import CrossEntropyLoss
    torch.manual_seed(seed)
    net = _Head().to(DEV).train()
    opt = FusedSGD(net.parameters(), lr=0.05, momentum=0.9, nesterov=True, weight_decay=5e-4, capturable=True)
    return net, CrossEntropyLoss(label_smoothing=0.1), opt, BatchMix(seed=mix_seed).to(DEV)


def _batches(n, B=4):
    gen = torch.Generator().manual_seed(17)
    return [(torch.randn(B, 64, 8, 8, generator=gen).to(DEV), torch.randint(0, 16, (B, 1), generator=gen).float().to(DEV)) for _ in range(n)]


def _step(net, crit, opt, mix, images, labels):
    images, labels = mix(images, labels)
    pred = net(images)
    opt.zero_grad(set_to_none=True)
    loss = crit(pred, labels)
    loss.backward()
    opt.step()
    return loss.detach().clone()


def test_step_with_batchmix_runs_two_mix_launches_no_aten_and_no_host_sync(monkeypatch):
    from fastvision_amd import MixedLabels, _lib
    net, crit, opt, mix = _parts()
    (images, labels), = _batches(1)
    for _ in range(2):
        _step(net, crit, opt, mix, images, labels)                 # warm-up: packed weights, optimizer tables
    torch.cuda.synchronize()

    def refuse(*a, **k):
        raise AssertionError('ATen op in the mixed train step')
    for name in ('cross_entropy', 'log_softmax', 'linear', 'adaptive_avg_pool2d', 'one_hot'):
        monkeypatch.setattr(F, name, refuse)
    for name in ('roll', 'lerp'):
        monkeypatch.setattr(torch, name, refuse)
    for name in ('roll', 'lerp_', 'lerp', 'scatter_'):
        monkeypatch.setattr(torch.Tensor, name, refuse)
    seen = []
    monkeypatch.setattr(_lib, 'tracer', lambda name, args: seen.append(name))
    torch.cuda.set_sync_debug_mode('error')
    try:
        mixed, target = mix(images, labels)
        assert seen == ['fva_mix_plan', 'fva_mix_apply'] and isinstance(target, MixedLabels) and target.plan is mix._plan
        loss = _step(net, crit, opt, mix, images, labels)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert 'fva_softmax_ce_soft' in seen and 'fva_softmax_ce' not in seen
    assert torch.isfinite(loss).item() and mixed.shape == images.shape and mixed.dtype == images.dtype
    assert mix._state.cpu().tolist() == [5, 4, 0, 0]
    mix.eval()
    a, b = mix(images, labels)
    assert a is images and b is labels and mix._state.cpu().tolist() == [5, 4, 0, 0]


def test_graphed_step_with_batchmix_is_bit_identical_with_eager_and_draws_a_new_plan_per_replay():
    from fastvision_amd import ops
    from fastvision_amd.graphs import GraphedTrainStep
    batches = _batches(3)
    prev = ops.set_wgrad_side_stream(False)                         # the single-stream capture equals the eager single-stream step
    try:
        net, crit, opt, mix = _parts()
        want, want_plans = [], []
        for im, lab in batches:
            want.append(_step(net, crit, opt, mix, im, lab))
            want_plans.append(mix._plan.clone())
        torch.cuda.synchronize()
    finally:
        ops.set_wgrad_side_stream(prev)
    net2, crit2, opt2, mix2 = _parts()
    step = GraphedTrainStep(net2, lambda p, t: crit2(p, t), opt2, batches[0][0], batches[0][1], mix=mix2)
    torch.cuda.synchronize()
    assert mix2._state.cpu().tolist() == [5, 0, 0, 0]               # warm-up and capture left the state where it was
    got, got_plans = [], []
    for im, lab in batches:
        got.append(step(im, lab).clone())
        got_plans.append(mix2._plan.clone())
    torch.cuda.synchronize()
    assert mix2._state.cpu().tolist() == [5, 3, 0, 0] and mix._state.cpu().tolist() == [5, 3, 0, 0]
    for a, b in zip(got, want):
        assert torch.equal(a, b), (a, b)
    for a, b in zip(got_plans, want_plans):
        assert torch.equal(a, b)
    assert not torch.equal(got_plans[0], got_plans[1]) and not torch.equal(got_plans[1], got_plans[2])      # a new plan on every replay
    ref = mr.plan(5, 0, 3, 0.2, 1.0, 1.0, 0.5, 8, 8)
    assert [int(p[0]) for p in got_plans] == ref['mode'].tolist()
    for (k, p), q in zip(net.state_dict().items(), net2.state_dict().values()):
        assert torch.equal(p, q), k
    for p, q in zip(net.parameters(), net2.parameters()):
        assert torch.equal(opt.state[p]['momentum_buffer'], opt2.state[q]['momentum_buffer'])
