"""fva_softmax_ce_soft on the GPU: every loss value and every gradient element against the float64 restatement of the same formula
(tests/mix_restatement.py: soft_ce_limits, the rule of tests/test_gpu_losses.py's cross-entropy rows), for the three target forms --
plain labels with smoothing, a mixed pair of labels with lambda read from a plan buffer on the device, dense probability rows --, the
NaN rows of an invalid label, bit-equality with fva_softmax_ce at smoothing 0 without a plan, and no gradient buffer under no_grad.
Accuracy(topk=) against torch.topk and against the stated rule on ties and NaN."""
import numpy as np
import pytest
import torch

import loss_restatement as lr
import mix_restatement as mr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LAM = float(np.float32(0.3))


def _logits(R, C_, gen, big=False):
    z = torch.randn(R, C_, generator=gen) * 4
    if big:                                                          # logits at +-80: exp(-160) underflows next to the maximum
        z = torch.where(torch.rand(R, C_, generator=gen) < 0.5, torch.full_like(z, 80.0), torch.full_like(z, -80.0)) + z * 0.01
    return z


def _dense(R, C_, gen, unnormalised=False):
    d = torch.softmax(torch.randn(R, C_, generator=gen) * 2, 1)
    if unnormalised:
        d[R - 1] *= 1.75                                             # a row that does not sum to 1
        d[0] *= 0.5
    return d


#        C     R  eps  form      lam   weights mean   labels  logits
CASES = [(1, 1, 0.0, 'pair', LAM, False, True, 'i64', 'randn'),
         (1, 5, 1.0, 'plain', None, True, False, 'f32', 'randn'),
         (7, 2, 0.1, 'pair', LAM, True, True, 'i64', 'randn'),
         (7, 5, 0.1, 'pair_same', LAM, False, False, 'f32', 'randn'),
         (7, 5, 0.0, 'dense', None, True, True, None, 'randn'),
         (1000, 1, 0.1, 'plain', None, False, True, 'i64', 'randn'),
         (1000, 5, 0.1, 'pair', LAM, True, True, 'f32', 'randn'),
         (1000, 5, 0.1, 'pair', 0.0, False, True, 'i64', 'randn'),
         (1000, 2, 1.0, 'pair', 1.0, False, False, 'i64', 'randn'),
         (1000, 5, 0.1, 'pair', LAM, False, True, 'i64', 'big'),
         (1000, 5, 1.0, 'plain', None, True, False, 'i64', 'big'),
         (1000, 2, 0.1, 'dense_unnormalised', None, False, False, None, 'big'),
         (1025, 5, 0.0, 'pair', LAM, True, False, 'i64', 'randn'),
         (1025, 2, 0.1, 'dense_unnormalised', None, True, True, None, 'randn'),
         (1025, 5, 1.0, 'dense', None, False, True, None, 'randn')]


def _run(z, target, eps, mean, w, need_grad=True):
    from fastvision_amd.loss import CrossEntropyLoss
    zd = z.to(DEV).requires_grad_(need_grad)
    loss = CrossEntropyLoss('mean' if mean else 'sum', label_smoothing=eps)(zd, target, None if w is None else w.to(DEV))
    if need_grad:
        loss.backward()
    return loss.detach(), zd.grad


@pytest.mark.parametrize('case', CASES, ids=lambda c: '-'.join(str(v) for v in c))
def test_soft_ce_every_value_and_gradient_element_against_float64(case):
    from fastvision_amd import MixedLabels
    C_, R, eps, form, lam, weighted, mean, labdt, kind = case
    gen = torch.Generator().manual_seed(C_ * 131 + R * 7 + int(eps * 10))
    z = _logits(R, C_, gen, kind == 'big')
    w = torch.rand(R, generator=gen) + 0.25 if weighted else None
    y = torch.randint(0, C_, (R,), generator=gen)
    if form == 'pair_same':
        y[1] = y[0]                                                  # both partners of row 1 carry the same label
        y[3] = y[2]
    kw = dict(eps=eps, weights=w, mean=mean)
    if form.startswith('dense'):
        dense = _dense(R, C_, gen, form.endswith('unnormalised'))
        kw['dense'] = dense
        target = dense.to(DEV)
    else:
        kw['labels'] = y
        lab = (y if labdt == 'i64' else y.float().view(-1, 1)).to(DEV)
        if form.startswith('pair'):
            kw['lam'] = lam
            target = MixedLabels(lab, mr.plan_words(1, lam, lam).to(DEV))
        else:
            target = lab
    r64, vlim, glim = mr.soft_ce_limits(z, **kw)
    got, grad = _run(z, target, eps, mean, w)
    wv, wg = lr.worst(got, r64['value'], vlim), lr.worst(grad, r64['grad'], glim)
    print(f'soft CE {case}: value {got.item():.7g} (float64 {r64["value"].item():.7g}) worst err / limit value {wv:.3f} gradient {wg:.3f}')
    assert got.shape == () and wv <= 1.0 and wg <= 1.0, (wv, wg)


def test_invalid_label_makes_the_rows_that_use_it_nan_and_no_other():
    from fastvision_amd import MixedLabels
    gen = torch.Generator().manual_seed(21)
    R, C_ = 5, 7
    z = _logits(R, C_, gen)
    y = torch.randint(0, C_, (R,), generator=gen)
    plan = mr.plan_words(1, LAM, LAM).to(DEV)
    r64, _, glim = mr.soft_ce_limits(z, labels=y, lam=LAM, eps=0.1)
    for bad in (C_, -1, 2.5, float('nan'), 10 ** 12):
        lab = y.float() if isinstance(bad, float) else y.clone()
        lab[1] = bad
        loss, g = _run(z, MixedLabels(lab.to(DEV), plan), 0.1, True, None)          # pair form: rows 1 and 2 use label 1
        assert torch.isnan(loss).item(), bad
        g = g.cpu()
        assert torch.isnan(g[[1, 2]]).all(), bad
        assert lr.worst(g[[0, 3, 4]], r64['grad'][[0, 3, 4]], glim[[0, 3, 4]]) <= 1.0, bad
        loss, g = _run(z, lab.to(DEV), 0.1, True, None)                             # plain form: row 1 alone
        r1, _, glim1 = mr.soft_ce_limits(z, labels=y, eps=0.1)
        assert torch.isnan(loss).item() and torch.isnan(g[1]).all().item()
        assert lr.worst(g.cpu()[[0, 2, 3, 4]], r1['grad'][[0, 2, 3, 4]], glim1[[0, 2, 3, 4]]) <= 1.0, bad
    lab = y.clone()
    lab[R - 1] = C_                                                                  # the last row's label is also row 0's partner
    _, g = _run(z, MixedLabels(lab.to(DEV), plan), 0.1, True, None)
    assert torch.isnan(g[[0, R - 1]]).all().item() and torch.isfinite(g[1:R - 1]).all().item()


@pytest.mark.parametrize('R,C_', [(1, 1), (5, 7), (5, 1000), (2, 1025)])
def test_bit_equal_with_softmax_ce_at_zero_smoothing_without_a_plan(R, C_):
    from fastvision_amd import _lib
    from fastvision_amd.ops import _p, _stream
    gen = torch.Generator().manual_seed(R + C_)
    z = _logits(R, C_, gen, big=C_ == 1000).to(DEV)
    w = (torch.rand(R, generator=gen) + 0.25).to(DEV)
    y = torch.randint(0, C_, (R,), generator=gen)
    ws = torch.empty(max(_lib.load().fva_softmax_ce_workspace(R), 4), dtype=torch.uint8, device=DEV)
    for lab, code in ((y.to(DEV), _lib.LABEL_I64), (y.float().to(DEV), _lib.LABEL_F32)):
        for red in (_lib.REDUCE_MEAN, _lib.REDUCE_SUM):
            for wt in (None, w):
                outs = []
                for soft in (False, True):
                    out = torch.full((1,), float('nan'), device=DEV)
                    grad = torch.full((R, C_), float('nan'), device=DEV)
                    if soft:
                        _lib.call('fva_softmax_ce_soft', _p(z), _p(lab), code, None, _p(wt), R, C_, red, 0.0, None, _p(out), _p(grad), _p(ws), _stream())
                    else:
                        _lib.call('fva_softmax_ce', _p(z), _p(lab), code, _p(wt), R, C_, red, _p(out), _p(grad), _p(ws), _stream())
                    outs.append((out, grad))
                (o0, g0), (o1, g1) = outs
                assert torch.equal(o0.view(torch.int32), o1.view(torch.int32)) and torch.equal(g0.view(torch.int32), g1.view(torch.int32)), (code, red, wt is None)


def test_default_arguments_launch_the_old_kernel_and_no_grad_allocates_no_gradient(monkeypatch):
    from fastvision_amd import MixedLabels, _lib
    from fastvision_amd.loss import CrossEntropyLoss
    seen = []
    monkeypatch.setattr(_lib, 'tracer', lambda name, args: seen.append((name, args)))
    gen = torch.Generator().manual_seed(5)
    z, y = torch.randn(4, 9, generator=gen).to(DEV).requires_grad_(True), torch.randint(0, 9, (4,), generator=gen).to(DEV)
    CrossEntropyLoss()(z, y)
    assert [n for n, _ in seen] == ['fva_softmax_ce']
    seen.clear()
    plan = mr.plan_words(1, LAM, LAM).to(DEV)
    with torch.no_grad():
        loss = CrossEntropyLoss(label_smoothing=0.1)(z, MixedLabels(y, plan))
    assert not loss.requires_grad and [n for n, _ in seen] == ['fva_softmax_ce_soft']
    assert seen[0][1][11].value is None                                             # the grad argument: a null pointer
    seen.clear()
    CrossEntropyLoss(label_smoothing=0.1)(z, y).backward()
    assert seen[0][0] == 'fva_softmax_ce_soft' and seen[0][1][11].value is not None
    r64 = mr.soft_ce(z.detach().cpu(), torch.float64, labels=y.cpu(), lam=LAM, eps=0.1)
    assert abs(loss.item() - r64['value'].item()) <= 1e-5 * abs(r64['value'].item())


# ---------------------------------------------------------------------------------------------------------------- top-k accuracy
def test_topk_accuracy_against_torch_topk_and_the_stated_rule():
    from fastvision_amd.metrics import Accuracy
    gen = torch.Generator().manual_seed(6)
    R, C_ = 301, 1000
    z = torch.randn(R, C_, generator=gen)                            # tie-free: torch.topk decides
    y = torch.randint(0, C_, (R,), generator=gen)
    order = z.argsort(1, descending=True)
    y[:150] = order[torch.arange(150), torch.arange(150) % 8]        # ranks 0 ... 7: both sides of k = 5
    for dt in (torch.float32, torch.bfloat16):
        zz = z.to(dt)
        if dt == torch.float32:
            want = (zz.topk(5, 1)[1] == y[:, None]).any(1).float().sum(0, keepdim=True) / R
        else:
            want = mr.topk_hits(zz, y, 5).float().sum(0, keepdim=True) / R      # bf16 rounding makes ties: the stated rule decides
        for lab in (y, y.float()):
            got = Accuracy(topk=5)(zz.to(DEV), lab.to(DEV))
            assert got.device.type == 'cuda' and got.shape == (1,) and torch.equal(got.cpu(), want), (dt, got.item(), want.item())
    # ties and NaN: exactly the stated rule; k = 1 equals the existing top-1
    t = torch.randn(64, 33, generator=gen)
    t[0] = 0.25                                                      # all equal: label j has j entries ahead of it
    t[1, 4] = t[1, 20] = 9.0
    t[2, 7] = float('nan')
    t[3, 30] = t[3, 2] = float('nan')
    t[4] = float('nan')
    t[5, ::2] = 1.0
    yy = torch.randint(0, 33, (64,), generator=gen)
    yy[0], yy[1], yy[2], yy[3], yy[4], yy[5], yy[6], yy[7] = 4, 20, 7, 30, 5, 8, -2, 33
    for k in (1, 2, 5, 6, 33, 40):
        want = mr.topk_hits(t, yy, k).float().sum(0, keepdim=True) / 64
        got = Accuracy(topk=k)(t.to(DEV), yy.to(DEV))
        assert torch.equal(got.cpu(), want), (k, got.item(), want.item())
    assert torch.equal(Accuracy(topk=1)(t.to(DEV), yy.to(DEV)), Accuracy()(t.to(DEV), yy.to(DEV)))
    from fastvision_amd import _lib
    from fastvision_amd.ops import _p, _stream
    out = torch.empty(1, device=DEV)
    ws = torch.empty(64, dtype=torch.int32, device=DEV)
    td, yd = t.to(DEV), yy.to(DEV)
    _lib.call('fva_topk_accuracy', _p(td), _lib.F32, _p(yd), _lib.LABEL_I64, 64, 33, 1, _p(out), _p(ws), _stream())
    assert torch.equal(out, Accuracy()(td, yd))
