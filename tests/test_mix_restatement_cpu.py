"""CPU-side tests of label smoothing, MixUp and CutMix (no GPU): tests/mix_restatement.py pinned against torch and against the known
moments of the Beta distribution, the chosen plan seeds free of undecidable draws, the C ABI of the four new entry points (version 12,
exports, refusals before anything is launched), CrossEntropyLoss's CPU branch with smoothing, probability and mixed targets,
Accuracy(topk=) on CPU tensors, and the host logic of Fit(mix=) and BatchMix."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mix_restatement as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('fva_mix_plan', 'fva_mix_apply', 'fva_softmax_ce_soft', 'fva_topk_accuracy')
F64 = torch.float64


@pytest.fixture(scope='module')
def built():
    import __graft_entry__ as ge
    ge.build()
    from fastvision_amd import _lib
    return _lib


# ---------------------------------------------------------------------------------------------------------------- the restatements
def _pair_probs(y, lam, C_):
    oh = F.one_hot(y, C_).double()
    return lam * oh + (1 - lam) * oh.roll(1, 0)


@pytest.mark.parametrize('eps', [0.0, 0.1, 1.0])
def test_soft_ce_restatement_against_torch(eps):
    gen = torch.Generator().manual_seed(12)
    R, C_ = 6, 11
    z = torch.randn(R, C_, generator=gen, dtype=F64) * 3
    y = torch.randint(0, C_, (R,), generator=gen)
    w = torch.rand(R, generator=gen, dtype=F64) + 0.25
    e = float(np.float32(eps))                                      # the restatement takes eps as the C ABI does: an fp32 value
    lam = float(np.float32(0.3))
    dense = torch.softmax(torch.randn(R, C_, generator=gen, dtype=F64), 1)
    forms = [(dict(labels=y), y), (dict(labels=y, lam=lam), _pair_probs(y, lam, C_)), (dict(dense=dense), dense)]
    for kw, target in forms:
        for mean in (True, False):
            leaf = z.clone().requires_grad_(True)
            want = F.cross_entropy(leaf, target, label_smoothing=e, reduction='mean' if mean else 'sum')
            want.backward()
            got = mr.soft_ce(z, F64, eps=eps, mean=mean, **kw)
            assert abs(got['value'] - want.detach()) <= 1e-12 * abs(want.detach()), (kw.keys(), mean)
            assert (got['grad'] - leaf.grad).abs().max() <= 1e-13, (kw.keys(), mean)
    # weights: torch has no per-row weights; rows = w * unweighted rows
    a, b = mr.soft_ce(z, F64, labels=y, eps=eps, weights=w, mean=False), mr.soft_ce(z, F64, labels=y, eps=eps, mean=False)
    assert torch.allclose(a['rows'], b['rows'] * w, rtol=1e-14, atol=0) and torch.allclose(a['grad'], b['grad'] * w[:, None], rtol=1e-14, atol=0)
    # a dense row that does not sum to 1: torch's expression -sum(q log_softmax)
    d2 = dense * torch.tensor([1.0, 0.5, 2.0, 1.0, 0.0, 1.5], dtype=F64)[:, None]
    leaf = z.clone().requires_grad_(True)
    want = F.cross_entropy(leaf, d2, label_smoothing=e, reduction='sum')
    want.backward()
    got = mr.soft_ce(z, F64, dense=d2, eps=eps, mean=False)
    assert abs(got['value'] - want.detach()) <= 1e-12 * abs(want.detach()) and (got['grad'] - leaf.grad).abs().max() <= 1e-13


def test_soft_ce_limits_are_positive_and_see_a_wrong_formula():
    gen = torch.Generator().manual_seed(2)
    z = torch.randn(5, 1000, generator=gen) * 4
    y = torch.randint(0, 1000, (5,), generator=gen)
    r64, vlim, glim = mr.soft_ce_limits(z, labels=y, lam=0.3, eps=0.1)
    assert vlim > 0 and (glim > 0).all() and vlim < 1e-3 * r64['value'].abs() and glim.max() < (1000 + 6) * 2.0 ** -24 / 5
    for kw in (dict(lam=0.3, eps=0.11), dict(lam=0.31, eps=0.1), dict(lam=None, eps=0.1)):     # each mistake is far outside the limits
        wrong = mr.soft_ce(z, F64, labels=y, **kw)
        assert abs(wrong['value'] - r64['value']) > 4 * vlim and ((wrong['grad'] - r64['grad']).abs() > 4 * glim).any(), kw


def test_uniform_and_words():
    assert mr.uniform(0) == 2.0 ** -25 and mr.uniform(5 << 8) == 5.5 * 2.0 ** -24 and mr.uniform(0x7FFFFFFF) == (2 ** 23 - 0.5) * 2.0 ** -24
    # from 2^23 on fp32 has no half: ties to even
    assert mr.uniform(0x80000000) == 0.5 and mr.uniform(0x80000100) == (2 ** 23 + 2) * 2.0 ** -24 and mr.uniform(0xFFFFFFFF) == 1.0
    w = mr.tick_words(9, np.array([0, 1, 2 ** 33], dtype=np.uint64), 0)
    from vgg_restatement import philox4x32_10
    one = philox4x32_10(np.array([0], dtype=np.uint64), 0, 0, 2, 9, 0)                     # tick 2^33: counter hi = 2
    assert all(int(w[i][2]) == int(one[i][0]) for i in range(4))


@pytest.mark.parametrize('alpha', [0.2, 1.0, 0.05])
def test_johnk_moments(alpha):
    """mean 1/2, variance 1 / (4 (2 alpha + 1)) within 5 sigma; alpha = 0.05 reaches the log-space branch (U^20 underflows)"""
    n = 20000
    lam, lam32, und = mr.johnk(11, np.arange(n, dtype=np.uint64), alpha)
    mean, var, mu4 = mr.beta_moments(alpha)
    assert ((lam >= 0) & (lam <= 1)).all()
    assert abs(lam.mean() - mean) <= 5 * np.sqrt(var / n)
    assert abs(lam.var() - var) <= 5 * np.sqrt((mu4 - var * var) / n)
    assert np.abs(lam32.astype(np.float64) - lam).max() <= 1e-4


def test_johnk_log_branch_equals_the_direct_form_where_both_exist():
    U, V = np.array([0.3, 0.6, 1e-3]), np.array([0.2, 0.1, 0.5])
    XpY, val = mr.johnk_pair(U, V, np.full(3, 0.5))
    lx, ly = np.log(U) / 0.5, np.log(V) / 0.5
    lm = np.maximum(lx, ly)
    logform = np.exp(lx - lm - np.log(np.exp(lx - lm) + np.exp(ly - lm)))
    assert np.allclose(val, logform, rtol=1e-13) and np.allclose(XpY, U ** 2 + V ** 2)
    tiny = mr.johnk_pair(np.array([2.0 ** -25]), np.array([2.0 ** -24]), np.array([0.01]))      # X + Y underflows to 0
    assert tiny[0][0] == 0.0 and 0.0 <= tiny[1][0] <= 1.0 and np.isclose(tiny[1][0], 2.0 ** -100 / (1 + 2.0 ** -100))


def test_plan_seeds_have_no_undecidable_draw_and_boxes_are_consistent():
    for seed, args in mr.PLAN_SETTINGS:
        p = mr.plan(seed, 0, mr.PLAN_TICKS, *args)
        H, W = args[4], args[5]
        assert not (p['und_accept'] | p['und_w'] | p['und_h']).any(), (seed, args)
        cut, mix, none = p['mode'] == 2, p['mode'] == 1, p['mode'] == 0
        assert cut.any() and mix.any() and (none.any() == (args[2] < 1.0))
        assert ((p['x1'] >= 0) & (p['x2'] <= W) & (p['x1'] <= p['x2']) & (p['y1'] >= 0) & (p['y2'] <= H) & (p['y1'] <= p['y2'])).all()
        assert ((p['rx'] >= 0) & (p['rx'] < W) & (p['ry'] >= 0) & (p['ry'] < H)).all()
        assert (p['lam'][none] == 1).all() and (p['lam'][mix] == p['lam_raw'][mix].astype(np.float32)).all()
        area = (p['x2'] - p['x1']) * (p['y2'] - p['y1'])
        assert np.allclose(p['lam'][cut], 1 - area[cut] / (H * W), atol=1e-6)
    # another seed or another starting counter gives other plans; the same arguments the same
    a, b, c = mr.plan(3, 0, 64, 0.2, 1.0, 1.0, 0.5, 64, 64), mr.plan(4, 0, 64, 0.2, 1.0, 1.0, 0.5, 64, 64), mr.plan(3, 0, 64, 0.2, 1.0, 1.0, 0.5, 64, 64)
    assert (a['lam'] == c['lam']).all() and (a['lam'] != b['lam']).any()
    assert (mr.plan(3, 5, 8, 0.2, 1.0, 1.0, 0.5, 64, 64)['lam'] == a['lam'][5:13]).all()


def test_undecidable_draws_are_flagged():
    lam = np.array([0.75, 0.0, 1.0, 1 - 1e-9])
    hw, und = mr._half_extent(lam, 64)                      # 0.5 * sqrt(0.25) * 64 = 16: on the boundary; lam = 0: 32, on it as well
    assert list(hw) == [16, 32, 0, 0] and list(und) == [True, True, False, False]
    hw, und = mr._half_extent(np.array([0.0, 0.5]), 53)     # 26.5 and 18.74: decidable
    assert list(hw) == [26, 18] and not und.any()


def test_apply_restatement():
    x = torch.arange(2 * 1 * 3 * 4, dtype=torch.float32).reshape(2, 1, 3, 4)
    out, _, inside = mr.apply(x, 2, 0.5, (1, 0, 3, 2), F64)
    assert inside.sum() == 4 and torch.equal(out[0, 0, :2, 1:3], x[1, 0, :2, 1:3].double()) and torch.equal(out[0, 0, 2], x[0, 0, 2].double())
    out, mag, _ = mr.apply(x, 1, 0.25, None, F64)
    assert torch.equal(out[1], 0.25 * x[1].double() + 0.75 * x[0].double()) and torch.equal(out[0], 0.25 * x[0].double() + 0.75 * x[1].double())
    assert torch.equal(mr.apply(x[:1], 1, 0.25, None, F64)[0], x[:1].double())
    assert torch.equal(mr.apply(x, 0, 1.0, None, F64)[0], x.double())
    t = mr.plan_words(2, 0.5, 0.75, 3, 4, 1, 2, 5, 6)
    assert t.tolist()[0] == 2 and t.tolist()[3:] == [3, 4, 1, 2, 5, 6] and t[1:3].view(torch.float32).tolist() == [0.5, 0.75]


def test_topk_restatement_against_torch_topk():
    gen = torch.Generator().manual_seed(3)
    z = torch.randn(50, 20, generator=gen)
    y = torch.randint(0, 20, (50,), generator=gen)
    for k in (1, 5, 20, 25):
        want = (z.topk(min(k, 20), 1)[1] == y[:, None]).any(1)
        assert torch.equal(mr.topk_hits(z, y, k), want), k


# ---------------------------------------------------------------------------------------------------------------- the C ABI
def test_version_and_new_symbols(built):
    lib = built.load()
    assert lib.fva_version() >= 12
    hdr = open(os.path.join(ROOT, 'include', 'fastvision_amd.h')).read()
    for name in NEW:
        assert f'{name}(' in hdr, name
        assert hasattr(lib, name) and name in built.PROTOTYPES, name
    assert 'fva_mix_plan_t' in hdr and C.sizeof(built.MixPlan) == 4 * mr.PLAN_WORDS
    assert [f[0] for f in built.MixPlan._fields_] == ['mode', 'lam_raw', 'lam', 'rx', 'ry', 'x1', 'y1', 'x2', 'y2']


def test_entry_points_reject_bad_arguments(built):
    lib = built.load()
    p, q = C.c_void_p(16), C.c_void_p(4096)             # never dereferenced: every case below must fail in the argument checks
    cases = [
        ('fva_mix_plan', lambda: lib.fva_mix_plan(None, 0.2, 1.0, 1.0, 0.5, 8, 8, p, None)),
        ('fva_mix_plan', lambda: lib.fva_mix_plan(p, 0.2, 1.0, 1.0, 0.5, 8, 8, None, None)),
        ('fva_mix_plan', lambda: lib.fva_mix_plan(p, 1.5, 1.0, 1.0, 0.5, 8, 8, p, None)),          # alpha > 1
        ('fva_mix_plan', lambda: lib.fva_mix_plan(p, 0.2, 2.0, 1.0, 0.5, 8, 8, p, None)),
        ('fva_mix_plan', lambda: lib.fva_mix_plan(p, -0.1, 1.0, 1.0, 0.5, 8, 8, p, None)),
        ('fva_mix_plan', lambda: lib.fva_mix_plan(p, float('nan'), 1.0, 1.0, 0.5, 8, 8, p, None)),
        ('fva_mix_plan', lambda: lib.fva_mix_plan(p, 0.2, 1.0, 1.5, 0.5, 8, 8, p, None)),
        ('fva_mix_plan', lambda: lib.fva_mix_plan(p, 0.2, 1.0, 1.0, -0.5, 8, 8, p, None)),
        ('fva_mix_plan', lambda: lib.fva_mix_plan(p, 0.2, 1.0, 1.0, 0.5, 0, 8, p, None)),
        ('fva_mix_plan', lambda: lib.fva_mix_plan(p, 0.2, 1.0, 1.0, 0.5, 65536, 65536, p, None)),
        ('fva_mix_apply', lambda: lib.fva_mix_apply(0, None, q, p, 2, 3, 8, 8, None)),
        ('fva_mix_apply', lambda: lib.fva_mix_apply(0, p, None, p, 2, 3, 8, 8, None)),
        ('fva_mix_apply', lambda: lib.fva_mix_apply(0, p, q, None, 2, 3, 8, 8, None)),
        ('fva_mix_apply', lambda: lib.fva_mix_apply(2, p, q, p, 2, 3, 8, 8, None)),
        ('fva_mix_apply', lambda: lib.fva_mix_apply(0, p, q, p, 0, 3, 8, 8, None)),
        ('fva_mix_apply', lambda: lib.fva_mix_apply(0, p, q, p, 70000, 3, 8, 8, None)),
        ('fva_mix_apply', lambda: lib.fva_mix_apply(1, p, q, p, 2, 4096, 1024, 1024, None)),
        ('fva_mix_apply', lambda: lib.fva_mix_apply(0, p, p, p, 2, 3, 8, 8, None)),                # in place
        ('fva_softmax_ce_soft', lambda: lib.fva_softmax_ce_soft(None, p, 0, None, None, 4, 10, 0, 0.1, None, p, p, p, None)),
        ('fva_softmax_ce_soft', lambda: lib.fva_softmax_ce_soft(p, None, 0, None, None, 4, 10, 0, 0.1, None, p, p, p, None)),   # neither labels nor dense
        ('fva_softmax_ce_soft', lambda: lib.fva_softmax_ce_soft(p, p, 0, None, None, 4, 10, 0, 0.1, None, None, p, p, None)),
        ('fva_softmax_ce_soft', lambda: lib.fva_softmax_ce_soft(p, p, 0, None, None, 4, 10, 0, 0.1, None, p, p, None, None)),
        ('fva_softmax_ce_soft', lambda: lib.fva_softmax_ce_soft(p, None, 0, p, None, 4, 10, 0, 0.1, p, p, p, p, None)),         # dense with a plan
        ('fva_softmax_ce_soft', lambda: lib.fva_softmax_ce_soft(p, p, 2, None, None, 4, 10, 0, 0.1, None, p, p, p, None)),
        ('fva_softmax_ce_soft', lambda: lib.fva_softmax_ce_soft(p, p, 0, None, None, 4, 10, 2, 0.1, None, p, p, p, None)),
        ('fva_softmax_ce_soft', lambda: lib.fva_softmax_ce_soft(p, p, 0, None, None, 0, 10, 0, 0.1, None, p, p, p, None)),
        ('fva_softmax_ce_soft', lambda: lib.fva_softmax_ce_soft(p, p, 0, None, None, 4, 0, 0, 0.1, None, p, p, p, None)),
        ('fva_softmax_ce_soft', lambda: lib.fva_softmax_ce_soft(p, p, 0, None, None, 4, 10, 0, 1.5, None, p, p, p, None)),
        ('fva_softmax_ce_soft', lambda: lib.fva_softmax_ce_soft(p, p, 0, None, None, 4, 10, 0, -0.1, None, p, p, p, None)),
        ('fva_softmax_ce_soft', lambda: lib.fva_softmax_ce_soft(p, p, 0, None, None, 4, 10, 0, float('nan'), None, p, p, p, None)),
        ('fva_topk_accuracy', lambda: lib.fva_topk_accuracy(None, 0, p, 0, 4, 10, 5, p, p, None)),
        ('fva_topk_accuracy', lambda: lib.fva_topk_accuracy(p, 0, None, 0, 4, 10, 5, p, p, None)),
        ('fva_topk_accuracy', lambda: lib.fva_topk_accuracy(p, 0, p, 0, 4, 10, 5, None, p, None)),
        ('fva_topk_accuracy', lambda: lib.fva_topk_accuracy(p, 0, p, 0, 4, 10, 5, p, None, None)),
        ('fva_topk_accuracy', lambda: lib.fva_topk_accuracy(p, 2, p, 0, 4, 10, 5, p, p, None)),
        ('fva_topk_accuracy', lambda: lib.fva_topk_accuracy(p, 0, p, 7, 4, 10, 5, p, p, None)),
        ('fva_topk_accuracy', lambda: lib.fva_topk_accuracy(p, 0, p, 0, 4, 10, 0, p, p, None)),      # k < 1
        ('fva_topk_accuracy', lambda: lib.fva_topk_accuracy(p, 0, p, 0, 4, 10, -3, p, p, None)),
        ('fva_topk_accuracy', lambda: lib.fva_topk_accuracy(p, 0, p, 0, 0, 10, 5, p, p, None)),
    ]
    for name, call in cases:
        assert call() == -1, name                        # FVA_ERR_ARG
        assert name in lib.fva_last_error().decode(), (name, lib.fva_last_error().decode())
    with pytest.raises(RuntimeError, match='fva_mix_plan'):
        built.call('fva_mix_plan', p, 1.5, 1.0, 1.0, 0.5, 8, 8, p, None)


# ---------------------------------------------------------------------------------------------------------------- the Python surface
def test_batchmix_construction_and_refusals():
    import fastvision_amd
    from fastvision_amd import BatchMix, MixedLabels
    torch.manual_seed(77)
    m = BatchMix()
    assert (m.mixup_alpha, m.cutmix_alpha, m.prob, m.switch_prob) == (0.2, 1.0, 1.0, 0.5)
    assert m._state.dtype == torch.int64 and m._state.tolist() == [77, 0, 0, 0]                 # seeded from torch.initial_seed(), read not drawn
    assert m._plan.dtype == torch.int32 and m._plan.numel() == mr.PLAN_WORDS
    assert set(dict(m.named_buffers())) == {'_state', '_plan'} and not m.state_dict()            # non-persistent
    assert BatchMix(seed=5)._state.tolist() == [5, 0, 0, 0]
    for bad in (dict(mixup_alpha=1.5), dict(cutmix_alpha=2.0), dict(mixup_alpha=-0.1), dict(prob=1.5), dict(switch_prob=-1)):
        with pytest.raises(ValueError):
            BatchMix(**bad)
    x, y = torch.randn(2, 3, 4, 4), torch.tensor([1, 2])
    with pytest.raises(RuntimeError):
        m.mix(x, y)                                              # no CPU path
    m.eval()
    a, b = m(x, y)
    assert a is x and b is y                                     # the identity in eval mode
    snap = m.snapshot_state()
    m._state[1] = 9
    m.restore_state(snap)
    assert m._state.tolist() == [77, 0, 0, 0]
    assert fastvision_amd.BatchMix is BatchMix and isinstance(MixedLabels(y, m._plan).lam(), torch.Tensor)


@pytest.mark.parametrize('eps', [0.0, 0.1])
def test_cross_entropy_cpu_branch_smoothing_soft_and_mixed(eps):
    from fastvision_amd import MixedLabels
    from fastvision_amd.loss import CrossEntropyLoss
    gen = torch.Generator().manual_seed(4)
    R, C_ = 5, 7
    z = torch.randn(R, C_, generator=gen)
    y = torch.randint(0, C_, (R,), generator=gen)
    w = torch.rand(R, generator=gen) + 0.5
    lam = float(np.float32(0.3))
    dense = torch.softmax(torch.randn(R, C_, generator=gen), 1)
    plan = mr.plan_words(1, lam, lam)
    forms = [(y, y), (y.view(-1, 1).float(), y), (MixedLabels(y, plan), _pair_probs(y, lam, C_).float()), (dense, dense)]
    for red in ('mean', 'sum'):
        for target, torch_target in forms:
            leaf = z.clone().requires_grad_(True)
            got = CrossEntropyLoss(red, label_smoothing=eps)(leaf, target)
            got.backward()
            ref = z.clone().requires_grad_(True)
            want = F.cross_entropy(ref, torch_target, label_smoothing=eps, reduction=red)
            want.backward()
            assert torch.allclose(got, want, rtol=1e-5, atol=1e-6) and torch.allclose(leaf.grad, ref.grad, rtol=1e-4, atol=1e-6)
    # weights keep their gradient on the CPU branch
    wl = w.clone().requires_grad_(True)
    CrossEntropyLoss('sum', label_smoothing=eps)(z, MixedLabels(y, plan), wl).backward()
    rows = F.cross_entropy(z, _pair_probs(y, lam, C_).float(), label_smoothing=eps, reduction='none')
    assert torch.allclose(wl.grad, rows, rtol=1e-5, atol=1e-6)
    with pytest.raises(ValueError):
        CrossEntropyLoss(label_smoothing=1.5)
    assert CrossEntropyLoss().label_smoothing == 0.0 and CrossEntropyLoss().reduction == 'mean'


def test_accuracy_topk_on_cpu_tensors():
    from fastvision_amd.metrics import Accuracy
    gen = torch.Generator().manual_seed(8)
    z = torch.randn(40, 30, generator=gen)
    y = torch.randint(0, 30, (40,), generator=gen)
    z[1] = 0.5                                                   # all equal: label j has j entries in front of it
    z[2, 3] = z[2, 9] = float('nan')
    y[1], y[2], y[3] = 4, 9, -1
    for k in (1, 2, 5):
        acc = Accuracy(topk=k)
        got = acc(z, y)
        want = mr.topk_hits(z, y, k).float().sum(0, keepdim=True) / 40
        assert got.shape == (1,) and torch.equal(got, want), k
        assert torch.equal(acc(z, y.float()), want)
    assert torch.equal(Accuracy()(z[4:], y[4:]), Accuracy(topk=1)(z[4:], y[4:])) and Accuracy().topk == 1
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError):
            Accuracy(topk=bad)


class _Recorder(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(4, 3)
        self.seen = []

    def forward(self, x, val=False):
        self.seen.append(x)
        return self.lin(x.flatten(1))


def test_fit_mixes_training_batches_only():
    from fastvision_amd.utils import Fit
    calls = []

    def mix(images, labels):
        calls.append((images, labels))
        return images + 1, ('mixed', labels)

    def loss(pred, labels):
        assert labels[0] == 'mixed'
        return pred.sum()

    model = _Recorder()
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    images, labels = torch.zeros(2, 1, 2, 2), torch.tensor([0, 1])
    fit = Fit(model, torch.device('cpu'), opt, None, loss, end_epoch=2, train_loader=[(images, labels)], save_last=None, mix=mix)
    fit.run_epoches()
    assert len(calls) == 2 and calls[0][0] is images and calls[0][1] is labels
    assert all(torch.equal(x, images + 1) for x in model.seen)
    plain = Fit(model, torch.device('cpu'), opt, None, lambda p, l: p.sum(), end_epoch=1, train_loader=[(images, labels)], save_last=None)
    assert plain.mix is None
    model.seen.clear()
    plain.run_epoches()
    assert model.seen[0] is images
