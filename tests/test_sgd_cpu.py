"""FusedSGD without a GPU: the constructor checks torch.optim.SGD's arguments the way torch does and refuses what it does not
implement, the C entry points report bad arguments instead of crashing, and the Faster R-CNN fit loop leaves clipping to an
optimizer that clips by itself."""
import ctypes as C

import pytest
import torch


@pytest.fixture(scope='module')
def built():
    import __graft_entry__ as ge
    ge.build()
    from fastvision_amd import _lib
    return _lib


def _params():
    return [torch.nn.Parameter(torch.zeros(3))]


@pytest.mark.parametrize('kw', [dict(lr=-1.0), dict(lr=0.1, momentum=-0.5), dict(lr=0.1, weight_decay=-1e-4),
                                dict(lr=0.1, nesterov=True), dict(lr=0.1, momentum=0.9, dampening=0.1, nesterov=True),
                                dict(lr=torch.tensor([0.1, 0.2]))])
def test_constructor_errors_match_torch(kw):
    from fastvision_amd import FusedSGD
    with pytest.raises(ValueError) as want:
        torch.optim.SGD(_params(), **kw)
    with pytest.raises(ValueError) as got:
        FusedSGD(_params(), **kw)
    assert str(got.value) == str(want.value)


@pytest.mark.parametrize('kw', [dict(maximize=True), dict(foreach=True), dict(fused=True), dict(differentiable=True)])
def test_unsupported_torch_options_are_refused(kw):
    from fastvision_amd import FusedSGD
    with pytest.raises(ValueError, match='not supported'):
        FusedSGD(_params(), lr=0.1, **kw)
    FusedSGD(_params(), lr=0.1, **{k: (None if k in ('foreach', 'fused') else False) for k in kw})     # defaults are accepted


@pytest.mark.parametrize('kw', [dict(foreach=False), dict(fused=False), dict(maximize=None), dict(differentiable=None)])
def test_non_default_values_of_unsupported_options_are_refused(kw):
    from fastvision_amd import FusedSGD
    with pytest.raises(ValueError, match='not supported'):
        FusedSGD(_params(), lr=0.1, **kw)


@pytest.mark.parametrize('clip', [0.0, -1.0, float('inf'), float('nan')])
def test_bad_clip_norm_is_refused(clip):
    from fastvision_amd import FusedSGD
    with pytest.raises(ValueError, match='clip_norm'):
        FusedSGD(_params(), lr=0.1, clip_norm=clip)


def test_state_dict_layout_matches_torch():
    from fastvision_amd import FusedSGD
    ps = _params()
    a = FusedSGD(ps, lr=0.1, momentum=0.9, nesterov=True, clip_norm=10.).state_dict()
    b = torch.optim.SGD(ps, lr=0.1, momentum=0.9, nesterov=True).state_dict()
    assert a == b


def test_cpu_parameters_are_refused():
    from fastvision_amd import FusedSGD
    ps = _params()
    ps[0].grad = torch.ones(3)
    with pytest.raises(RuntimeError, match='GPU'):
        FusedSGD(ps, lr=0.1, momentum=0.9).step()


def test_sgd_entry_points_report_bad_arguments(built):
    lib = built.load()
    assert lib.fva_version() >= 2
    assert lib.fva_sgd_chunk_elems() > 0 and lib.fva_sgd_chunk_elems() % 4 == 0
    p = C.c_void_p(16)
    assert lib.fva_sgd_clip_coef(None, 1, p, 1, p, 10.0, p, None) == -1 and b'fva_sgd_clip_coef' in lib.fva_last_error()
    assert lib.fva_sgd_clip_coef(p, 1, p, 0, p, 10.0, p, None) == -1
    assert lib.fva_sgd_clip_coef(p, 1, p, 1, None, 10.0, p, None) == -1
    for bad in (0.0, -2.0, float('inf'), float('nan')):
        assert lib.fva_sgd_clip_coef(p, 1, p, 1, p, bad, p, None) == -1 and b'clip_norm' in lib.fva_last_error()
    assert lib.fva_sgd_step(p, 0, p, 1, p, p, 0, None, None) == -1 and b'fva_sgd_step' in lib.fva_last_error()
    assert lib.fva_sgd_step(p, 1, p, 1, None, p, 0, None, None) == -1
    assert lib.fva_sgd_step(p, 1, p, 1, p, None, 0, None, None) == -1
    with pytest.raises(RuntimeError, match='fva_sgd_step'):
        built.call('fva_sgd_step', None, 1, p, 1, p, p, 0, None, None)


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.tensor([3.0, 4.0]))

    def forward(self, images, targets):
        l = (self.w * images).sum()
        return None, l * 100, l * 0, l * 0, targets.sum() * self.w.sum() * 0


class _Stub:
    """Records the gradient it is asked to step on; clips by itself when clip_norm is set."""

    def __init__(self, net, clip_norm):
        if clip_norm is not None:
            self.clip_norm = clip_norm
        self.net, self.seen = net, []
        self.param_groups = [{'params': list(net.parameters()), 'lr': 1.0}]

    def zero_grad(self):
        for p in self.net.parameters():
            p.grad = None

    def step(self):
        self.seen.append(self.net.w.grad.clone())


def test_fit_loop_leaves_clipping_to_a_clipping_optimizer(monkeypatch):
    from fastvision_amd.demos.faster_rcnn.cfg import _fit
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    called = []
    monkeypatch.setattr(_fit, 'clip_gradient', lambda *a: called.append(a))
    net = _Net()
    opt = _Stub(net, 10.)
    _fit._Train(net, [(torch.ones(2), torch.zeros(1))], opt, log=None)
    assert called == [] and len(opt.seen) == 1
    assert torch.equal(opt.seen[0], torch.tensor([100.0, 100.0]))          # the loss gradient, unclipped


def test_fit_loop_still_clips_for_other_optimizers(monkeypatch):
    from fastvision_amd.demos.faster_rcnn.cfg import _fit
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    net = _Net()
    opt = _Stub(net, None)
    _fit._Train(net, [(torch.ones(2), torch.zeros(1))], opt, log=None)
    assert len(opt.seen) == 1
    assert torch.allclose(opt.seen[0], torch.tensor([10.0, 10.0]) / 2 ** 0.5)     # norm 100 * sqrt(2) clipped to 10
