"""ModelEMA without a GPU: the float64 restatement of the ramp and the update (tests/ema_restatement.py) pinned by hand-written values,
the two C entry points declared everywhere they must be and refusing bad arguments, CPU models refused, and the fit loops still
accepting the argument lists they had before ``ema=`` was added."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import ema_restatement as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def built():
    import __graft_entry__ as ge
    ge.build()
    from fastvision_amd import _lib
    return _lib


# ---------------------------------------------------------------------------------------------------------------- the restatement
def test_ramp_values_at_the_default_decay_and_tau():
    # 1 - 0.9999 * (1 - exp(-k / 2000)), worked out with 50 decimal digits
    assert abs(er.weight(1) - 0.99950017496667135) < 1e-15
    assert abs(er.weight(2) - 0.99900059978339165) < 1e-15
    assert abs(er.weight(2000) - 0.36794265322732518) < 1e-15         # 1 - 0.9999 * (1 - 1 / e)
    assert abs(er.weight(100000) - 1.0e-4) < 1e-15                    # the ramp has ended: w = 1 - decay
    assert er.weight(1, decay=0.9, tau=0.0) == 1.0 - 0.9              # tau == 0: no ramp, from the first update on
    assert er.weight(10 ** 6, decay=0.9, tau=0.0) == 1.0 - 0.9
    assert er.weight(5, decay=0.0, tau=7.0) == 1.0                    # decay 0: the average IS the model


def test_one_update_and_its_bound_by_hand():
    # e = 1, p = 3, w = 0.25: 1 + 0.25 * 2 = 1.5; bound = half an ulp of 1.5 (2^-24) + 0.25 * 2^-24 * 2
    ref = er.step(np.float32([1.0]), np.float32([3.0]), 0.25)
    assert ref.dtype == np.float64 and ref[0] == 1.5
    assert er.step_bound(ref, np.float32([1.0]), np.float32([3.0]), 0.25)[0] == 2.0 ** -24 + 2.0 ** -25
    # p == e: the result is e and the bound half an ulp of it; both zero: the bound is zero (an exact zero must come out exact)
    assert er.step(np.float32([0.75]), np.float32([0.75]), 0.3)[0] == 0.75
    assert er.step_bound(np.float64([0.75]), np.float32([0.75]), np.float32([0.75]), 0.3)[0] == 2.0 ** -25
    assert er.step_bound(np.float64([0.0]), np.float32([0.0]), np.float32([0.0]), 0.3)[0] == 0.0
    assert er.ulp32(np.float64([1.0, 1.9999, 2.0, -0.5, 2.0 ** -126, 2.0 ** -140, 0.0])).tolist() == \
        [2.0 ** -23, 2.0 ** -23, 2.0 ** -22, 2.0 ** -24, 2.0 ** -149, 2.0 ** -149, 0.0]
    assert er.w32(0.1) == float(np.float32(0.1)) and er.w32(0.1) != 0.1


def test_recurrence_follows_the_model_and_sums_its_bounds():
    e0 = np.float32([0.0, 1.0])
    ps = [np.float32([1.0, 1.0])] * 3
    got = list(er.follow(e0, ps, [0.5, 0.5, 0.5]))
    assert [r[0][0] for r in got] == [0.5, 0.75, 0.875] and [r[0][1] for r in got] == [1.0, 1.0, 1.0]
    assert got[0][1][0] == 0.5 * 2.0 ** -24 + 0.5 * 2.0 ** -24 * 1.0      # half an ulp of 0.5 + w * 2^-24 * |1 - 0|


# ---------------------------------------------------------------------------------------------------------------- the C ABI
def test_entry_points_are_declared_everywhere():
    from fastvision_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'fastvision_amd.h')).read()
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in ('fva_ema_chunk_elems', 'fva_ema_update'):
        assert re.search(r'\b' + name + r'\s*\(', hdr), name
        assert name in _lib.PROTOTYPES, name
        assert name in doc, name
    assert 'ModelEMA' in doc


def test_entry_points_report_bad_arguments(built):
    lib = built.load()
    per = lib.fva_ema_chunk_elems()
    assert per > 0 and per % 4 == 0
    p = C.c_void_p(16)
    bad = [(None, 1, p, 1, 0.9, 2000.0, p), (p, 0, p, 1, 0.9, 2000.0, p), (p, 1, None, 1, 0.9, 2000.0, p), (p, 1, p, 0, 0.9, 2000.0, p),
           (p, 1, p, 1, 0.9, 2000.0, None), (p, 1, p, 1, 1.0, 2000.0, p), (p, 1, p, 1, -0.1, 2000.0, p), (p, 1, p, 1, float('nan'), 2000.0, p),
           (p, 1, p, 1, 0.9, -1.0, p), (p, 1, p, 1, 0.9, float('nan'), p)]
    for args in bad:
        assert lib.fva_ema_update(*args, None) == -1, args
        assert b'fva_ema_update' in lib.fva_last_error()
    with pytest.raises(RuntimeError, match='decay'):
        built.call('fva_ema_update', p, 1, p, 1, 1.5, 0.0, p, None)


# ---------------------------------------------------------------------------------------------------------------- the Python surface
def test_exports():
    import fastvision
    import fastvision_amd
    from fastvision_amd.ema import ModelEMA
    assert fastvision_amd.ModelEMA is ModelEMA and fastvision_amd.utils.ModelEMA is ModelEMA
    assert fastvision.ModelEMA is ModelEMA and fastvision.utils.ModelEMA is ModelEMA


def test_cpu_models_and_bad_hyper_parameters_are_refused():
    from fastvision_amd import ModelEMA
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 1), torch.nn.BatchNorm2d(4))
    with pytest.raises(RuntimeError, match='no CPU path'):
        ModelEMA(net)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ModelEMA(torch.nn.DataParallel(net))
    for kw in (dict(decay=1.0), dict(decay=-0.1), dict(tau=-1.0), dict(updates=-1)):
        with pytest.raises(ValueError):
            ModelEMA(net, **kw)


def _names(fn):
    return list(inspect.signature(fn).parameters)


def test_fit_loops_keep_their_argument_lists():
    from fastvision_amd.demos.yolov3_u.cfg import _fit as demo
    from fastvision_amd.graphs import GraphedTrainStep
    from fastvision_amd.utils import Fit
    old = ['self', 'model', 'device', 'optimizer', 'scheduler', 'loss', 'end_epoch', 'start_epoch', 'train_loader', 'val_loader',
           'test_loader', 'data_dict', 'log_every', 'save_last']
    assert _names(Fit.__init__) == old + ['ema'] and inspect.signature(Fit.__init__).parameters['ema'].default is None
    assert _names(demo.Fit) == ['model', 'args', 'optimizer', 'criterion', 'metric', 'train_loader', 'validation_loader', 'ema']
    assert _names(demo._Train) == ['model', 'train_loader', 'optimizer', 'criterion', 'epoch', 'log', 'ema']
    assert _names(demo._Validate) == ['model', 'val_loader', 'criterion', 'epoch', 'log', 'ema']
    assert _names(demo._run_epoch) == ['model', 'loader', 'criterion', 'epoch', 'optimizer', 'log', 'ema']
    for fn in (demo.Fit, demo._Train, demo._Validate, demo._run_epoch):
        assert inspect.signature(fn).parameters['ema'].default is None
    sig = inspect.signature(GraphedTrainStep.__init__).parameters
    assert list(sig)[:11] == ['self', 'model', 'loss_fn', 'optimizer', 'images', 'targets', 'max_targets', 'warmup', 'pre_step', 'on_capture',
                              'side_stream'] and sig['ema'].default is None


def test_library_fit_without_an_ema_runs_as_before(tmp_path, monkeypatch):
    """The old positional argument list, no EMA: the checkpoint has exactly the entries it had."""
    from fastvision_amd.utils import Fit
    monkeypatch.chdir(tmp_path)

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.ones(3))

        def forward(self, x, val=False):
            return (x * self.w).sum()
    net = Net()
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    loader = [(torch.ones(3), torch.zeros(1)), (torch.full((3,), 2.0), torch.zeros(1))]
    fit = Fit(net, torch.device('cpu'), opt, None, lambda pred, labels: pred + labels.sum(), 1, 0, loader, None, None, None, 0, 'last.pth')
    assert fit.ema is None
    fit.run_epoches()
    assert set(torch.load(tmp_path / 'last.pth', weights_only=False)) == {'model', 'optimizer', 'date'}
    assert torch.allclose(net.w.detach(), torch.ones(3) - 0.1 * 3.0)


def test_demo_train_without_an_ema_runs_as_before(monkeypatch):
    from fastvision_amd.demos.yolov3_u.cfg import _fit as demo
    monkeypatch.setattr(torch.Tensor, 'cuda', lambda self, *a, **k: self)

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.ones(2))

        def forward(self, x):
            return (x * self.w).sum()
    net = Net()
    opt = torch.optim.SGD(net.parameters(), lr=0.5)
    seen = []

    def criterion(predict, target, model):
        seen.append(model)
        return predict + target.sum()
    loader = [(torch.ones(2), torch.zeros(1))]
    assert demo._Train(net, loader, opt, criterion, 0, None) == 2.0
    assert demo._Validate(net, loader, criterion, 0, None) == 1.0         # w = 1 - 0.5 * 1 = 0.5 each
    assert seen == [net, net] and not net.training


def test_demo_fit_without_an_ema_calls_its_runners_as_before(tmp_path, monkeypatch):
    """Code that replaces ``_Train`` / ``_Validate`` by functions with the old argument lists keeps working."""
    import types
    from fastvision_amd.demos.yolov3_u.cfg import _fit as demo
    monkeypatch.chdir(tmp_path)
    got = []

    def train(model, train_loader, optimizer, criterion, epoch, log=print):
        got.append('train')
        return 0.5

    def validate(model, val_loader, criterion, epoch, log=print):
        got.append('val')
        return 0.25
    monkeypatch.setattr(demo, '_Train', train)
    monkeypatch.setattr(demo, '_Validate', validate)
    net = torch.nn.Linear(2, 1)
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    demo.Fit(net, types.SimpleNamespace(start_epoch=0, max_epochs=2), opt, None, None, [], [])
    assert got == ['train', 'val'] * 2 and (tmp_path / 'epoch_1_loss_0.25.pth').exists()
