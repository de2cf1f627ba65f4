"""The second YOLOv3 demo (demos/yolov3_huaweiShip) without a GPU: the import lines of the reference's train.py:10-16 resolve through the
path entry to the new package, whose model is the yolov3_u object; the C ABI carries the new entry points and refuses bad arguments
before any pointer is dereferenced; and the fit loop keeps the reference's contract (cfg/_fit.py:6-74)."""
import ctypes as C
import os
import re
import subprocess
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHIP_IMPORTS = '''
from data_gen import create_dataset
from utils.anchor_generator import AnchorGenerator
from utils.map import mean_average_precision
from cfg._fit import Fit
from models.yolov3 import YoloV3

from utils.lossv3 import ComputeLoss
'''
NEW_SYMBOLS = ('fva_demo_ciou_loss', 'fva_demo_ciou_loss_workspace', 'fva_scale_head_groups')


def test_ship_import_lines_resolve_through_the_path_entry():
    code = SHIP_IMPORTS + '''
import fastvision_amd.demos.yolov3_huaweiShip as ship
import fastvision_amd.demos.yolov3_u as first
import fastvision_amd.demos.yolov3_huaweiShip.inference, fastvision_amd.demos.yolov3_huaweiShip.models.darknet, fastvision_amd.demos.yolov3_huaweiShip.utils.iou
import fastvision_amd.demos.yolov3_u.cfg._fit, fastvision_amd.demos.yolov3_u.inference, fastvision_amd.demos.yolov3_u.data_gen, fastvision_amd.demos.yolov3_u.utils.anchor_generator
assert ComputeLoss is ship.utils.lossv3.ComputeLoss and ComputeLoss.__module__ == 'fastvision_amd.demos.yolov3_huaweiShip.utils.lossv3'
assert Fit is ship.cfg._fit.Fit and Fit.__module__ == 'fastvision_amd.demos.yolov3_huaweiShip.cfg._fit'
assert ComputeLoss is not first.utils.lossv3.ComputeLoss and Fit is not first.cfg._fit.Fit
# everything else is the yolov3_u module object: no second copy
assert YoloV3 is first.models.yolov3.YoloV3 and ship.models.yolov3 is first.models.yolov3 and ship.models.darknet is first.models.darknet
assert create_dataset is first.data_gen.create_dataset and ship.data_gen is first.data_gen
assert ship.utils.iou is first.utils.iou and ship.utils.map is first.utils.map and ship.utils.anchor_generator is first.utils.anchor_generator
assert AnchorGenerator is first.utils.anchor_generator.AnchorGenerator and mean_average_precision is first.utils.map.mean_average_precision
import inference
assert inference.postProcess is ship.inference.postProcess and inference.postProcess is not first.inference.postProcess
import inspect
assert len(inspect.signature(inference.postProcess).parameters) == 10
a = inference.anchor_fn('cpu')
assert [t.tolist() for t in a][0] == [[462 / 64, 202 / 64], [340 / 64, 431 / 64], [522 / 64, 364 / 64]]
assert a[1].tolist()[0] == [113 / 32, 270 / 32] and a[2].tolist()[2] == [79 / 16, 134 / 16]
print('ok')
'''
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, 'demos', 'yolov3_huaweiShip'), ROOT, os.environ.get('PYTHONPATH', '')]),
               PYTHONDONTWRITEBYTECODE='1')
    r = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=300, cwd='/tmp')
    assert r.returncode == 0 and r.stdout.strip().endswith('ok'), r.stdout + r.stderr


@pytest.fixture(scope='module')
def built():
    import __graft_entry__ as ge
    ge.build()
    from fastvision_amd import _lib
    return _lib


def test_new_entry_points_are_declared_bound_and_documented(built):
    lib = built.load()
    assert lib.fva_version() >= 5
    hdr = open(os.path.join(ROOT, 'include', 'fastvision_amd.h')).read()
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in NEW_SYMBOLS:
        assert re.search(r'\b' + name + r'\s*\(', hdr), name
        assert name in built.PROTOTYPES and hasattr(lib, name), name
        assert name in doc, name
    assert re.search(r'variant 2', hdr) and 'variant 2' in doc


def _level(built, data=16, grad=None, B=2, A=3, H=4, W=4, K=6):
    lv = built.HeadLevel()
    lv.data, lv.grad = data, grad
    lv.sb, lv.sa, lv.sy, lv.sx, lv.sk = A * K * H * W, K * H * W, W, 1, H * W
    lv.B, lv.A, lv.H, lv.W, lv.K = B, A, H, W, K
    lv.stride = 1.0
    return lv


def test_argument_errors_are_reported_before_any_pointer_is_read(built):
    """Every pointer below is 16 or NULL: a call that read one would crash instead of returning."""
    lib = built.load()
    p = C.c_void_p(16)
    levels = (built.HeadLevel * 1)(_level(built))
    need = lib.fva_demo_ciou_loss_workspace(5, levels, 1)
    assert need == lib.fva_demo_loss_workspace(5, levels, 1) and need > 0
    assert lib.fva_demo_ciou_loss(p, 5, None, 1, p, p, need, None) == -1                       # null levels
    assert b'fva_demo_ciou_loss' in lib.fva_last_error()
    assert lib.fva_demo_ciou_loss(p, 0, levels, 1, p, p, need, None) == -1                     # T < 1
    assert lib.fva_demo_ciou_loss(None, 5, levels, 1, p, p, need, None) == -1
    assert lib.fva_demo_ciou_loss(p, 5, levels, 5, p, p, need, None) == -1                     # more than four levels
    rc = lib.fva_demo_ciou_loss(p, 5, levels, 1, p, p, need - 1, None)                         # a short workspace: refused, as fva_demo_loss does
    assert rc == lib.fva_demo_loss(p, 5, levels, 1, p, p, need - 1, None) and rc < 0
    assert b'workspace too small' in lib.fva_last_error()
    bad = (built.HeadLevel * 1)(_level(built, K=5))
    assert lib.fva_demo_ciou_loss(p, 5, bad, 1, p, p, need, None) == -1                        # K < 6
    # the group scale: null level, a level without a gradient buffer, null scalars, a bad shape
    lv = _level(built, grad=16)
    assert lib.fva_scale_head_groups(None, p, p, p, None) == -1
    assert lib.fva_scale_head_groups(C.byref(_level(built)), p, p, p, None) == -1
    assert lib.fva_scale_head_groups(C.byref(lv), None, p, p, None) == -1
    assert lib.fva_scale_head_groups(C.byref(lv), p, p, None, None) == -1
    assert lib.fva_scale_head_groups(C.byref(_level(built, grad=16, A=9)), p, p, p, None) == -1
    # decode: variant 3 does not exist, and the letterbox tail belongs to the two demo variants
    lb = built.Letterbox(0.5, 0.0, 0.0, 100.0, 100.0, 5.0)
    rows = 3 * 4 * 4
    assert lib.fva_yolo_decode(levels, 1, 3, None, p, rows, None) == -1
    assert b'bad variant' in lib.fva_last_error()
    assert lib.fva_yolo_decode(levels, 1, -1, None, p, rows, None) == -1
    assert lib.fva_yolo_decode(levels, 1, 0, C.byref(lb), p, rows, None) == -1
    assert b'letterbox' in lib.fva_last_error()
    assert lib.fva_yolo_decode(levels, 1, 2, C.byref(lb), p, rows + 1, None) == -1             # variant 2 is known: the next check speaks
    assert b'rows_per_image' in lib.fva_last_error()


@pytest.mark.parametrize('name', ['fva_demo_loss', 'fva_demo_ciou_loss'])
def test_a_bad_later_level_is_refused_before_anything_is_enqueued(built, name):
    """Two levels, the first valid, the second with K = 5; every pointer is 16 and the workspace is large enough.  The level check of
    level 1 has to speak before the first device call (the accumulator memset), with or without a GPU."""
    lib = built.load()
    p = C.c_void_p(16)
    levels = (built.HeadLevel * 2)(_level(built), _level(built, K=5))
    need = lib.fva_demo_loss_workspace(5, levels, 2)
    assert need > 0
    assert getattr(lib, name)(p, 5, levels, 2, p, p, need, None) == -1
    err = lib.fva_last_error().decode()
    assert 'bad level shape' in err and err.startswith(name + ':'), err


def test_ship_fit_loop_contract(tmp_path, monkeypatch):
    """warm-up ramp per iteration, min_lr on the validation loader in the no-augmentation phase, scheduler.step() only for
    warmup_epoch <= epoch < total_epoch - no_aug_epoch - 1, forward / zero_grad / three losses / backward / step, best-epoch_* and
    epoch_* checkpoints of the unwrapped model (reference _fit.py:6-74)."""
    from fastvision_amd.demos.yolov3_huaweiShip.cfg import _fit
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    events, seen_lr, loaders = [], [], []

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.tensor([1.0, 2.0]))

        def forward(self, images):
            events.append('forward')
            return (self.w * images).sum()

    class Wrapped(torch.nn.Module):                      # what nn.DataParallel looks like to the loop
        def __init__(self, m):
            super().__init__()
            self.module = m

        def forward(self, x):
            return self.module(x)

    class Opt(torch.optim.SGD):
        def zero_grad(self, *a, **k):
            events.append('zero_grad')
            return super().zero_grad(*a, **k)

        def step(self, *a, **k):
            events.append('step')
            seen_lr.append([g['lr'] for g in self.param_groups])
            return super().step(*a, **k)

    class Sched:                                         # a scheduler that visibly changes the rate
        def __init__(self):
            self.epochs = []

        def step(self):
            self.epochs.append(state['epoch'])
            for g in opt.param_groups:
                g['lr'] = 0.01 * 0.5 ** len(self.epochs)

    def criterion(predict, target, model):
        events.append('loss')
        assert isinstance(model, Wrapped)
        return predict.reshape(1) * 1.0, predict.reshape(1) * 0.5, target.sum().reshape(1) * 0 + 0.25

    class Loader(list):
        def __init__(self, name, items):
            super().__init__(items)
            self.name = name

        def __iter__(self):
            loaders.append(self.name)
            state['epoch'] = len(loaders) - 1
            return super().__iter__()

    state = {'epoch': None}
    net = Wrapped(Net())
    opt = Opt([{'params': [net.module.w]}, {'params': [torch.nn.Parameter(torch.zeros(1))], 'weight_decay': 5e-4}], lr=0.01, momentum=0.937, nesterov=True)
    batch = (torch.ones(2), torch.zeros(1, 6))
    train, val = Loader('train', [batch] * 3), Loader('val', [batch] * 3)
    args = types.SimpleNamespace(start_epoch=0, total_epoch=6, warmup_epoch=2, no_aug_epoch=1, init_lr=0.01, warmup_init_lr=0.001, min_lr=0.0001,
                                 warmup_iters=2 * 3)
    sched = Sched()
    _fit.Fit(net, args, opt, criterion, None, sched, train, val)
    # loaders: the last no_aug_epoch epochs run on the validation loader
    assert loaders == ['train'] * 5 + ['val']
    # step order, every batch
    assert events == ['forward', 'zero_grad', 'loss', 'step'] * 18
    # scheduler: epochs 2 and 3 only (warmup_epoch <= epoch < 6 - 1 - 1)
    assert sched.epochs == [2, 3]
    # learning rates, by hand from the reference's formulas
    want = []
    for epoch in range(6):
        for b in range(3):
            if epoch < 2:
                lr = (0.01 - 0.001) * (epoch * 3 + b) / float(6) + 0.001
            elif epoch >= 5:
                lr = 0.0001
            else:
                lr = 0.01 * 0.5 ** min(epoch - 2, 2)     # after the ramp's last value until the first scheduler step at the end of epoch 2
                if epoch == 2:
                    lr = (0.01 - 0.001) * 5 / float(6) + 0.001
            want.append(lr)
    assert len(seen_lr) == 18
    for got, w in zip(seen_lr, want):
        assert got == [w, w], (got, w)                   # every group
    # checkpoints: epoch_* every epoch, best-epoch_* on a better mean train loss, the reference's names, the unwrapped model's keys
    names = sorted(os.listdir(tmp_path))
    every = [n for n in names if n.startswith('epoch_')]
    best = [n for n in names if n.startswith('best-epoch_')]
    assert [n[:15] for n in every] == [f'epoch_00{e}_loss_' for e in range(1, 7)] and all(n.endswith('.pth') for n in names)
    assert len(best) >= 1 and best[0].startswith('best-epoch_001_loss_')
    losses = [float(n[len('epoch_001_loss_'):-len('.pth')]) for n in every]
    improving = [e + 1 for e, l in enumerate(losses) if l < min(losses[:e] + [float('inf')])]
    assert [int(n[len('best-epoch_'):len('best-epoch_') + 3]) for n in best] == improving
    for n in best:
        assert 'epoch_' + n[len('best-epoch_'):] in every                                  # the same loss value in both names
    assert set(torch.load(tmp_path / every[-1])) == {'w'}
    # _Train returns the mean of the summed losses, read back once per batch
    logged = []
    net2 = Wrapped(Net())
    opt2 = Opt([net2.module.w], lr=0.0)
    mean = _fit._Train(net2, [batch, batch], opt2, criterion, 3, args, log=logged.append)
    assert abs(mean - (3.0 * 1.5 + 0.25)) < 1e-6 and len(logged) == 2 and logged[0].startswith('epoch : 004 batch : 1 / 2 loss : 4.750 lr : 0.00000000')
