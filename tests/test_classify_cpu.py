"""CPU-side tests of the classification top (no GPU): the C ABI of the four new entry points (version, exports, argument errors
reported before anything is launched), the ``fastvision.metrics.Accuracy`` import and its CPU path against the reference's
expression, CrossEntropyLoss on CPU tensors unchanged, and the Darknet-53 state_dict keys."""
import ctypes as C
import os

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('fva_gap_fwd', 'fva_gap_bwd', 'fva_softmax_ce', 'fva_softmax_ce_workspace', 'fva_top1_accuracy')


@pytest.fixture(scope='module')
def built():
    import __graft_entry__ as ge
    ge.build()
    from fastvision_amd import _lib
    return _lib


def test_version_and_new_symbols(built):
    lib = built.load()
    assert lib.fva_version() >= 3
    hdr = open(os.path.join(ROOT, 'include', 'fastvision_amd.h')).read()
    for name in NEW:
        assert f'{name}(' in hdr, name
        assert hasattr(lib, name) and name in built.PROTOTYPES, name


def _err(lib):
    return lib.fva_last_error().decode()


def test_entry_points_reject_bad_arguments(built):
    lib = built.load()
    p = C.c_void_p(16)                 # never dereferenced: every case below must fail in the argument checks
    cases = [
        ('fva_gap_fwd', lambda: lib.fva_gap_fwd(0, None, 1, 2, 7, 7, 64, p, None)),
        ('fva_gap_fwd', lambda: lib.fva_gap_fwd(0, p, 1, 2, 7, 7, 64, None, None)),
        ('fva_gap_fwd', lambda: lib.fva_gap_fwd(5, p, 1, 2, 7, 7, 64, p, None)),
        ('fva_gap_fwd', lambda: lib.fva_gap_fwd(0, p, 2, 2, 7, 7, 64, p, None)),
        ('fva_gap_fwd', lambda: lib.fva_gap_fwd(1, p, 1, 0, 7, 7, 64, p, None)),
        ('fva_gap_fwd', lambda: lib.fva_gap_fwd(1, p, 1, 2, 7, 7, 0, p, None)),
        ('fva_gap_bwd', lambda: lib.fva_gap_bwd(0, None, 2, 7, 7, 64, p, None)),
        ('fva_gap_bwd', lambda: lib.fva_gap_bwd(0, p, 2, 7, 7, 64, None, None)),
        ('fva_gap_bwd', lambda: lib.fva_gap_bwd(0, p, 2, 0, 7, 64, p, None)),
        ('fva_gap_bwd', lambda: lib.fva_gap_bwd(3, p, 2, 7, 7, 64, p, None)),
        ('fva_softmax_ce', lambda: lib.fva_softmax_ce(None, p, 0, None, 4, 10, 0, p, p, p, None)),
        ('fva_softmax_ce', lambda: lib.fva_softmax_ce(p, None, 0, None, 4, 10, 0, p, p, p, None)),
        ('fva_softmax_ce', lambda: lib.fva_softmax_ce(p, p, 0, None, 4, 10, 0, None, p, p, None)),
        ('fva_softmax_ce', lambda: lib.fva_softmax_ce(p, p, 0, None, 4, 10, 0, p, p, None, None)),
        ('fva_softmax_ce', lambda: lib.fva_softmax_ce(p, p, 2, None, 4, 10, 0, p, p, p, None)),
        ('fva_softmax_ce', lambda: lib.fva_softmax_ce(p, p, 0, None, 4, 10, 2, p, p, p, None)),
        ('fva_softmax_ce', lambda: lib.fva_softmax_ce(p, p, 0, None, 0, 10, 0, p, p, p, None)),
        ('fva_softmax_ce', lambda: lib.fva_softmax_ce(p, p, 1, None, 4, 0, 1, p, p, p, None)),
        ('fva_top1_accuracy', lambda: lib.fva_top1_accuracy(None, 0, p, 0, 4, 10, p, p, None)),
        ('fva_top1_accuracy', lambda: lib.fva_top1_accuracy(p, 0, None, 0, 4, 10, p, p, None)),
        ('fva_top1_accuracy', lambda: lib.fva_top1_accuracy(p, 0, p, 0, 4, 10, None, p, None)),
        ('fva_top1_accuracy', lambda: lib.fva_top1_accuracy(p, 0, p, 0, 4, 10, p, None, None)),
        ('fva_top1_accuracy', lambda: lib.fva_top1_accuracy(p, 2, p, 0, 4, 10, p, p, None)),
        ('fva_top1_accuracy', lambda: lib.fva_top1_accuracy(p, 0, p, 7, 4, 10, p, p, None)),
        ('fva_top1_accuracy', lambda: lib.fva_top1_accuracy(p, 0, p, 0, 4, 0, p, p, None)),
    ]
    for name, call in cases:
        assert call() != 0, name
        assert name in _err(lib), (name, _err(lib))
    assert lib.fva_softmax_ce_workspace(0) == 0 and lib.fva_softmax_ce_workspace(4096) >= 4096 * 4
    with pytest.raises(RuntimeError, match='fva_softmax_ce'):
        built.call('fva_softmax_ce', None, p, 0, None, 4, 10, 0, p, p, p, None)


def test_accuracy_import_is_the_library_object():
    from fastvision.metrics import Accuracy
    import fastvision_amd.metrics
    assert Accuracy is fastvision_amd.metrics.Accuracy


def _ref_accuracy(y_pred, y_true):          # metrics/accuracy.py of the reference
    y_pred = torch.argmax(y_pred, dim=1)
    correct = y_pred.eq(y_true.expand_as(y_pred)).float().sum(0, keepdim=True)
    return correct / y_pred.size(0)


def test_accuracy_cpu_matches_reference_expression():
    from fastvision_amd.metrics import Accuracy
    g = torch.Generator().manual_seed(3)
    z = torch.randn(37, 11, generator=g)
    z[3] = 0.5                                             # all equal: argmax is 0
    z[4, 2] = z[4, 9] = 9.0                                # a tie: the first index wins
    y = torch.randint(0, 11, (37,), generator=g)
    y[3], y[4] = 0, 2
    acc = Accuracy()
    for lab in (y, y.float()):
        got = acc(z, lab)
        assert got.shape == (1,) and got.dtype == torch.float32
        assert torch.equal(got, _ref_accuracy(z, lab))
    with pytest.raises(RuntimeError):
        acc(z, y.view(-1, 1))                              # the reference's expand_as quirk: [N, 1] labels raise


def _ref_ce(y_pre, y_true, weights=None, reduction='mean'):     # loss/classification_loss.py:8-33 as the repository had it
    col = y_true.view(-1, 1).long()
    target = torch.zeros((col.size(0), y_pre.size(-1))).to(y_true).scatter_(1, col, 1).float()
    loss = -torch.sum(target * F.log_softmax(y_pre, dim=-1), dim=1)
    if weights is not None:
        loss = loss * weights
    return torch.mean(loss) if reduction == 'mean' else torch.sum(loss)


def test_cross_entropy_cpu_is_unchanged():
    from fastvision_amd.loss import CrossEntropyLoss
    g = torch.Generator().manual_seed(5)
    z = torch.randn(9, 13, generator=g)
    y = torch.randint(0, 13, (9, 1), generator=g)
    w = torch.rand(9, generator=g)
    for red in ('mean', 'sum'):
        for wt in (None, w):
            for lab in (y, y.view(-1), y.float()):
                assert torch.equal(CrossEntropyLoss(red)(z, lab, wt), _ref_ce(z, lab, wt, red))


def test_darknet53_state_dict_keys_unchanged():
    from fastvision_amd.classfication.models import darknet53
    from oracle.model import Backbone
    m = darknet53(num_classes=1000)
    keys = list(m.state_dict().keys())
    want = list(Backbone().state_dict().keys()) + ['fc.weight', 'fc.bias']
    assert keys == want
    assert isinstance(m.gap, torch.nn.AdaptiveAvgPool2d) and tuple(m.fc.weight.shape) == (1000, 1024)
    assert list(darknet53(num_classes=10, including_top=False).state_dict().keys()) == list(Backbone().state_dict().keys())
