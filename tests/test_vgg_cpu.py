"""CPU-side tests of the VGG classifiers (no GPU): state_dict keys, shapes and order of all eight factories against the fixture written from
the reference (tests/golden/vgg_state_keys.json), strict loading of a stock-torch restatement's weights, the alias import, the dropout
state's place in the module, the new C symbols and their argument checks."""
import ctypes as C
import json
import os

import pytest
import torch

from vgg_restatement import NAMES, StockVGG, dropout_keep_mask, philox4x32_10

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = dict(zip(NAMES, (22, 62, 26, 76, 32, 97, 38, 118)))
NEW = ('fva_bn_relu_apply', 'fva_bn_relu_bwd_reduce', 'fva_bn_relu_bwd_apply', 'fva_bn_bias_running_mean', 'fva_bn_eval_coeffs_bias',
       'fva_adaptive_avgpool7_fwd', 'fva_adaptive_avgpool7_bwd', 'fva_dropout_fwd', 'fva_dropout_bwd')


@pytest.fixture(scope='module')
def golden():
    return json.load(open(os.path.join(ROOT, 'tests', 'golden', 'vgg_state_keys.json')))


@pytest.fixture(scope='module')
def built():
    import __graft_entry__ as ge
    ge.build()
    from fastvision_amd import _lib
    return _lib


@pytest.mark.parametrize('name', NAMES)
def test_state_dict_keys_shapes_and_order(name, golden):
    from fastvision_amd.classfication import models
    m = getattr(models, name)(num_classes=10)
    got = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    assert len(got) == COUNTS[name]
    assert got == golden[name]                                   # names, shapes and the reference's order
    assert '_dropout_state' in dict(m.named_buffers()) and m._dropout_state.dtype == torch.int64
    assert isinstance(m.gmp, torch.nn.AdaptiveAvgPool2d) and isinstance(m.classifier[2], torch.nn.Dropout)


@pytest.mark.parametrize('name', ['vgg11', 'vgg16_bn'])
def test_loads_a_stock_checkpoint_strictly(name):
    from fastvision_amd.classfication import models
    torch.manual_seed(3)
    ref = StockVGG(name, num_classes=10)
    m = getattr(models, name)(num_classes=10)
    missing = m.load_state_dict(ref.state_dict(), strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    for (k, a), (_, b) in zip(m.state_dict().items(), ref.state_dict().items()):
        assert torch.equal(a, b), k


def test_same_seed_same_init_as_the_restatement_and_same_dropout_seed():
    from fastvision_amd.classfication.models import vgg11_bn
    torch.manual_seed(11)
    a = vgg11_bn(num_classes=10)
    torch.manual_seed(11)
    b = StockVGG('vgg11_bn', num_classes=10)
    for (k, x), (_, y) in zip(a.state_dict().items(), b.state_dict().items()):
        assert torch.equal(x, y), k
    assert a._dropout_state.tolist() == [11, 0, 0, 0]
    torch.manual_seed(12)
    assert vgg11_bn(num_classes=10)._dropout_state.tolist() == [12, 0, 0, 0]


def test_philox_restatement_gives_the_published_known_answers():
    """kat_vectors of the Random123 distribution, philox4x32 10 rounds: counter, key -> output"""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = philox4x32_10(*[[v] for v in ctr], *key)
        assert tuple(int(v[0]) for v in got) == want, (ctr, key)
    m = dropout_keep_mask(0, 0, 8, 0.5)          # seed 0, call 0: the first group is the first vector above
    assert m[:4].tolist() == [w >= 0x80000000 for w in kat[0][2]]


def test_alias_import_and_signature():
    import fastvision.classfication.models as alias
    import fastvision_amd.classfication.models as real
    for name in NAMES:
        assert getattr(alias, name) is getattr(real, name)
    m = alias.vgg16_bn(in_channels=3, num_classes=7)
    assert m.normal is True and m.in_channles == 512 and m.classifier[6].out_features == 7
    assert real.VGG(3, 5, [1, 1, 1, 1, 1], [64, 128, 256, 512, 512]).normal is False


def test_forward_on_cpu_tensors_raises():
    from fastvision_amd.classfication.models import vgg11
    with pytest.raises(RuntimeError, match='GPU'):
        vgg11(num_classes=10)(torch.zeros(1, 3, 32, 32))


def test_faster_rcnn_vgg_still_refuses_batchnorm():
    from fastvision_amd.demos.faster_rcnn.models.vgg import VGG
    with pytest.raises(NotImplementedError):
        VGG(3, 10, [1, 1, 1, 1, 1], [64, 128, 256, 512, 512], normal=True)


def test_new_symbols_and_version(built):
    lib = built.load()
    assert lib.fva_version() >= 4
    hdr = open(os.path.join(ROOT, 'include', 'fastvision_amd.h')).read()
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in NEW:
        assert f'{name}(' in hdr, name
        assert hasattr(lib, name) and name in built.PROTOTYPES, name
        assert name in doc, name


def test_entry_points_reject_bad_arguments(built):
    lib = built.load()
    p = C.c_void_p(16)                 # never dereferenced: every case below must fail in the argument checks
    cases = [
        ('fva_bn_relu_apply', lambda: lib.fva_bn_relu_apply(0, None, p, p, p, 1, 2, 8, 8, 64, None)),
        ('fva_bn_relu_apply', lambda: lib.fva_bn_relu_apply(0, p, p, p, p, 1, 2, 8, 8, 6, None)),
        ('fva_bn_relu_apply', lambda: lib.fva_bn_relu_apply(1, p, p, p, p, 1, 2, 8, 8, 24, None)),       # 3 chunks: not a power of two
        ('fva_bn_relu_apply', lambda: lib.fva_bn_relu_apply(7, p, p, p, p, 1, 2, 8, 8, 64, None)),
        ('fva_bn_relu_apply', lambda: lib.fva_bn_relu_apply(0, p, p, p, p, 2, 2, 8, 8, 64, None)),
        ('fva_bn_relu_apply', lambda: lib.fva_bn_relu_apply(0, p, p, p, p, 1, 0, 8, 8, 64, None)),
        ('fva_bn_relu_bwd_reduce', lambda: lib.fva_bn_relu_bwd_reduce(0, p, p, p, p, p, p, None, 1, 128, 64, None)),
        ('fva_bn_relu_bwd_reduce', lambda: lib.fva_bn_relu_bwd_reduce(0, p, p, p, p, p, p, p, 99, 128, 64, None)),
        ('fva_bn_relu_bwd_reduce', lambda: lib.fva_bn_relu_bwd_reduce(0, p, p, p, p, p, p, p, 1, 128, 6, None)),
        ('fva_bn_relu_bwd_apply', lambda: lib.fva_bn_relu_bwd_apply(0, p, p, p, p, p, p, None, p, 1, 2, 8, 8, 64, None)),
        ('fva_bn_relu_bwd_apply', lambda: lib.fva_bn_relu_bwd_apply(0, p, p, p, p, p, p, p, p, 1, 2, 8, 0, 64, None)),
        ('fva_bn_bias_running_mean', lambda: lib.fva_bn_bias_running_mean(64, None, p, 0.1, None)),
        ('fva_bn_bias_running_mean', lambda: lib.fva_bn_bias_running_mean(0, p, p, 0.1, None)),
        ('fva_bn_eval_coeffs_bias', lambda: lib.fva_bn_eval_coeffs_bias(64, p, p, p, p, None, 1e-5, p, p, None)),
        ('fva_adaptive_avgpool7_fwd', lambda: lib.fva_adaptive_avgpool7_fwd(0, None, 1, 2, 7, 7, 64, p, None)),
        ('fva_adaptive_avgpool7_fwd', lambda: lib.fva_adaptive_avgpool7_fwd(1, p, 1, 2, 7, 7, 12, p, None)),
        ('fva_adaptive_avgpool7_fwd', lambda: lib.fva_adaptive_avgpool7_fwd(0, p, 2, 2, 7, 7, 64, p, None)),
        ('fva_adaptive_avgpool7_fwd', lambda: lib.fva_adaptive_avgpool7_fwd(0, p, 1, 2, 0, 7, 64, p, None)),
        ('fva_adaptive_avgpool7_bwd', lambda: lib.fva_adaptive_avgpool7_bwd(0, p, 2, 7, 7, 64, None, None)),
        ('fva_adaptive_avgpool7_bwd', lambda: lib.fva_adaptive_avgpool7_bwd(3, p, 2, 7, 7, 64, p, None)),
        ('fva_dropout_fwd', lambda: lib.fva_dropout_fwd(0, p, p, 4096, 0.5, None, None)),
        ('fva_dropout_fwd', lambda: lib.fva_dropout_fwd(0, p, p, 4096, 0.0, p, None)),
        ('fva_dropout_fwd', lambda: lib.fva_dropout_fwd(0, p, p, 4096, 1.0, p, None)),
        ('fva_dropout_fwd', lambda: lib.fva_dropout_fwd(1, p, p, 4100, 0.5, p, None)),
        ('fva_dropout_bwd', lambda: lib.fva_dropout_bwd(0, p, None, p, 4096, 0.5, None)),
        ('fva_dropout_bwd', lambda: lib.fva_dropout_bwd(0, p, p, p, 0, 0.5, None)),
    ]
    for name, call in cases:
        assert call() != 0, name
        assert name in lib.fva_last_error().decode(), (name, lib.fva_last_error().decode())
