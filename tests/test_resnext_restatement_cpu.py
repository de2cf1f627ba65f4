"""CPU-side tests of the ResNeXt classifiers and the grouped convolution (no GPU): the float64 reference of the grouped convolution
(tests/resnext_restatement.py) pinned against F.conv2d(..., groups=) and autograd; state_dict keys, shapes and order of both factories and
the seeded default init against the fixture written from the reference (tests/golden/resnext_state_keys.json); strict loading of the
stock-torch restatement; the alias import; the new C symbols, their argument checks and fva_version() >= 10; the seed of
tests/test_gpu_resnext.py under the decision cap."""
import ctypes as C
import hashlib
import json
import os

import pytest
import torch
import torch.nn.functional as F

import resnext_restatement as xr
import streaming_measure as sm
from resnext_restatement import NAMES, StockResNeXt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = {'resnext50_32x4d': 23_000_394, 'resnext101_32x8d': 86_762_826}          # 10 classes, counted on the reference
ENTRIES = {'resnext50_32x4d': 320, 'resnext101_32x8d': 626}
NEW = ('fva_gconv_fwd', 'fva_gconv_stat_blocks', 'fva_gconv_dgrad', 'fva_gconv_wgrad', 'fva_gconv_wgrad_workspace')


@pytest.fixture(scope='module')
def golden():
    return json.load(open(os.path.join(ROOT, 'tests', 'golden', 'resnext_state_keys.json')))


@pytest.fixture(scope='module')
def built():
    import __graft_entry__ as ge
    ge.build()
    from fastvision_amd import _lib
    return _lib


def _sha1_of_parameters(m):
    h = hashlib.sha1()
    for p in m.parameters():
        h.update(p.detach().numpy().tobytes())
    return h.hexdigest()


# ------------------------------------------------------------------------------------------------ the grouped convolution's reference
@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('c_cg', [(64, 4), (64, 16), (128, 64), (64, 64)])
def test_gconv_reference_is_conv2d_with_groups_and_its_autograd(c_cg, stride):
    Cc, Cg = c_cg
    groups = Cc // Cg
    g = torch.Generator().manual_seed(Cc + Cg + stride)
    B, H, W = 2, 6, 4
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    x = torch.randn(B, H, W, Cc, generator=g, dtype=torch.float64)
    w = torch.randn(Cc, Cg, 3, 3, generator=g, dtype=torch.float64)
    dy = torch.randn(B, OH, OW, Cc, generator=g, dtype=torch.float64)
    r = xr.gconv_reference(x, w, dy, groups, stride, torch.float64)
    xn, wn = x.permute(0, 3, 1, 2).clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = F.conv2d(xn, wn, None, stride, 1, 1, groups)
    y.backward(dy.permute(0, 3, 1, 2))
    assert torch.allclose(r['y'], y.detach().permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)
    assert torch.allclose(r['dx'], xn.grad.permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)
    assert torch.allclose(r['dw'], wn.grad, rtol=1e-12, atol=1e-12)
    yd = y.detach()
    assert torch.allclose(r['s1'], yd.sum((0, 2, 3)), rtol=1e-12, atol=1e-12) and torch.allclose(r['s2'], (yd * yd).sum((0, 2, 3)), rtol=1e-12)
    # the magnitudes: the largest term of each sum, so never above the sum of the absolute terms and never zero where the element is not
    ya = F.conv2d(xn.detach().abs(), w.abs(), None, stride, 1, 1, groups).permute(0, 2, 3, 1)
    assert (r['y_mag'] <= ya + 1e-12).all() and (r['y_mag'] * 9 * Cg >= r['y'].abs() - 1e-12).all()
    assert (r['dx_mag'] * 9 * Cg >= r['dx'].abs() - 1e-12).all() and (r['dw_mag'] * B * OH * OW >= r['dw'].abs() - 1e-12).all()
    # the measure accepts an fp32 evaluation of the same formula and refuses one that leaks 2^-10 of a neighbouring element
    r32 = xr.gconv_reference(x.float(), w.float(), dy.float(), groups, stride, torch.float32)
    x32 = xr.gconv_reference(x.float(), w.float(), dy.float(), groups, stride, torch.float64)
    assert sm.check(r32['y'], x32['y'], r32['y'], x32['y_mag'], False, what='y') <= 1.0
    with pytest.raises(AssertionError):
        sm.check(r32['y'] + 2.0 ** -10 * r32['y'].roll(1, 3), x32['y'], r32['y'], x32['y_mag'], False, what='leak')


# ------------------------------------------------------------------------------------------------ the models
@pytest.mark.parametrize('name', NAMES)
def test_state_dict_keys_shapes_order_and_parameter_count(name, golden):
    """The fixture was written from the reference's classfication/models/resnext.py (it imports with torch alone), as ``ref``:

        out[name] = [[k, list(v.shape)] for k, v in getattr(ref, name)(num_classes=10).state_dict().items()]      # both factories
        torch.manual_seed(0); m = ref.resnext50_32x4d(num_classes=10); h = hashlib.sha1()
        for p in m.parameters(): h.update(p.detach().numpy().tobytes())
        out['seed0_resnext50_32x4d_sha1'] = h.hexdigest()
    """
    from fastvision_amd.classfication import models
    m = getattr(models, name)(num_classes=10)
    got = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    assert len(got) == ENTRIES[name]
    assert got == golden[name]
    assert sum(p.numel() for p in m.parameters()) == PARAMS[name]
    assert [[k, list(v.shape)] for k, v in StockResNeXt(name, num_classes=10).state_dict().items()] == golden[name]
    wide = 2 if name == 'resnext101_32x8d' else 1
    assert [getattr(m, f'res{s}')[0].conv2.weight.shape[0] for s in (2, 3, 4, 5)] == [128 * wide, 256 * wide, 512 * wide, 1024 * wide]
    assert all(getattr(m, f'res{s}')[0].conv2.groups == 32 for s in (2, 3, 4, 5))


def test_seeded_init_is_the_references(golden):
    """No initialize_weights in this file: torch's default init, in the reference's construction order."""
    from fastvision_amd.classfication import models
    torch.manual_seed(0)
    assert _sha1_of_parameters(models.resnext50_32x4d(num_classes=10)) == golden['seed0_resnext50_32x4d_sha1']
    torch.manual_seed(0)
    assert _sha1_of_parameters(StockResNeXt('resnext50_32x4d', num_classes=10)) == golden['seed0_resnext50_32x4d_sha1']


def test_loads_a_stock_checkpoint_strictly():
    from fastvision_amd.classfication import models
    torch.manual_seed(3)
    ref = StockResNeXt('resnext50_32x4d', num_classes=10)
    m = models.resnext50_32x4d(num_classes=10)
    res = m.load_state_dict(ref.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for (k, a), (_, b) in zip(m.state_dict().items(), ref.state_dict().items()):
        assert torch.equal(a, b), k


def test_alias_import_signature_and_quirks():
    import fastvision.classfication.models as alias
    import fastvision.classfication.models.resnext as alias_mod
    import fastvision_amd.classfication.models as real
    assert alias_mod is real.resnext
    for name in NAMES:
        assert getattr(alias, name) is getattr(real, name) is getattr(real.resnext, name)
    assert real.ResNet is real.resnet.ResNet and real.Bottleneck is real.resnet.Bottleneck and real.BasicBlock is real.resnet.BasicBlock
    assert real.resnext.ResNet is not real.resnet.ResNet
    m = alias.resnext50_32x4d(in_channels=3, num_classes=7, including_top=True)
    assert m.fc.out_features == 7 and m.fc.in_features == 2048 and m.planes == 2048 and m.width_per_group == 64 and m.groups == 32
    b = m.res2[0]
    assert b.down and b.downsample[0].stride == (1, 1) and b.conv2.stride == (1, 1) and b.conv2.groups == 32
    assert m.res3[0].conv2.stride == (2, 2) and m.res3[0].conv1.stride == (1, 1)
    assert not m.res3[1].down and not hasattr(m.res3[1], 'downsample')
    assert not hasattr(real.resnext101_32x8d(num_classes=5, including_top=False), 'fc')
    blk = real.resnext.Bottleneck(64, 64, groups=32, width_per_group=4)
    assert blk.conv1.out_channels == 128 and blk.conv3.out_channels == 256
    with pytest.raises(TypeError):                                   # the reference's BasicBlock takes neither groups nor width_per_group
        real.resnext.ResNet(3, 10, [1, 1, 1, 1], real.resnext.BasicBlock, 32, 4)


def test_forward_on_cpu_tensors_raises():
    from fastvision_amd.classfication.models import resnext50_32x4d
    with pytest.raises(RuntimeError, match='GPU'):
        resnext50_32x4d(num_classes=10)(torch.zeros(1, 3, 32, 32))


def test_grouped_convolutions_outside_the_contract_are_refused():
    import torch.nn as nn
    from fastvision_amd import resnet_ops
    with pytest.raises(RuntimeError, match='Cg in'):
        resnet_ops.conv_bn_relu(torch.zeros(1, 96, 4, 4), nn.Conv2d(96, 96, 3, 1, 1, groups=32, bias=False), nn.BatchNorm2d(96))        # Cg = 3
    with pytest.raises(RuntimeError, match='C % 64 == 0'):
        resnet_ops.conv_bn_relu(torch.zeros(1, 96, 4, 4), nn.Conv2d(96, 96, 3, 1, 1, groups=24, bias=False), nn.BatchNorm2d(96))        # C = 96
    with pytest.raises(RuntimeError, match='odd map in front of a stride-2 block'):
        resnet_ops.conv_bn_relu(torch.zeros(1, 128, 7, 7), nn.Conv2d(128, 128, 3, 2, 1, groups=32, bias=False), nn.BatchNorm2d(128))
    with pytest.raises(RuntimeError, match='bias-free'):
        resnet_ops.conv_bn_relu(torch.zeros(1, 128, 8, 8), nn.Conv2d(128, 128, 3, 1, 1, groups=32, bias=True), nn.BatchNorm2d(128))
    with pytest.raises(RuntimeError, match='bias-free'):
        resnet_ops.conv_bn_relu(torch.zeros(1, 128, 8, 8), nn.Conv2d(128, 128, 1, 1, 0, groups=32, bias=False), nn.BatchNorm2d(128))    # a grouped 1x1
    with pytest.raises(RuntimeError, match='bias-free'):
        resnet_ops.conv_bn_add_relu(torch.zeros(1, 128, 8, 8), nn.Conv2d(128, 128, 3, 1, 1, groups=32, bias=False), nn.BatchNorm2d(128),
                                    torch.zeros(1, 128, 8, 8))                                                                      # the tail stays dense
    with pytest.raises(RuntimeError, match='GPU'):
        resnet_ops.conv_bn_relu(torch.zeros(1, 128, 8, 8), nn.Conv2d(128, 128, 3, 1, 1, groups=32, bias=False), nn.BatchNorm2d(128))


@pytest.mark.parametrize('name', NAMES)
def test_seed_keeps_the_restatement_alone_under_the_kink_cap(name):
    """tests/test_gpu_resnext.py adopts the device's ReLU / pooling decisions where float64 is within the rounding room, at most
    KINK_SHARE_MAX of a layer.  Here, without a GPU: the fp32 restatement in the device's place stays under that cap for the test's seed."""
    import test_gpu_resnet as T
    import test_gpu_resnext as X
    ref = X._reference(name, X.SEED)
    images, _ = T._batch(2, 64, X.SEED + 2)
    _, share = X.ref64_forward(X._double(ref, name), ref, images, T.cpu_decisions(ref, images))
    print(f'\n  {name}: largest share of a layer on which fp32 and float64 part ways {share:.2e} (cap {T.KINK_SHARE_MAX:.0e})')
    assert share <= T.KINK_SHARE_MAX


# ------------------------------------------------------------------------------------------------ the C ABI
def test_new_symbols_and_version(built):
    lib = built.load()
    assert lib.fva_version() >= 10
    hdr = open(os.path.join(ROOT, 'include', 'fastvision_amd.h')).read()
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert 'fva_gconv_desc' in hdr and 'fva_gconv_desc' in doc
    for name in NEW:
        assert f'{name}(' in hdr, name
        assert hasattr(lib, name) and name in built.PROTOTYPES, name
        assert name in doc, name
    assert {'fva_gconv_stat_blocks', 'fva_gconv_wgrad_workspace'} <= built.UNCHECKED
    d = built.GConvDesc(0, 3, 10, 34, 128, 32, 1, 1, 1)
    assert lib.fva_gconv_stat_blocks(C.byref(d)) == (3 * 10 * 34 + 255) // 256
    ws = lib.fva_gconv_wgrad_workspace(C.byref(d))
    assert ws > 0 and ws % (128 * 4 * 9 * 8) == 0
    d2 = built.GConvDesc(1, 2, 8, 8, 2048, 32, 2, 1, 1)
    assert lib.fva_gconv_stat_blocks(C.byref(d2)) == 1 and lib.fva_gconv_wgrad_workspace(C.byref(d2)) > 0


def test_entry_points_reject_bad_arguments(built):
    lib = built.load()
    p, n = C.c_void_p(16), None           # p is never dereferenced: every case below must fail in the argument checks
    G = built.GConvDesc
    bad = {
        'Cg = 3': G(0, 1, 8, 8, 96, 32, 1, 1, 1),
        'C = 96': G(0, 1, 8, 8, 96, 24, 1, 1, 1),
        'Cg = 2': G(0, 1, 8, 8, 64, 32, 1, 1, 1),
        'Cg = 128': G(0, 1, 8, 8, 256, 2, 1, 1, 1),
        'C = 4096': G(0, 1, 8, 8, 4096, 64, 1, 1, 1),
        'groups does not divide C': G(0, 1, 8, 8, 128, 24, 1, 1, 1),
        'stride 3': G(0, 1, 8, 8, 128, 32, 3, 1, 1),
        'odd map at stride 2': G(0, 1, 7, 8, 128, 32, 2, 1, 1),
        'dtype': G(2, 1, 8, 8, 128, 32, 1, 1, 1),
        'in_pad 0': G(0, 1, 8, 8, 128, 32, 1, 0, 1),
        'dy_pad 0': G(0, 1, 8, 8, 128, 32, 1, 1, 0),
        'B = 0': G(0, 0, 8, 8, 128, 32, 1, 1, 1),
    }
    for what, d in bad.items():
        for name, call in (('fva_gconv_fwd', lambda: lib.fva_gconv_fwd(C.byref(d), p, p, p, n, None)),
                           ('fva_gconv_dgrad', lambda: lib.fva_gconv_dgrad(C.byref(d), p, p, p, None)),
                           ('fva_gconv_wgrad', lambda: lib.fva_gconv_wgrad(C.byref(d), p, p, p, p, 1 << 40, None))):
            assert call() == -1, (what, name)
            assert name in lib.fva_last_error().decode(), (what, name, lib.fva_last_error().decode())
        assert lib.fva_gconv_stat_blocks(C.byref(d)) == 0 and lib.fva_gconv_wgrad_workspace(C.byref(d)) == 0, what
    ok = G(0, 1, 8, 8, 128, 32, 1, 1, 1)
    for name, call in (('fva_gconv_fwd', lambda: lib.fva_gconv_fwd(C.byref(ok), n, p, p, n, None)),
                       ('fva_gconv_fwd', lambda: lib.fva_gconv_fwd(C.byref(ok), p, n, p, n, None)),
                       ('fva_gconv_dgrad', lambda: lib.fva_gconv_dgrad(C.byref(ok), p, p, n, None)),
                       ('fva_gconv_wgrad', lambda: lib.fva_gconv_wgrad(C.byref(ok), p, p, n, p, 1 << 40, None)),
                       ('fva_gconv_wgrad', lambda: lib.fva_gconv_wgrad(C.byref(ok), p, p, p, n, 1 << 40, None))):
        assert call() == -1, name
        assert name in lib.fva_last_error().decode(), name
    assert lib.fva_gconv_wgrad(C.byref(ok), p, p, p, p, 16, None) == -3 and 'fva_gconv_wgrad' in lib.fva_last_error().decode()      # short workspace
