"""CPU-side tests of the ResNet classifiers (no GPU): the float64 restatement (tests/resnet_restatement.py) pinned against F.unfold,
F.max_pool2d, F.batch_norm and autograd; state_dict keys, shapes and order of the five factories against the fixture written from the
reference (tests/golden/resnet_state_keys.json); strict loading of the stock-torch restatement's weights; parameter counts; the alias
import; the new C symbols, their argument checks and fva_version() >= 9."""
import ctypes as C
import json
import os

import pytest
import torch
import torch.nn.functional as F

import resnet_restatement as rr
from resnet_restatement import NAMES, StockResNet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# parameters (10 classes) and state_dict entries of the five factories, counted on the reference
PARAMS = dict(zip(NAMES, (11_181_642, 21_289_802, 23_528_522, 42_520_650, 58_164_298)))
ENTRIES = dict(zip(NAMES, (122, 218, 320, 626, 932)))
NEW = ('fva_stem7_kp', 'fva_stem7_patches', 'fva_maxpool3s2_fwd', 'fva_maxpool3s2_bwd', 'fva_subsample2_fwd', 'fva_subsample2_bwd',
       'fva_bn_add_relu_apply', 'fva_bn_add_relu_bwd_blocks', 'fva_bn_add_relu_bwd_reduce', 'fva_bn_add_relu_bwd_apply')


@pytest.fixture(scope='module')
def golden():
    return json.load(open(os.path.join(ROOT, 'tests', 'golden', 'resnet_state_keys.json')))


@pytest.fixture(scope='module')
def built():
    import __graft_entry__ as ge
    ge.build()
    from fastvision_amd import _lib
    return _lib


# ------------------------------------------------------------------------------------------------ the restatement against torch
@pytest.mark.parametrize('shape', [(2, 3, 32, 32), (1, 3, 14, 18), (1, 1, 8, 8), (1, 4, 16, 16), (1, 2, 7, 9)])
def test_patch_matrix_is_unfold_and_the_gemm_is_the_convolution(shape):
    B, Cin, H, W = shape
    g = torch.Generator().manual_seed(H * W)
    x = torch.randn(shape, generator=g, dtype=torch.float64)
    for bf16 in (False, True):
        kp = rr.stem_kp(Cin, bf16)
        assert kp % (64 if bf16 else 32) == 0 and 0 <= kp - Cin * 49 < (64 if bf16 else 32)
        P = rr.patch_matrix(x, kp)
        OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        want = F.unfold(x, 7, padding=3, stride=2).transpose(1, 2).reshape(B * OH * OW, Cin * 49)          # unfold's rows: ci, kh, kw
        assert torch.equal(P[:, :Cin * 49], want) and not P[:, Cin * 49:].any()
        w = torch.randn(8, Cin, 7, 7, generator=g, dtype=torch.float64)
        wp = torch.zeros(8, kp, dtype=torch.float64)
        wp[:, :Cin * 49] = w.view(8, -1)
        y = (P @ wp.t()).view(B, OH, OW, 8).permute(0, 3, 1, 2)
        assert torch.allclose(y, F.conv2d(x, w, None, 2, 3), rtol=1e-12, atol=1e-12)
    assert rr.stem_kp(3, False) == 160 and rr.stem_kp(1, False) == 64 and rr.stem_kp(4, False) == 224
    assert rr.stem_kp(3, True) == 192 and rr.stem_kp(1, True) == 64 and rr.stem_kp(4, True) == 256


def _pool_inputs(kind, B, H, W, Cc, g):
    x = torch.randn(B, H, W, Cc, generator=g, dtype=torch.float64)
    if kind == 'negative':
        x = -x.abs() - 0.5
    elif kind == 'relu':
        x = torch.relu(x - 0.3)                                     # more than half exact zeros: ties everywhere
    elif kind == 'constant':
        x = torch.full_like(x, 1.25)
    elif kind == 'nan':
        x[0, H // 2, W // 2, 1] = float('nan')
        x[0, 0, 0, 2] = float('nan')
        x[0, min(1, H - 1), 0, 2] = float('nan')                # two NaNs in one window: the scan ends on the last
    return x


@pytest.mark.parametrize('hw', [(8, 8), (7, 5), (2, 2), (1, 1), (16, 6)])
@pytest.mark.parametrize('kind', ['random', 'negative', 'relu', 'constant', 'nan'])
def test_maxpool_restatement_is_torchs_forward_indices_and_backward(hw, kind):
    H, W = hw
    g = torch.Generator().manual_seed(H * 31 + W)
    x = _pool_inputs(kind, 2, H, W, 4, g)
    out, arg = rr.maxpool3s2(x)
    xn = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    want, idx = F.max_pool2d(xn, 3, 2, 1, return_indices=True)
    assert torch.equal(torch.nan_to_num(out.permute(0, 3, 1, 2), nan=7e77), torch.nan_to_num(want.detach(), nan=7e77))
    OH, OW = out.shape[1], out.shape[2]
    oy, ox = torch.arange(OH).view(1, OH, 1, 1), torch.arange(OW).view(1, 1, OW, 1)
    flat = (2 * oy - 1 + arg // 3) * W + (2 * ox - 1 + arg % 3)     # the restatement's choice as torch's flat index
    assert torch.equal(flat.permute(0, 3, 1, 2), idx)
    dz = torch.randn(out.shape, generator=g, dtype=torch.float64)
    want.backward(dz.permute(0, 3, 1, 2))
    got = rr.maxpool3s2_bwd(dz, x)
    got = got.permute(0, 3, 1, 2)
    assert torch.equal(got != 0, xn.grad != 0)                                           # the same pixels
    assert torch.allclose(got, xn.grad, rtol=1e-14, atol=0)                               # up to four windows add in another order
    got = got.permute(0, 2, 3, 1)
    assert torch.allclose(got.sum((1, 2)), dz.sum((1, 2)), rtol=1e-12, atol=1e-12)              # every dz lands exactly once


def test_subsample_restatement():
    x = torch.arange(2 * 4 * 6 * 3, dtype=torch.float64).view(2, 4, 6, 3)
    xs = rr.subsample2(x)
    assert torch.equal(xs, x[:, ::2, ::2]) and tuple(xs.shape) == (2, 2, 3, 3)
    xn = x.clone().requires_grad_(True)
    g = torch.randn(xs.shape, dtype=torch.float64)
    xn[:, ::2, ::2].backward(g)
    assert torch.equal(rr.subsample2_bwd(g), xn.grad)


@pytest.mark.parametrize('form2', [False, True])
def test_add_relu_restatement_is_batch_norm_and_autograd(form2):
    g = torch.Generator().manual_seed(5 + form2)
    B, H, W, Cc, eps = 3, 4, 5, 6, 1e-5
    n = B * H * W
    y = torch.randn(B, H, W, Cc, generator=g, dtype=torch.float64, requires_grad=True)
    q = torch.randn(B, H, W, Cc, generator=g, dtype=torch.float64, requires_grad=True)          # the identity, or y_d
    gamma, beta, gamma_d, beta_d = (torch.randn(Cc, generator=g, dtype=torch.float64) for _ in range(4))
    dz = torch.randn(B, H, W, Cc, generator=g, dtype=torch.float64)

    def bn(t, ga, be):
        return F.batch_norm(t.permute(0, 3, 1, 2), None, None, ga, be, True, 0.1, eps).permute(0, 2, 3, 1)

    z = torch.relu(bn(y, gamma, beta) + (bn(q, gamma_d, beta_d) if form2 else q))
    z.backward(dz)

    def stats(t, ga, be):
        t = t.detach()
        mean, var = t.mean((0, 1, 2)), t.var((0, 1, 2), unbiased=False)
        rstd = 1 / torch.sqrt(var + eps)
        return mean, rstd, ga * rstd, be - mean * ga * rstd

    mean, rstd, scale, shift = stats(y, gamma, beta)
    mean_d, rstd_d, scale_d, shift_d = stats(q, gamma_d, beta_d)
    ops = (y.detach(), scale, shift) + ((None, q.detach(), scale_d, shift_d) if form2 else (q.detach(), None, None, None))
    zz, _ = rr.add_relu_apply(*ops, torch.float64)
    assert torch.allclose(zz, z.detach(), rtol=1e-12, atol=1e-12)
    du = rr.add_relu_du(dz, *ops)
    t1, t2 = rr.add_relu_terms(du, y.detach(), mean, rstd, torch.float64)
    a, cb, cc = rr.bwd_coef(t1.sum((0, 1, 2)), t2.sum((0, 1, 2)), n, gamma, rstd)
    dy, _ = rr.add_relu_dy(du, y.detach(), mean, rstd, a, cb, cc, torch.float64)
    assert torch.allclose(dy, y.grad, rtol=1e-10, atol=1e-12)
    if form2:
        d1, d2 = rr.add_relu_terms(du, q.detach(), mean_d, rstd_d, torch.float64)
        assert torch.equal(d1, t1)                                                           # sum dU is shared by both BatchNorms
        a, cb, cc = rr.bwd_coef(d1.sum((0, 1, 2)), d2.sum((0, 1, 2)), n, gamma_d, rstd_d)
        dyd, _ = rr.add_relu_dy(du, q.detach(), mean_d, rstd_d, a, cb, cc, torch.float64)
        assert torch.allclose(dyd, q.grad, rtol=1e-10, atol=1e-12)
    else:
        assert torch.equal(du, q.grad)                                                       # dr = dU


# ------------------------------------------------------------------------------------------------ the models
@pytest.mark.parametrize('name', NAMES)
def test_state_dict_keys_shapes_order_and_parameter_count(name, golden):
    from fastvision_amd.classfication import models
    m = getattr(models, name)(num_classes=10)
    got = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    assert len(got) == ENTRIES[name]
    assert got == golden[name]                                   # names, shapes and the reference's order
    assert sum(p.numel() for p in m.parameters()) == PARAMS[name]
    assert [[k, list(v.shape)] for k, v in StockResNet(name, num_classes=10).state_dict().items()] == golden[name]
    for k in ('conv1.0.weight', 'res3.0.downsample.1.running_var', 'fc.bias'):
        assert k in m.state_dict()
    assert ('res2.0.downsample.0.weight' in m.state_dict()) == (name in ('resnet50', 'resnet101', 'resnet152'))


@pytest.mark.parametrize('name', ['resnet18', 'resnet50'])
def test_loads_a_stock_checkpoint_strictly_and_same_seed_same_init(name):
    from fastvision_amd.classfication import models
    torch.manual_seed(3)
    ref = StockResNet(name, num_classes=10)
    torch.manual_seed(3)
    same = getattr(models, name)(num_classes=10)
    for (k, a), (_, b) in zip(same.state_dict().items(), ref.state_dict().items()):
        assert torch.equal(a, b), k                              # torch.manual_seed reproduces the init
    m = getattr(models, name)(num_classes=10)
    res = m.load_state_dict(ref.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for (k, a), (_, b) in zip(m.state_dict().items(), ref.state_dict().items()):
        assert torch.equal(a, b), k


def test_alias_import_signature_and_quirks():
    import fastvision.classfication.models as alias
    import fastvision_amd.classfication.models as real
    for name in NAMES + ['ResNet', 'BasicBlock', 'Bottleneck']:
        assert getattr(alias, name) is getattr(real, name)
    m = alias.resnet50(in_channels=3, num_classes=7, including_top=True)
    assert m.fc.out_features == 7 and m.fc.in_features == 2048 and m.planes == 2048 and m.including_top is True
    b = m.res2[0]
    assert b.down and b.downsample[0].stride == (1, 1) and b.conv2.stride == (1, 1)          # a stride-1 64 -> 256 shortcut
    assert m.res3[0].conv2.stride == (2, 2) and m.res3[0].conv1.stride == (1, 1)            # Bottleneck: the stride on conv2
    assert not m.res3[1].down and not hasattr(m.res3[1], 'downsample')
    r = real.resnet18(in_channels=1, num_classes=5, including_top=False)
    assert not hasattr(r, 'fc') and r.conv1[0].in_channels == 1
    assert r.res3[0].conv1.stride == (2, 2) and r.res3[0].conv2.stride == (1, 1) and not r.res2[0].down          # BasicBlock: on conv1
    assert real.Bottleneck.expansion == 4 and real.BasicBlock.expansion == 1
    assert real.ResNet(3, 10, [1, 1, 1, 1], real.BasicBlock).fc.in_features == 512


def test_forward_on_cpu_tensors_raises():
    from fastvision_amd.classfication.models import resnet18
    with pytest.raises(RuntimeError, match='GPU'):
        resnet18(num_classes=10)(torch.zeros(1, 3, 32, 32))


def test_ops_refuse_what_is_not_on_the_path():
    import torch.nn as nn
    from fastvision_amd import resnet_ops
    x = torch.zeros(1, 64, 7, 7)
    bn = nn.BatchNorm2d(64)
    with pytest.raises(RuntimeError, match='odd map in front of a stride-2 block'):
        resnet_ops.conv_bn_relu(x, nn.Conv2d(64, 64, 3, 2, 1, bias=False), bn)
    with pytest.raises(RuntimeError, match='odd map in front of a stride-2 block'):
        resnet_ops.conv_bn_add_relu(x, nn.Conv2d(64, 64, 3, 1, 1, bias=False), bn, x, nn.Conv2d(64, 64, 1, 2, bias=False), nn.BatchNorm2d(64))
    with pytest.raises(RuntimeError, match='bias-free'):
        resnet_ops.conv_bn_relu(x, nn.Conv2d(64, 64, 3, 1, 1, bias=True), bn)
    with pytest.raises(RuntimeError, match='bias-free'):
        resnet_ops.conv_bn_relu(x, nn.Conv2d(64, 64, 1, 2, bias=False), bn)               # the strided 1x1 exists only as a shortcut
    with pytest.raises(RuntimeError, match='requires_grad'):
        resnet_ops.stem_bn_relu(torch.zeros(1, 3, 8, 8, requires_grad=True), nn.Conv2d(3, 64, 7, 2, 3, bias=False), bn)
    with pytest.raises(RuntimeError, match='7x7'):
        resnet_ops.stem_bn_relu(torch.zeros(1, 3, 8, 8), nn.Conv2d(3, 64, 3, 1, 1, bias=False), bn)
    assert 'frozen statistics' in resnet_ops.FROZEN_TAIL and 'out of scope' in resnet_ops.FROZEN_TAIL


@pytest.mark.parametrize('name', NAMES)
def test_seed_keeps_the_restatement_alone_under_the_kink_cap(name):
    """tests/test_gpu_resnet.py adopts the device's ReLU / pooling decisions where float64 is within the rounding room, at most
    KINK_SHARE_MAX of a layer.  Here, without a GPU: the fp32 restatement in the device's place stays under that cap for the test's seed,
    and every decision it takes differently from float64 lies inside the room."""
    import test_gpu_resnet as T
    ref = T._reference(name, T.SEED)
    images, _ = T._batch(2, 64, T.SEED + 2)
    _, share = T._ref64_forward(T._double(ref, name), ref, images, T.cpu_decisions(ref, images))
    print(f'\n  {name}: largest share of a layer on which fp32 and float64 part ways {share:.2e} (cap {T.KINK_SHARE_MAX:.0e})')
    assert share <= T.KINK_SHARE_MAX


# ------------------------------------------------------------------------------------------------ the C ABI
def test_new_symbols_and_version(built):
    lib = built.load()
    assert lib.fva_version() >= 9
    hdr = open(os.path.join(ROOT, 'include', 'fastvision_amd.h')).read()
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in NEW:
        assert f'{name}(' in hdr, name
        assert hasattr(lib, name) and name in built.PROTOTYPES, name
        assert name in doc, name
    assert [lib.fva_stem7_kp(0, c) for c in (1, 3, 4)] == [64, 160, 224]
    assert [lib.fva_stem7_kp(1, c) for c in (1, 3, 4)] == [64, 192, 256]
    assert lib.fva_stem7_kp(0, 0) == 0 and lib.fva_stem7_kp(5, 3) == 0
    # the backward reduce: 256 threads = (chunk columns) x (pixel rows); a block owns at least 8 steps of its pixel rows
    assert lib.fva_bn_add_relu_bwd_blocks(1, 300, 64) == 2 and lib.fva_bn_add_relu_bwd_blocks(1, 256, 64) == 1
    assert lib.fva_bn_add_relu_bwd_blocks(0, 15, 2048) == 2 and lib.fva_bn_add_relu_bwd_blocks(0, 15, 2052) == 0
    assert lib.fva_bn_add_relu_bwd_blocks(1, 0, 64) == 0


def test_entry_points_reject_bad_arguments(built):
    lib = built.load()
    p, n = C.c_void_p(16), None           # p is never dereferenced: every case below must fail in the argument checks
    cases = [
        ('fva_stem7_patches', lambda: lib.fva_stem7_patches(0, n, p, 1, 3, 8, 8, None)),
        ('fva_stem7_patches', lambda: lib.fva_stem7_patches(4, p, p, 1, 3, 8, 8, None)),
        ('fva_stem7_patches', lambda: lib.fva_stem7_patches(0, p, p, 1, 0, 8, 8, None)),
        ('fva_stem7_patches', lambda: lib.fva_stem7_patches(0, p, p, 0, 3, 8, 8, None)),
        ('fva_maxpool3s2_fwd', lambda: lib.fva_maxpool3s2_fwd(0, n, 1, p, 1, 1, 8, 8, 64, None)),
        ('fva_maxpool3s2_fwd', lambda: lib.fva_maxpool3s2_fwd(1, p, 1, p, 1, 1, 8, 8, 12, None)),
        ('fva_maxpool3s2_fwd', lambda: lib.fva_maxpool3s2_fwd(0, p, 2, p, 1, 1, 8, 8, 64, None)),
        ('fva_maxpool3s2_fwd', lambda: lib.fva_maxpool3s2_fwd(0, p, 1, p, 1, 1, 0, 8, 64, None)),
        ('fva_maxpool3s2_fwd', lambda: lib.fva_maxpool3s2_fwd(0, p, 1, p, 1, 1, 8, 8, 4096, None)),
        ('fva_maxpool3s2_bwd', lambda: lib.fva_maxpool3s2_bwd(0, p, n, 1, p, 1, 8, 8, 64, None)),
        ('fva_maxpool3s2_bwd', lambda: lib.fva_maxpool3s2_bwd(3, p, p, 1, p, 1, 8, 8, 64, None)),
        ('fva_subsample2_fwd', lambda: lib.fva_subsample2_fwd(0, p, 1, n, 1, 8, 8, 64, None)),
        ('fva_subsample2_fwd', lambda: lib.fva_subsample2_fwd(0, p, 1, p, 1, 7, 8, 64, None)),
        ('fva_subsample2_bwd', lambda: lib.fva_subsample2_bwd(0, p, p, 1, 8, 5, 64, None)),
        ('fva_subsample2_bwd', lambda: lib.fva_subsample2_bwd(1, p, p, 1, 8, 8, 4, None)),
        ('fva_bn_add_relu_apply', lambda: lib.fva_bn_add_relu_apply(0, p, p, p, n, 0, n, n, n, p, 1, 1, 4, 4, 64, None)),          # no second operand
        ('fva_bn_add_relu_apply', lambda: lib.fva_bn_add_relu_apply(0, p, p, p, p, 0, p, p, p, p, 1, 1, 4, 4, 64, None)),          # both
        ('fva_bn_add_relu_apply', lambda: lib.fva_bn_add_relu_apply(0, p, p, p, n, 0, p, n, p, p, 1, 1, 4, 4, 64, None)),          # y_d without scale_d
        ('fva_bn_add_relu_apply', lambda: lib.fva_bn_add_relu_apply(0, p, p, p, p, 0, n, n, n, p, 2, 1, 4, 4, 64, None)),
        ('fva_bn_add_relu_apply', lambda: lib.fva_bn_add_relu_apply(0, p, p, p, p, 0, n, n, n, p, 1, 1, 4, 4, 2052, None)),
        ('fva_bn_add_relu_apply', lambda: lib.fva_bn_add_relu_apply(1, p, p, p, p, 0, n, n, n, p, 1, 1, 4, 4, 36, None)),
        ('fva_bn_add_relu_bwd_reduce', lambda: lib.fva_bn_add_relu_bwd_reduce(0, p, p, p, p, p, p, p, 0, n, n, n, n, n, p, n, 99, 1, 4, 4, 64, None)),
        ('fva_bn_add_relu_bwd_reduce', lambda: lib.fva_bn_add_relu_bwd_reduce(0, p, p, p, p, p, p, p, 0, n, n, n, n, n, n, n, 1, 1, 4, 4, 64, None)),
        ('fva_bn_add_relu_bwd_reduce', lambda: lib.fva_bn_add_relu_bwd_reduce(0, p, p, p, p, p, p, n, 0, p, p, p, p, p, p, n, 1, 1, 4, 4, 64, None)),   # form 2 without partial_d
        ('fva_bn_add_relu_bwd_apply', lambda: lib.fva_bn_add_relu_bwd_apply(0, p, p, p, p, p, p, p, p, 0, n, n, n, n, n, n, p, n, 1, n, 1, 4, 4, 64, None)),   # form 1 without dr
        ('fva_bn_add_relu_bwd_apply', lambda: lib.fva_bn_add_relu_bwd_apply(0, p, p, p, p, p, p, p, n, 0, p, p, p, p, p, p, p, n, 1, n, 1, 4, 4, 64, None)),   # form 2 without dy_d
        ('fva_bn_add_relu_bwd_apply', lambda: lib.fva_bn_add_relu_bwd_apply(0, p, p, p, p, p, p, n, p, 0, n, n, n, n, n, n, p, n, 1, p, 1, 4, 4, 64, None)),   # no coef
    ]
    for name, call in cases:
        assert call() != 0, name
        assert name in lib.fva_last_error().decode(), (name, lib.fva_last_error().decode())
