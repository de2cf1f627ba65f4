"""Training with frozen BatchNorm statistics (the BatchNorm2d modules in eval mode, convolutions and affine parameters training): the
one-pass backward kernel element by element against float64 (tests/frozen_bn_restatement.py, measured by tests/streaming_measure.py),
the autograd nodes that use it against float64 autograd, mixed training / frozen neighbours, a whole YOLOv3 step against the CPU oracle
(fp32) and against the fp32 device step (bf16), the captured graph and the fit loop.  Every test prints its figures (pytest -s)."""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import frozen_bn_restatement as fr
import streaming_measure as sm

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
BF, FP = torch.bfloat16, torch.float32
NAN = float('nan')
BAR = 1e-3                  # the project's fp32 bar: max |got - ref| within 1e-3 of the tensor's largest magnitude


def api():
    from fastvision_amd import _lib, ops
    return _lib, ops


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def rel_err(got, ref):
    ref = ref.detach().double().cpu()
    return ((got.detach().double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


# ================================================================================================ 1. the kernel, element by element
#  B   H    W    C     regime
SHAPES = [
    (2, 5, 7, 32, 'the stem\'s channel count (4 chunks per pixel in bf16); one block walks every row'),
    (2, 13, 9, 256, '3 blocks, odd sizes'),
    (2, 3, 5, 1024, 'a row shorter than one block step in bf16 (896 of 2 x 256 x 2 chunks); cpp = 256 in fp32'),
    (2, 24, 40, 64, '122 880 elements: the rounding-bias shape; 30 blocks'),
    (2, 520, 64, 8, '1044 padded rows > 1024 blocks (66 560 pixels / 64 = 1040): the table is full, blocks 0..19 walk two rows; two-level table fold'),
]


@functools.lru_cache(maxsize=None)
def kernel_reference(shape, dt, act):
    """Operands and the float64 / fp32 restatement of one launch: computed once, shared by the dy_pad variants, never modified."""
    B, H, W, Cc = shape
    y, dz, scale, shift, m, r = fr.make_inputs(B, H, W, Cc, dt, 1000 + Cc + W)
    u64, du64, t64, dy64 = fr.terms(dz, y, scale, shift, m, r, act, torch.float64)
    _, du32, t32, dy32 = fr.terms(dz, y, scale, shift, m, r, act, torch.float32)
    kink = fr.kink_mask(y, scale, shift) if act == 'relu' else torch.zeros_like(u64, dtype=torch.bool)
    return dict(y=y, dz=dz, scale=scale, shift=shift, m=m, r=r, du64=du64, t64=t64, dy64=dy64, du32=du32, t32=t32, dy32=dy32, kink=kink)


def launch(act, dt, ref, shape, pad, sums):
    """One launch into NaN-filled outputs.  Returns (dy on the host, partial table rows on the host or None, nblocks, device table)."""
    _lib, ops = api()
    lib = _lib.load()
    B, H, W, Cc = shape
    code = ops._code(dt)
    d = {k: ref[k].to(DEV) for k in ('y', 'dz', 'scale', 'shift', 'm', 'r')}
    dy = torch.full((B, H + 2 * pad, W + 2 * pad, Cc), NAN, dtype=dt, device=DEV)
    nb = lib.fva_bn_frozen_bwd_blocks(code, B, H, W, Cc, pad)
    assert nb > 0
    part = torch.full((lib.fva_bn_partial_rows(nb), 2, Cc), NAN, dtype=FP, device=DEV) if sums else None
    _lib.call(f'fva_bn_{act}_frozen_bwd', code, ops._p(d['dz']), ops._p(d['y']), ops._p(d['scale']), ops._p(d['shift']),
              ops._p(d['m']) if sums else None, ops._p(d['r']) if sums else None, ops._p(part), ops._p(dy), pad, B, H, W, Cc, ops._stream())
    torch.cuda.synchronize()
    return dy.cpu(), (part[:nb].cpu() if sums else None), nb, part


def interior(buf, pad, what):
    assert not torch.isnan(buf).any(), f'{what}: NaN left in the output'
    if pad == 0:
        return buf
    Hp, Wp = buf.shape[1], buf.shape[2]
    border = torch.ones(Hp, Wp, dtype=torch.bool)
    border[pad:Hp - pad, pad:Wp - pad] = False
    assert not bits(buf)[:, border].any(), f'{what}: the border is not +0'
    return buf[:, pad:Hp - pad, pad:Wp - pad]


@pytest.mark.parametrize('pad', [0, 1])
@pytest.mark.parametrize('act', ['silu', 'relu'])
@pytest.mark.parametrize('dt', [BF, FP], ids=['bf16', 'f32'])
@pytest.mark.parametrize('shape', [s[:4] for s in SHAPES], ids=['x'.join(map(str, s[:4])) for s in SHAPES])
def test_frozen_bwd_kernel_element_by_element(shape, dt, act, pad):
    _lib, ops = api()
    B, H, W, Cc = shape
    ref = kernel_reference(shape, dt, act)
    what = f'fva_bn_{act}_frozen_bwd {"bf16" if dt == BF else "f32"} {shape} pad {pad}'
    dy_a, part_a, nb, _ = launch(act, dt, ref, shape, pad, True)
    dy_b, part_b, _, table = launch(act, dt, ref, shape, pad, True)
    dy_c, _, _, _ = launch(act, dt, ref, shape, pad, False)
    assert torch.equal(bits(dy_a), bits(dy_b)) and torch.equal(bits(part_a), bits(part_b)), f'{what}: two runs differ'
    assert torch.equal(bits(dy_a), bits(dy_c)), f'{what}: dY differs between SUMS on and off'

    # ---- dY
    got = interior(dy_a, pad, what)
    kink = ref['kink']
    share = kink.double().mean().item()
    assert share <= fr.KINK_SHARE_MAX, f'{what}: {share:.2e} of the elements sit on the ReLU kink'
    keep = ~kink
    bf = dt == BF
    w_dy = sm.check(got[keep], ref['dy64'][keep], ref['dy32'][keep], ref['dy64'][keep].abs(), bf, bias=bf and shape == (2, 24, 40, 64),
                    factor=sm.FACTOR_SIGMOID if act == 'silu' else sm.FACTOR, what=what)

    # ---- the partial table, added up on the host in float64
    assert not torch.isnan(part_a).any(), f'{what}: a row of the partial table was not written'
    epc = 8 if bf else 4
    n = fr.chain_length(nb, B, H, W, Cc, pad, epc)
    worst = []
    per_channel = lambda t: t.reshape(-1, Cc).sum(0)
    sums64, lims = [], []
    for k, (t64, t32) in enumerate(((ref['du64'], ref['du32']), (ref['t64'], ref['t32']))):
        want = per_channel(t64)
        lim = sm.sum_limit(n, per_channel(t64.abs()), per_channel((t32.double() - t64).abs()))
        # an element on the kink may honestly be masked either way: its term may be there or not
        other = ref['dz'].double() * (1.0 if k == 0 else (ref['y'].double() - ref['m'].double()) * ref['r'].double())
        lim = lim + per_channel(torch.where(kink, other.abs(), torch.zeros_like(other)))
        err = (part_a[:, k].double().sum(0) - want).abs()
        worst.append((err / lim.clamp_min(1e-300)).max().item())
        sums64.append(want)
        lims.append(lim)
    assert max(worst) <= 1.0, f'{what}: partial sums, worst err / limit {worst}'

    # ---- the table fold: dbeta = s1, dgamma = s2, dbias = scale * s1
    out = torch.full((3, Cc), NAN, dtype=FP, device=DEV)
    scale_d = ref['scale'].to(DEV)
    _lib.call('fva_bn_frozen_bwd_finalize', ops._p(table), nb, table.shape[0], Cc, ops._p(scale_d), ops._p(out[0]), ops._p(out[1]), ops._p(out[2]),
              ops._stream())
    dgamma, dbeta, dbias = out.cpu().double()
    grow = (n + fr.finalize_chain(nb) + 2) / (n + 2)              # the longer chain, applied to the whole limit
    sc = ref['scale'].double()
    w_fin = max(((dbeta - sums64[0]).abs() / (grow * lims[0]).clamp_min(1e-300)).max().item(),
                ((dgamma - sums64[1]).abs() / (grow * lims[1]).clamp_min(1e-300)).max().item(),
                ((dbias - sc * sums64[0]).abs() / (sc.abs() * grow * lims[0] + sm.EPS32 * (sc * sums64[0]).abs()).clamp_min(1e-300)).max().item())
    assert w_fin <= 1.0, f'{what}: dgamma / dbeta / dbias, worst err / limit {w_fin:.3f}'
    print(f'\n  {what}: {nb} blocks, chain {n}; worst err / limit dY {w_dy:.3f}, sums {max(worst):.3f}, folded {w_fin:.3f}; kink share {share:.1e}')


# ================================================================================================ 2. the autograd nodes, fp32, against float64 autograd
def _randomize_bn(bn, g):
    """Non-trivial running statistics and affine parameters (gamma of both signs)."""
    Cc = bn.num_features
    with torch.no_grad():
        bn.running_mean.copy_(0.3 * torch.randn(Cc, generator=g))
        bn.running_var.copy_(0.5 + 1.5 * torch.rand(Cc, generator=g))
        bn.weight.copy_((0.5 + torch.rand(Cc, generator=g)) * torch.where(torch.rand(Cc, generator=g) < 0.2, -1.0, 1.0))
        bn.bias.copy_(0.5 * torch.randn(Cc, generator=g))


def _bn64(y, bn, training=False):
    """float64 BatchNorm of the module's parameters; training=True works on clones of the running statistics."""
    rm, rv = bn.running_mean.detach().double().cpu().clone(), bn.running_var.detach().double().cpu().clone()
    return F.batch_norm(y, rm, rv, bn.weight64, bn.bias64, training=training, momentum=bn.momentum, eps=bn.eps)


def _leaf64(mod):
    """float64 leaf copies of a module's parameters, hung on the module: ``p64`` names -> tensors."""
    for m in mod.modules():
        for k, p in list(m._parameters.items()):
            if p is not None:
                setattr(m, k + '64', p.detach().double().cpu().requires_grad_())


def _conv_block64(x, cb, training=False):
    c = cb.conv
    return F.silu(_bn64(F.conv2d(x, c.weight64, None, c.stride, c.padding), cb.bn, training))


def _bn_state(mod):
    return {k: v.detach().clone() for k, v in mod.state_dict().items() if 'running' in k or 'num_batches' in k}


def _assert_state_unchanged(mod, before, what):
    for k, v in before.items():
        assert torch.equal(mod.state_dict()[k], v), f'{what}: {k} changed'


def _make(kind, g):
    from fastvision_amd.classfication.models.darknet53 import ConvBlock1x1, ConvBlock3x3, ResidualBlock
    torch.manual_seed(5)
    if kind == '3x3s1':
        mod, cin = ConvBlock3x3(64, 64), 64
    elif kind == '3x3s2':
        mod, cin = ConvBlock3x3(64, 128, stride=(2, 2)), 64
    elif kind == '1x1':
        mod, cin = ConvBlock1x1(64, 32), 64
    elif kind == 'residual':
        mod, cin = ResidualBlock(64, 32), 64
    elif kind == 'stem':
        mod, cin = ConvBlock3x3(3, 32), 3
    else:
        raise ValueError(kind)
    for m in mod.modules():
        if isinstance(m, nn.BatchNorm2d):
            _randomize_bn(m, g)
    return mod.to(DEV), cin


def _ref64(kind, mod, x64):
    if kind == 'residual':
        return x64 + _conv_block64(_conv_block64(x64, mod.conv1), mod.conv2)
    return _conv_block64(x64, mod)


def _device_grads(mod, x, dz, input_grad):
    import fastvision_amd
    for p in mod.parameters():
        p.grad = None
    xd = x.to(DEV).requires_grad_(input_grad)
    with fastvision_amd.compute_dtype(FP):
        out = mod(xd)
        out.backward(dz.to(DEV))
    torch.cuda.synchronize()
    return out.detach(), (xd.grad.detach().clone() if input_grad else None), {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in mod.named_parameters()}


@pytest.mark.parametrize('kind', ['3x3s1', '3x3s2', '1x1', 'residual', 'stem'])
def test_frozen_silu_blocks_fp32_vs_float64_autograd(kind):
    g = torch.Generator().manual_seed(3)
    mod, cin = _make(kind, g)
    mod.train()
    for m in mod.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.eval()                                 # frozen statistics without the helper: a plain bn.eval()
    x = torch.randn(2, cin, 12, 10, generator=g) if kind != 'stem' else torch.rand(2, 3, 12, 10, generator=g)
    input_grad = kind != 'stem'                      # the stem refuses a gradient for the images
    _leaf64(mod)
    x64 = x.double().requires_grad_(input_grad)
    want = _ref64(kind, mod, x64)
    dz = torch.randn(want.shape, generator=g)
    want.backward(dz.double())

    before = _bn_state(mod)
    out, dx, grads = _device_grads(mod, x, dz, input_grad)
    _assert_state_unchanged(mod, before, kind)
    figs = {'out': rel_err(out, want)}
    if input_grad:
        figs['dx'] = rel_err(dx, x64.grad)
    for name, p in mod.named_parameters():
        owner = mod.get_submodule(name.rsplit('.', 1)[0]) if '.' in name else mod
        figs[name] = rel_err(grads[name], getattr(owner, name.rsplit('.', 1)[-1] + '64').grad)
    print(f'\n  frozen {kind} fp32 vs float64: ' + ', '.join(f'{k} {v:.1e}' for k, v in figs.items()))
    assert max(figs.values()) < BAR, max(figs, key=figs.get)

    # only what autograd asks for: gamma / beta frozen too -> their gradients stay None, dx and dW keep their bits
    bns = [m for m in mod.modules() if isinstance(m, nn.BatchNorm2d)]
    for bn in bns:
        bn.weight.requires_grad_(False); bn.bias.requires_grad_(False)
    _, dx2, grads2 = _device_grads(mod, x, dz, input_grad)
    for name in grads:
        if '.bn.' in name or name.startswith('bn.'):
            assert grads2[name] is None, name
        else:
            assert torch.equal(grads2[name], grads[name]), name
    assert not input_grad or torch.equal(dx2, dx)
    for bn in bns:
        bn.weight.requires_grad_(True); bn.bias.requires_grad_(True)
    # a weight that asks for no gradient: no weight-gradient launch, dx keeps its bits
    if input_grad:
        convs = [m for m in mod.modules() if isinstance(m, nn.Conv2d)]
        for c in convs:
            c.weight.requires_grad_(False)
        _, dx3, grads3 = _device_grads(mod, x, dz, True)
        assert torch.equal(dx3, dx)
        for name in grads:
            if name.endswith('conv.weight'):
                assert grads3[name] is None, name
            else:
                assert torch.equal(grads3[name], grads[name]), name
    _assert_state_unchanged(mod, before, kind)


def test_frozen_relu_block_with_bias_fp32_vs_float64_autograd():
    """Conv2d(bias) -> BatchNorm2d -> ReLU of the VGG classifiers with frozen statistics: the bias no longer cancels, its gradient is real.
    ReLU is discontinuous in its gradient, so the reference takes the device's side on exactly the decisions that an fp32 evaluation
    cannot make, |u64| <= 2 (9 Cin + 4) 2^-24 (sum |w||x| + |b|) |scale_bn|; any other disagreement is an error, and such
    elements are at most 0.1 % of the layer."""
    import fastvision_amd
    from fastvision_amd import vgg_ops
    g = torch.Generator().manual_seed(9)
    torch.manual_seed(6)
    conv, bn = nn.Conv2d(64, 64, 3, 1, 1, bias=True).to(DEV), nn.BatchNorm2d(64)
    _randomize_bn(bn, g)
    bn = bn.to(DEV).eval()
    with torch.no_grad():
        conv.bias.copy_(torch.randn(64, generator=g))
    x = torch.randn(2, 64, 12, 10, generator=g)
    dz = torch.randn(2, 64, 12, 10, generator=g)
    before = _bn_state(bn)

    def device(input_grad=True):
        for p in (*conv.parameters(), *bn.parameters()):
            p.grad = None
        xd = x.to(DEV).requires_grad_(input_grad)
        with fastvision_amd.compute_dtype(FP):
            z = vgg_ops.conv_bn_relu(xd, conv, bn)
            z.backward(dz.to(DEV))
        torch.cuda.synchronize()
        return z.detach(), xd.grad, {'weight': conv.weight.grad, 'bias': conv.bias.grad, 'gamma': bn.weight.grad, 'beta': bn.bias.grad}
    z, dx, grads = device()
    _assert_state_unchanged(bn, before, 'conv_bn_relu')

    p64 = {k: v.detach().double().cpu().requires_grad_() for k, v in (('weight', conv.weight), ('bias', conv.bias), ('gamma', bn.weight), ('beta', bn.bias))}
    rm, rv = bn.running_mean.double().cpu(), bn.running_var.double().cpu()
    x64 = x.double().requires_grad_()
    u = F.batch_norm(F.conv2d(x64, p64['weight'], p64['bias'], 1, 1), rm.clone(), rv.clone(), p64['gamma'], p64['beta'], training=False, eps=bn.eps)
    with torch.no_grad():
        mag = F.conv2d(x64.abs(), p64['weight'].abs(), p64['bias'].abs(), 1, 1)
        lim = 2 * (9 * 64 + 4) * sm.EPS32 * mag * (p64['gamma'] / (rv + bn.eps).sqrt()).abs()[None, :, None, None]
        own, dev = u > 0, (z > 0).cpu()
        mism = own != dev
        assert (u.abs()[mism] <= lim[mism]).all(), 'the device masks an element that is not on the kink'
        share = mism.double().mean().item()
        assert share <= fr.KINK_SHARE_MAX, share
        keep = torch.where(mism, dev, own).double()
    want = u * keep
    want.backward(dz.double())
    figs = {'out': rel_err(z, want), 'dx': rel_err(dx, x64.grad)}
    figs.update({k: rel_err(grads[k], p64[k].grad) for k in grads})
    print(f'\n  frozen conv_bn_relu fp32 vs float64: ' + ', '.join(f'{k} {v:.1e}' for k, v in figs.items()) + f'; decisions taken from the device {share:.1e}')
    assert max(figs.values()) < BAR, max(figs, key=figs.get)
    assert p64['bias'].grad.abs().max() > 1e-2 and grads['bias'].abs().max() > 1e-2       # not the zeros of training mode

    keep_bits = {k: v.clone() for k, v in grads.items()}
    for p in (conv.bias, bn.weight, bn.bias):
        p.requires_grad_(False)
    _, dx2, grads2 = device()
    assert grads2['bias'] is None and grads2['gamma'] is None and grads2['beta'] is None
    assert torch.equal(dx2, dx) and torch.equal(grads2['weight'], keep_bits['weight'])
    conv.weight.requires_grad_(False)
    _, dx3, grads3 = device()
    assert grads3['weight'] is None and torch.equal(dx3, dx)
    _assert_state_unchanged(bn, before, 'conv_bn_relu')


# ================================================================================================ 3. mixed modes
@pytest.mark.parametrize('frozen_first', [False, True], ids=['train-then-frozen', 'frozen-then-train'])
def test_training_and_frozen_neighbours(frozen_first):
    """A training-mode block feeding a frozen one and the reverse, with the dgrad-epilogue fusion on (the default): the frozen block's dgrad
    sums the training-mode producer's BatchNorm-backward statistics; a frozen producer is simply not fused."""
    from fastvision_amd import ops
    from fastvision_amd.classfication.models.darknet53 import ConvBlock3x3
    assert ops._BN_FUSE[0]
    g = torch.Generator().manual_seed(21)
    torch.manual_seed(8)
    a, b = ConvBlock3x3(64, 64), ConvBlock3x3(64, 64)
    for cb in (a, b):
        _randomize_bn(cb.bn, g)
    mod = nn.Sequential(a, b).to(DEV).train()
    (a if frozen_first else b).bn.eval()
    frozen, live = (a, b) if frozen_first else (b, a)
    x = torch.randn(2, 64, 12, 10, generator=g)
    _leaf64(mod)
    x64 = x.double().requires_grad_()
    want = _conv_block64(_conv_block64(x64, a, training=not frozen_first), b, training=frozen_first)
    dz = torch.randn(want.shape, generator=g)
    want.backward(dz.double())
    before = _bn_state(frozen)
    out, dx, grads = _device_grads(mod, x, dz, True)
    _assert_state_unchanged(frozen, before, 'the frozen block')
    assert live.bn.num_batches_tracked.item() == 1
    figs = {'out': rel_err(out, want), 'dx': rel_err(dx, x64.grad)}
    for i, cb in enumerate((a, b)):
        figs[f'{i}.conv.weight'] = rel_err(grads[f'{i}.conv.weight'], cb.conv.weight64.grad)
        figs[f'{i}.bn.weight'] = rel_err(grads[f'{i}.bn.weight'], cb.bn.weight64.grad)
        figs[f'{i}.bn.bias'] = rel_err(grads[f'{i}.bn.bias'], cb.bn.bias64.grad)
    print(f'\n  {"frozen -> training" if frozen_first else "training -> frozen"} fp32 vs float64: ' + ', '.join(f'{k} {v:.1e}' for k, v in figs.items()))
    assert max(figs.values()) < BAR, max(figs, key=figs.get)


# ================================================================================================ 4. / 5. the whole YOLOv3 step
def lib_model(seed=20220504):
    from fastvision_amd.classfication.models import darknet53
    from fastvision_amd.detection.head import yolov3head
    from fastvision_amd.detection.models import yolov3
    from fastvision_amd.detection.neck import yolov3neck
    from fastvision_amd.synthetic import coco_anchors_px
    torch.manual_seed(seed)
    m = yolov3(backbone=darknet53, neck=yolov3neck, head=yolov3head, anchors=coco_anchors_px(), num_anchors_per_level=[3, 3, 3],
               in_channels=3, num_classes=80, training=True)
    return m.to(DEV).train()


CALIB_IMAGES = 16


def healthy_statistics(net, images):
    """Give every BatchNorm the statistics of one batch: a no_grad training-mode forward at momentum 1.0, the momentum put back."""
    import fastvision_amd
    bns = [m for m in net.modules() if isinstance(m, nn.BatchNorm2d)]
    old = [m.momentum for m in bns]
    for m in bns:
        m.momentum = 1.0
    net.train()
    with torch.no_grad(), fastvision_amd.compute_dtype(FP):
        net(images.to(DEV))
    for m, mom in zip(bns, old):
        m.momentum = mom
    torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def calibrated_state():
    """The state_dict (on the host) of the seeded model after healthy_statistics: shared by the tests below, never modified.
    The one calibration forward sees CALIB_IMAGES = 16 images, not the two of the step: at 64 px the deepest maps are 2 x 2, so two images
    leave 8 values per channel, whose variance estimate scatters by sqrt(2 / 7) = 53 % -- measured: smallest running_var 2.6e-3, a frozen
    scale of gamma / 0.05 that amplifies every rounding below it -- where 16 images give 64 values and 18 % (smallest running_var 1.9e-2).
    Statistics of 8 values are not what a pretrained network carries."""
    from fastvision_amd.synthetic import synthetic_batch
    net = lib_model()
    healthy_statistics(net, synthetic_batch(CALIB_IMAGES, 64, seed=5)[0])
    return {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}


def frozen_model(backbone_only):
    """The calibrated model in train mode with every BatchNorm (or only the backbone's, through the helper) frozen."""
    from fastvision_amd.utils import freeze_batchnorm
    net = lib_model()
    net.load_state_dict(calibrated_state())
    if backbone_only:
        freeze_batchnorm(net.backbone)
        net.train()
    else:
        net.train()
        for m in net.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.eval()
    return net


def device_step(net, dtype, images, tg):
    import fastvision_amd
    from fastvision_amd.loss import Yolov3Loss
    for p in net.parameters():
        p.grad = None
    with fastvision_amd.compute_dtype(dtype):
        crit = Yolov3Loss(net, 0.5, 0.05, 1.0, 0.5)
        pred = net(images.to(DEV))
        loss = crit(pred, tg.to(DEV))
        loss.backward()
    torch.cuda.synchronize()
    return [p.detach().float().cpu() for p in pred], loss.item(), {k: p.grad.detach().float().cpu() for k, p in net.named_parameters()}


@pytest.mark.parametrize('backbone_only', [False, True], ids=['all-frozen', 'backbone-frozen'])
def test_frozen_yolov3_step_fp32_vs_oracle(backbone_only):
    from fastvision_amd.synthetic import synthetic_batch
    from oracle import train as otrain
    images, tg = synthetic_batch(2, 64)
    net = frozen_model(backbone_only)
    ref, ref_crit = otrain.make_library(20220504)
    ref.load_state_dict(calibrated_state())
    ref.train()
    for m in (ref.backbone if backbone_only else ref).modules():
        if isinstance(m, nn.BatchNorm2d):
            m.eval()
    n_frozen = sum(isinstance(m, nn.BatchNorm2d) and not m.training for m in net.modules())
    assert n_frozen == sum(isinstance(m, nn.BatchNorm2d) and not m.training for m in ref.modules()) and n_frozen >= 52
    frozen_before = {k: v.clone() for k, v in net.state_dict().items()
                     if ('running' in k or 'num_batches' in k) and (not backbone_only or k.startswith('backbone.'))}
    rpred = ref(images)
    rloss = ref_crit(rpred, tg)
    rloss.backward()
    heads, loss, grads = device_step(net, FP, images, tg)
    for k, v in frozen_before.items():
        assert torch.equal(net.state_dict()[k], v), k
    herr = [rel_err(h, r) for h, r in zip(heads, rpred)]
    lrel = abs(loss - rloss.item()) / abs(rloss.item())
    gref = dict(ref.named_parameters())
    assert list(grads) == list(gref)
    gerr = {k: rel_err(grads[k], gref[k].grad) for k in grads}
    worst = max(gerr, key=gerr.get)
    print(f'\n  frozen YOLOv3 step fp32 ({"backbone" if backbone_only else "all"}, {n_frozen} BatchNorms frozen): heads {herr}, loss {loss:.6f} vs oracle '
          f'{rloss.item():.6f} (rel {lrel:.1e}), gradients: median {np.median(list(gerr.values())):.1e}, worst {gerr[worst]:.1e} ({worst})')
    assert max(herr) < BAR and lrel < BAR
    assert gerr[worst] < BAR, worst


def test_frozen_yolov3_step_bf16_vs_fp32():
    """bf16 against the fp32 device step, at the bf16 bars of tests/test_gpu_fullsize.py: heads 1.3e-1 of the scale, loss 1e-3, per-tensor
    gradient norms 1.2e-1 (all parameters), cosine 0.96 (that test's sampled tensors; the minimum over all tensors is printed beside it).
    Measured on an MI355X (all 72 BatchNorms frozen, 2 x 3 x 64^2): heads 0.057 / 0.049 / 0.052, loss 5.4e-4, gradient norms median 3.5e-3,
    worst 4.2e-2 (backbone.conv0.bn.weight), cosine 0.9936 sampled / 0.9911 over all tensors.  The bars depend on the statistics being
    healthy (calibrated_state): with statistics of the step's own two images -- 8 values per channel at the deepest level -- the same
    step read heads 0.214, loss 4.9e-3, norms 1.78e-1, cosine 0.912, and the TRAINING-mode step of that size, which normalises with exactly
    such statistics, heads 0.234, loss 1.2e-3, norms 1.66e-1, cosine 0.801."""
    from fastvision_amd.synthetic import synthetic_batch
    from test_gpu_fullsize import GRAD_SAMPLE
    images, tg = synthetic_batch(2, 64)
    net = frozen_model(False)
    h32, l32, g32 = device_step(net, FP, images, tg)
    h16, l16, g16 = device_step(net, BF, images, tg)
    herr = [rel_err(a, b) for a, b in zip(h16, h32)]
    lrel = abs(l16 - l32) / abs(l32)
    nrm = {k: abs(g16[k].double().norm().item() - g32[k].double().norm().item()) / max(g32[k].double().norm().item(), 1e-12) for k in g32}
    cos = {k: (g16[k].double().flatten() @ g32[k].double().flatten() / (g16[k].double().norm() * g32[k].double().norm()).clamp_min(1e-300)).item() for k in g32}
    wn, wa = max(nrm, key=nrm.get), min(cos, key=cos.get)
    wc = min(GRAD_SAMPLE, key=cos.get)
    print(f'\n  frozen YOLOv3 step bf16 vs fp32: heads {herr}, loss rel {lrel:.1e}, gradient norms: median {np.median(list(nrm.values())):.1e} worst {nrm[wn]:.1e} ({wn}), '
          f'cosine: sampled min {cos[wc]:.5f} ({wc}), over all tensors {cos[wa]:.5f} ({wa})')
    assert all(torch.isfinite(v).all() for v in g16.values())
    missed = [what for what, ok in (('heads', max(herr) < 1.3e-1), ('loss', lrel < 1e-3), (f'gradient norm of {wn}', nrm[wn] < 1.2e-1),
                                    (f'cosine of {wc}', cos[wc] > 0.96)) if not ok]
    assert not missed, missed


# ================================================================================================ 6. graph and fit loop
def test_graphed_frozen_backbone_step_is_bit_identical_with_eager():
    import fastvision_amd
    from fastvision_amd import FusedAdam, ops
    from fastvision_amd.graphs import GraphedTrainStep
    from fastvision_amd.loss import Yolov3Loss
    from fastvision_amd.synthetic import synthetic_batch
    batches = [synthetic_batch(2, 64, seed=s) for s in (1234, 7, 99)]
    cap = max(t.shape[0] for _, t in batches) + 5

    def make():
        net = frozen_model(True)
        return net, Yolov3Loss(net, 0.5, 0.05, 1.0, 0.5), FusedAdam(net.parameters(), lr=1e-4, betas=(0.937, 0.999), weight_decay=5e-4, capturable=True)
    prev = ops.set_wgrad_plan('alone')                # one fp32 summation order of dW for the eager and the single-stream captured step
    try:
        with fastvision_amd.compute_dtype(FP):
            net, crit, opt = make()
            want = []
            for im, tg in batches:
                pred = net(im.to(DEV))
                opt.zero_grad()
                loss = crit(pred, tg.to(DEV))
                loss.backward()
                opt.step()
                want.append(loss.detach().clone())
            torch.cuda.synchronize()
            net2, crit2, opt2 = make()
            assert net2.training and not net2.backbone.conv0.bn.training          # the top-level flag is what GraphedTrainStep reads
            step = GraphedTrainStep(net2, lambda p, t: crit2(p, t), opt2, batches[0][0].to(DEV), batches[0][1].to(DEV), max_targets=cap)
            got = [step(im.to(DEV), tg.to(DEV)).clone() for im, tg in batches]
            torch.cuda.synchronize()
    finally:
        ops.set_wgrad_plan(prev)
    for a, b in zip(got, want):
        assert torch.equal(a, b), (a, b)
    s1, s2 = net.state_dict(), net2.state_dict()
    for k in s1:
        assert torch.equal(s1[k], s2[k]), k
    calib = calibrated_state()
    for k in s1:
        if k.startswith('backbone.') and ('running' in k or 'num_batches' in k):
            assert torch.equal(s2[k].cpu(), calib[k]), k                            # frozen: untouched by capture, warm-up and replays
    assert s2['neck.neck1.conv1.bn.num_batches_tracked'].item() == calib['neck.neck1.conv1.bn.num_batches_tracked'].item() + 3


def test_fit_loop_keeps_frozen_statistics_and_learns():
    import fastvision_amd
    from fastvision_amd import FusedAdam
    from fastvision_amd.loss import Yolov3Loss
    from fastvision_amd.synthetic import synthetic_batch
    from fastvision_amd.utils import Fit, freeze_batchnorm
    net = lib_model()
    net.load_state_dict(calibrated_state())
    freeze_batchnorm(net)
    calib = calibrated_state()
    # a fine-tuning learning rate: nothing renormalises a frozen layer's output after a step (a first version of this test, statistics
    # of two images and lr 1e-3, read NaN from the first epoch on; which of the two did it was not separated)
    loader = [synthetic_batch(2, 64, seed=s) for s in (1, 2)]
    with fastvision_amd.compute_dtype(FP):
        crit = Yolov3Loss(net, 0.5, 0.05, 1.0, 0.5)
        opt = FusedAdam(net.parameters(), lr=1e-4, betas=(0.937, 0.999))
        fit = Fit(net, torch.device(DEV), opt, None, crit, end_epoch=3, train_loader=loader, save_last=None)
        fit.run_epoches()
    torch.cuda.synchronize()
    assert net.training and not any(m.training for m in net.modules() if isinstance(m, nn.BatchNorm2d))
    state = net.state_dict()
    stats = [k for k in state if 'running' in k or 'num_batches' in k]
    assert len(stats) == 3 * 72
    for k in stats:
        assert torch.equal(state[k].cpu(), calib[k]), k
    first, last = np.mean(fit.history[0]), np.mean(fit.history[-1])
    print(f'\n  frozen fit loop: mean loss per epoch {[round(float(np.mean(h)), 4) for h in fit.history]}')
    assert np.isfinite(last) and last < first
    twin = copy.deepcopy(net)                        # what SaveModel(weights_only=False) does
    twin.train()
    assert not twin.backbone.conv0.bn.training
