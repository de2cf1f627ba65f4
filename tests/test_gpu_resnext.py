"""resnext50_32x4d / resnext101_32x8d on the device against the CPU restatement (tests/resnext_restatement.py: StockResNeXt), with the
machinery of tests/test_gpu_resnet.py (imported as T; that module is unchanged): one fp32 train step of both factories against float64 on
the same weights, eval mode, ``including_top=False``, a frozen-BatchNorm backward through one grouped conv_bn_relu, bf16 against the
float64 restatement, the train step as a whole (no ATen compute, no host synchronisation, same bits from the same seed and between eager
and a captured graph) and the older families' keys.  At 2 x 3 x 64 x 64 the grouped layers run at 16^2, 8^2, 4^2 and 2^2 with every Cg."""
import hashlib
from unittest import mock

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import test_gpu_resnet as T
from resnext_restatement import NAMES, StockResNeXt, _XBlock

pytestmark = pytest.mark.gpu

DEV = T.DEV
BF, FP = torch.bfloat16, torch.float32
SEED = 9                         # fp32: the restatement alone stays under T.KINK_SHARE_MAX for both factories (test_resnext_restatement_cpu.py)
SEED_BF16 = 11                   # bf16: at seed 9 the CPU bf16-store emulation itself is 1.32e-1 off float64 in a gradient norm, over the 1.2e-1 bar


def _mag_through_bn(x, conv, bn, y):
    """T._mag_through_bn with the convolution's groups"""
    mag = F.conv2d(x.abs(), conv.weight.abs(), None, conv.stride, conv.padding, 1, conv.groups)
    sc = (bn.weight / (y.var((0, 2, 3), unbiased=False) + bn.eps).sqrt()).abs()[None, :, None, None]
    return (mag + mag.mean((0, 2, 3), keepdim=True)) * sc + bn.bias.abs()[None, :, None, None]


def ref64_forward(r64, ref32, images, decisions):
    """T._ref64_forward, its kink room computed with the grouped convolutions' own terms"""
    with mock.patch.object(T, '_mag_through_bn', _mag_through_bn):
        return T._ref64_forward(r64, ref32, images, decisions)


def _reference(name, seed, including_top=True):
    """StockResNeXt with torch's default init (the reference's: resnext.py calls no initialize_weights) and T._reference's BatchNorm / fc
    scaling: gamma in 0.5 ... 1.5, a tenth of it on the BatchNorm that closes a branch, small biases and statistics, a tenth of the fc weight."""
    torch.manual_seed(seed)
    ref = StockResNeXt(name, num_classes=10, including_top=including_top)
    g = torch.Generator().manual_seed(seed + 1)
    tails = {id(b.units()[-1][1]) for b in ref.modules() if isinstance(b, _XBlock)}
    with torch.no_grad():
        for m in ref.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                if id(m) in tails:
                    m.weight.mul_(0.1)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
                m.running_mean.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.bias.shape, generator=g) + 0.5)
        if including_top:
            ref.fc.weight.mul_(0.1)
    return ref.train()


def _pair(name, seed, including_top=True):
    from fastvision_amd.classfication import models
    ref = _reference(name, seed, including_top)
    net = getattr(models, name)(num_classes=10, including_top=including_top)
    net.load_state_dict(ref.state_dict(), strict=True)
    return ref, net.to(DEV).train()


def _double(ref, name, including_top=True):
    r64 = StockResNeXt(name, num_classes=10, including_top=including_top).double()
    r64.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in ref.state_dict().items()})
    return r64.train()


def _grad_names():
    """the stem, conv2 (grouped) of a stride-1 and -- from res3 on -- a stride-2 block in every stage, 1x1s, a shortcut, a BatchNorm, the fc"""
    return ['conv1.0.weight', 'res2.0.conv2.weight', 'res2.1.conv2.weight', 'res3.0.conv2.weight', 'res3.1.conv2.weight', 'res4.0.conv2.weight',
            'res4.1.conv2.weight', 'res5.0.conv2.weight', 'res5.1.conv2.weight', 'res2.0.conv1.weight', 'res3.1.conv3.weight',
            'res3.0.downsample.0.weight', 'res5.0.downsample.1.weight', 'res4.1.bn2.bias', 'fc.weight', 'fc.bias']


def _both_steps(name, dtype, seed, adopt=True):
    import fastvision_amd
    from fastvision_amd.loss import CrossEntropyLoss
    ref, net = _pair(name, seed)
    images, labels = T._batch(2, 64, seed + 2)
    r64 = _double(ref, name)
    share = 0.0
    if adopt:
        rl, share = ref64_forward(r64, ref, images, T._device_decisions(name, net, images, dtype))
    else:
        rl = r64(images.double())
    rloss = F.cross_entropy(rl, labels)
    rloss.backward()
    with fastvision_amd.compute_dtype(dtype):
        gl = net(images.to(DEV))
        gloss = CrossEntropyLoss()(gl, labels.to(DEV))
        gloss.backward()
    torch.cuda.synchronize()
    assert gl.dtype == torch.float32 and tuple(gl.shape) == (2, 10)
    return ref, r64, net, rl.detach(), rloss.item(), gl.detach().cpu(), gloss.item(), images, labels, share


# ================================================================================================ fp32 against float64
@pytest.mark.parametrize('name', NAMES)
def test_train_step_fp32_both_factories(name):
    """2 x 3 x 64 x 64, 10 classes.  Bar: 1e-3 on logits, loss, the sampled gradients and every BatchNorm buffer; then eval mode."""
    import fastvision_amd
    ref, r64, net, rl, rloss, gl, gloss, images, labels, share = _both_steps(name, FP, SEED)
    rp, gp = dict(r64.named_parameters()), dict(net.named_parameters())
    figs = {'logits': T.rel_err(gl, rl), 'loss': abs(gloss - rloss) / abs(rloss)}
    for k in _grad_names():
        figs[k] = T.rel_err(gp[k].grad, rp[k].grad)
    rb, gb = dict(r64.named_buffers()), dict(net.named_buffers())
    assert len(rb) == len(gb)
    for k, v in rb.items():
        if k.endswith('num_batches_tracked'):
            assert gb[k].item() == v.item() == 1, k
        else:
            figs[k] = T.rel_err(gb[k], v)
    worst = max(figs, key=figs.get)
    print(f'\n  {name} fp32 64x64: logits {figs["logits"]:.2e} loss {figs["loss"]:.2e}; worst {worst} {figs[worst]:.2e}; '
          f'largest share of a layer\'s decisions taken from the device {share:.1e} (cap {T.KINK_SHARE_MAX:.0e})')
    assert all(np.isfinite(v) and v < 1e-3 for v in figs.values()), {k: v for k, v in figs.items() if not v < 1e-3}
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.parameters())
    net.load_state_dict(ref.state_dict(), strict=True)
    ref.eval(), net.eval()
    with torch.no_grad(), fastvision_amd.compute_dtype(FP):
        e = T.rel_err(net(images.to(DEV)), ref.double()(images.double()))
    print(f'  {name} fp32 64x64 eval logits {e:.2e}')
    assert e < 1e-3, e


def test_including_top_false_shapes_and_values():
    import fastvision_amd
    name = 'resnext50_32x4d'
    ref, net = _pair(name, SEED, including_top=False)
    images, _ = T._batch(2, 64, SEED + 2)
    r64 = _double(ref, name, including_top=False)
    with torch.no_grad(), fastvision_amd.compute_dtype(FP):
        want, got = r64(images.double()), net(images.to(DEV))
    assert [tuple(t.shape) for t in got] == [(2, 2048, 2, 2), (2, 1024, 4, 4), (2, 512, 8, 8)]          # [res5, res4, res3]
    for g, w in zip(got, want):
        assert tuple(g.shape) == tuple(w.shape) and T.rel_err(g, w) < 1e-3


@pytest.mark.parametrize('stride', [1, 2])
def test_frozen_bn_backward_through_a_grouped_block(stride):
    """bn.eval(): the one-pass backward (ops.frozen_bn_bwd) in front of fva_gconv_dgrad / fva_gconv_wgrad, against float64 autograd."""
    import fastvision_amd
    from fastvision_amd import resnet_ops as ro
    gen = torch.Generator().manual_seed(17 + stride)
    conv = nn.Conv2d(128, 128, 3, stride, 1, groups=32, bias=False)
    bn = nn.BatchNorm2d(128)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(128, generator=gen) + 0.5)
        bn.bias.copy_(torch.randn(128, generator=gen) * 0.1)
        bn.running_mean.copy_(torch.randn(128, generator=gen) * 0.1)
        bn.running_var.copy_(torch.rand(128, generator=gen) + 0.5)
    x = torch.randn(2, 128, 6, 10, generator=gen)
    dz = torch.randn(2, 128, (6 - 1) // stride + 1, (10 - 1) // stride + 1, generator=gen)
    import copy
    c64, b64 = copy.deepcopy(conv).double(), copy.deepcopy(bn).double().eval()
    x64 = x.double().requires_grad_(True)
    torch.relu(b64(c64(x64))).backward(dz.double())
    conv, bn = conv.to(DEV), bn.to(DEV).eval()
    xg = x.to(DEV).requires_grad_(True)
    with fastvision_amd.compute_dtype(FP):
        z = ro.conv_bn_relu(xg, conv, bn)
        z.backward(dz.to(DEV))
    torch.cuda.synchronize()
    assert bn.num_batches_tracked.item() == 0
    figs = {'z': T.rel_err(z, torch.relu(b64(c64(x64)))), 'dx': T.rel_err(xg.grad, x64.grad), 'dw': T.rel_err(conv.weight.grad, c64.weight.grad),
            'dgamma': T.rel_err(bn.weight.grad, b64.weight.grad), 'dbeta': T.rel_err(bn.bias.grad, b64.bias.grad)}
    print(f'\n  frozen grouped block stride {stride}: {figs}')
    assert all(v < 1e-5 for v in figs.values()), figs


@pytest.mark.parametrize('kind', ['dense 1x1', 'grouped 3x3'])
def test_wide_fp32_block_takes_the_add_relu_passes_and_refuses_the_frozen_backward(kind):
    """fp32 tensors of 2048 channels (conv1 / conv2 of resnext101_32x8d's res5) are more than the 256 chunks per pixel fva_bn_relu_apply and
    its backward serve: resnet_ops._wide sends them through fva_bn_add_relu_* with a zero addend.  One such block, training mode, against
    float64 autograd; bar 1e-4 of each tensor's scale (one convolution and one BatchNorm over 8 values per channel in fp32: the whole
    models hold 1e-3).  The frozen one-pass backward has no such route and must refuse; the eval forward itself runs."""
    import copy
    import fastvision_amd
    from fastvision_amd import resnet_ops as ro
    gen = torch.Generator().manual_seed(23)
    conv = nn.Conv2d(64, 2048, 1, bias=False) if kind == 'dense 1x1' else nn.Conv2d(2048, 2048, 3, 1, 1, groups=32, bias=False)
    bn = nn.BatchNorm2d(2048)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(2048, generator=gen) + 0.5)
        bn.bias.copy_(torch.randn(2048, generator=gen) * 0.1)
    x = torch.randn(2, conv.in_channels, 2, 2, generator=gen)
    dz = torch.randn(2, 2048, 2, 2, generator=gen)
    c64, b64 = copy.deepcopy(conv).double(), copy.deepcopy(bn).double().train()
    x64 = x.double().requires_grad_(True)
    z64 = torch.relu(b64(c64(x64)))
    z64.backward(dz.double())
    conv, bn = conv.to(DEV), bn.to(DEV).train()
    assert ro._wide(0, 2048) and not ro._wide(1, 2048) and not ro._wide(0, 1024)
    xg = x.to(DEV).requires_grad_(True)
    with fastvision_amd.compute_dtype(FP):
        z = ro.conv_bn_relu(xg, conv, bn)
        z.backward(dz.to(DEV))
    torch.cuda.synchronize()
    figs = {'z': T.rel_err(z, z64), 'dx': T.rel_err(xg.grad, x64.grad), 'dw': T.rel_err(conv.weight.grad, c64.weight.grad),
            'dgamma': T.rel_err(bn.weight.grad, b64.weight.grad), 'dbeta': T.rel_err(bn.bias.grad, b64.bias.grad),
            'running_mean': T.rel_err(bn.running_mean, b64.running_mean), 'running_var': T.rel_err(bn.running_var, b64.running_var)}
    print(f'\n  wide fp32 {kind}: {figs}')
    assert all(v < 1e-4 for v in figs.values()), figs
    bn.eval(), b64.eval()
    with fastvision_amd.compute_dtype(FP):
        with torch.no_grad():
            assert T.rel_err(ro.conv_bn_relu(x.to(DEV), conv, bn), torch.relu(b64(c64(x.double())))) < 1e-4
        x2 = x.to(DEV).requires_grad_(True)
        z = ro.conv_bn_relu(x2, conv, bn)
        with pytest.raises(RuntimeError, match='frozen statistics.*wider than 1024 channels'):
            z.float().sum().backward()
    torch.cuda.synchronize()


# ================================================================================================ bf16
# cosine of the bf16 store emulation (T._emulated_bf16_step on StockResNeXt) with the float64 restatement, measured on the CPU at SEED_BF16,
# 2 x 3 x 64 x 64, and the bar from it: 0.96, or 1 - 2 (1 - cosine) rounded down to two digits where the emulation itself is below that
BF16_COSINE = {
    'conv1.0.weight': (0.9478, 0.89), 'res2.0.conv2.weight': (0.9510, 0.90), 'res2.1.conv2.weight': (0.9629, 0.92),
    'res3.0.conv2.weight': (0.9584, 0.91), 'res3.1.conv2.weight': (0.9558, 0.91), 'res4.0.conv2.weight': (0.9594, 0.91),
    'res4.1.conv2.weight': (0.9568, 0.91), 'res5.0.conv2.weight': (0.9717, 0.94), 'res5.1.conv2.weight': (0.9738, 0.94),
    'res2.0.conv1.weight': (0.9530, 0.90), 'res3.1.conv3.weight': (0.9624, 0.92), 'res3.0.downsample.0.weight': (0.9627, 0.92),
    'res5.0.downsample.1.weight': (0.9981, 0.96), 'res4.1.bn2.bias': (0.9561, 0.91), 'fc.weight': (0.9999, 0.96), 'fc.bias': (1.0000, 0.96),
}


def test_train_step_bf16_resnext50():
    """The bars of T.test_train_step_bf16: logits within 1.3e-1 of their scale, gradient norms within 1.2e-1, sampled cosines above
    BF16_COSINE's bar.  The emulation on the CPU at SEED_BF16: logits 1.0e-2 of their scale from float64, gradient norms at most 6.4e-2 off."""
    name = 'resnext50_32x4d'
    ref, r64, net, rl, rloss, gl, gloss, images, labels, _ = _both_steps(name, BF, SEED_BF16, adopt=False)
    rp, gp = dict(r64.named_parameters()), dict(net.named_parameters())
    T._emulated_bf16_step(ref.train(), images, labels)
    ep = dict(ref.named_parameters())
    herr = T.rel_err(gl, rl)
    rel, cos, bar = {}, {}, {}
    for k, p in rp.items():
        a, b = gp[k].grad.double().cpu(), p.grad.double()
        assert torch.isfinite(a).all(), k
        rel[k] = abs(a.norm().item() - b.norm().item()) / max(b.norm().item(), 1e-300)
    for k in _grad_names():
        cos[k] = T._cosine(gp[k].grad, rp[k].grad)
        bar[k] = (BF16_COSINE[k][1], T._cosine(ep[k].grad, rp[k].grad))
    wk = max(rel, key=rel.get)
    print(f'\n  {name} bf16 64: logits {herr:.2e} of scale, loss {gloss:.5f} vs {rloss:.5f}, gradient norms median {np.median(list(rel.values())):.2e} '
          f'max {rel[wk]:.2e} ({wk}); cosine device / emulation / bar: ' + ', '.join(f'{k} {cos[k]:.4f} / {bar[k][1]:.4f} / {bar[k][0]:.2f}' for k in cos))
    assert herr < 1.3e-1
    assert rel[wk] < 1.2e-1, wk
    for k in cos:
        assert cos[k] > bar[k][0], (k, cos[k], bar[k])


# ================================================================================================ the train step as a whole
NAME = 'resnext50_32x4d'


def test_train_step_runs_without_aten_compute(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError('ATen op in the ResNeXt train step')
    net, crit, opt = T._train_parts(NAME)
    images, labels = T._batch(2, 64, 1)
    for fn in ('conv2d', 'batch_norm', 'relu', 'max_pool2d', 'adaptive_avg_pool2d', 'linear', 'cross_entropy', 'unfold'):
        monkeypatch.setattr(F, fn, refuse)
    monkeypatch.setattr(torch, 'relu', refuse)
    loss = T._step(net, crit, opt, images.to(DEV), labels.to(DEV))
    monkeypatch.undo()
    assert torch.isfinite(loss).item()
    assert net.res2[0].bn2.num_batches_tracked.item() == 1 and net.res5[0].bn2.num_batches_tracked.item() == 1


def test_train_step_does_not_synchronise_the_host():
    net, crit, opt = T._train_parts(NAME)
    images, labels = T._batch(4, 64, 2)
    images, labels = images.to(DEV), labels.to(DEV)
    for _ in range(2):
        T._step(net, crit, opt, images, labels)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        loss = T._step(net, crit, opt, images, labels)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert torch.isfinite(loss).item()


def test_same_seed_trains_to_the_same_bits():
    images, labels = T._batch(4, 64, 9)
    runs = []
    for _ in range(2):
        net, crit, opt = T._train_parts(NAME)
        losses = [T._step(net, crit, opt, images.to(DEV), labels.to(DEV)).item() for _ in range(3)]
        torch.cuda.synchronize()
        runs.append((losses, [p.detach().clone() for p in net.parameters()], [b.detach().clone() for b in net.buffers()]))
    assert runs[0][0] == runs[1][0] and len(set(runs[0][0])) == 3, runs
    for a, b in zip(runs[0][1] + runs[0][2], runs[1][1] + runs[1][2]):
        assert torch.equal(a, b)


def test_graphed_step_is_bit_identical_with_eager():
    """Three captured steps against three eager ones: the grouped layers read the master weight the optimizer has just written (no packed
    copy, nothing keyed on the parameter's version), so a replay sees every update."""
    from fastvision_amd import ops
    from fastvision_amd.graphs import GraphedTrainStep
    gen = torch.Generator().manual_seed(5)
    batches = [(torch.randn(4, 3, 64, 64, generator=gen), torch.randint(0, 10, (4, 1), generator=gen).float()) for _ in range(3)]
    prev = ops.set_wgrad_side_stream(False)
    try:
        net, crit, opt = T._train_parts(NAME)
        want = [T._step(net, crit, opt, im.to(DEV), lab.to(DEV)) for im, lab in batches]
        torch.cuda.synchronize()
    finally:
        ops.set_wgrad_side_stream(prev)
    net2, crit2, opt2 = T._train_parts(NAME)
    step = GraphedTrainStep(net2, lambda p, t: crit2(p, t), opt2, batches[0][0].to(DEV), batches[0][1].to(DEV))
    got = [step(im.to(DEV), lab.to(DEV)).clone() for im, lab in batches]
    torch.cuda.synchronize()
    assert len({w.item() for w in want}) == 3
    for a, b in zip(got, want):
        assert torch.equal(a, b), (a, b)
    for (k, p), q in zip(net.state_dict().items(), net2.state_dict().values()):
        assert torch.equal(p, q), k
    for p, q in zip(net.parameters(), net2.parameters()):
        assert torch.equal(opt.state[p]['momentum_buffer'], opt2.state[q]['momentum_buffer'])


def test_grouped_refusals_name_the_contract():
    from fastvision_amd import resnet_ops as ro
    x = torch.zeros(1, 96, 4, 4, device=DEV)
    with pytest.raises(RuntimeError, match='Cg in'):
        ro.conv_bn_relu(x, nn.Conv2d(96, 96, 3, 1, 1, groups=32, bias=False).to(DEV), nn.BatchNorm2d(96).to(DEV))          # Cg = 3
    with pytest.raises(RuntimeError, match='bias-free'):
        ro.conv_bn_relu(torch.zeros(1, 64, 4, 4, device=DEV), nn.Conv2d(64, 64, 1, 1, 0, groups=4, bias=False).to(DEV), nn.BatchNorm2d(64).to(DEV))
    with pytest.raises(RuntimeError, match='bias-free'):
        ro.conv_bn_add_relu(torch.zeros(1, 64, 4, 4, device=DEV), nn.Conv2d(64, 64, 3, 1, 1, groups=4, bias=False).to(DEV),
                            nn.BatchNorm2d(64).to(DEV), torch.zeros(1, 64, 4, 4, device=DEV))


# sha1 of '\\n'.join(state_dict keys), computed on the parent commit
OLD_FAMILIES = {'resnet50': (320, '5e25e7bb36a5eefc9d7039a945fb49312d1642a8'), 'darknet53': (314, 'f2b6d9c3e113bd2bf3efa00a1c326f4f59f0b8cb')}


def test_older_families_keep_their_keys():
    from fastvision_amd.classfication import models
    for name, (count, digest) in OLD_FAMILIES.items():
        keys = list(getattr(models, name)(num_classes=10).state_dict())
        assert len(keys) == count, (name, len(keys))
        assert hashlib.sha1('\n'.join(keys).encode()).hexdigest() == digest, name
