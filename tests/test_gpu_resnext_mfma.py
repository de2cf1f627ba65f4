"""resnext50_32x4d on the device under resnet_ops.set_grouped_path('mfma') (restored after every test), with the machinery and the bars
of tests/test_gpu_resnext.py (imported as X; that module is unchanged): the bf16 train step against the float64 restatement, three
captured steps bit-identical with three eager ones, the same seed training to the same bits, and a frozen-BatchNorm backward through one
grouped block.  At 2 x 3 x 64 x 64 the stride-1 grouped layers run at 16^2, 8^2, 4^2 and 2^2 with Cg = 4, 8, 16, 32; every test also
asserts that the matrix-unit entries were the ones launched."""
import collections
import contextlib
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

import test_gpu_resnet as T
import test_gpu_resnext as X

pytestmark = pytest.mark.gpu

DEV = T.DEV
NAME = 'resnext50_32x4d'


@contextlib.contextmanager
def mfma_path():
    """'mfma' for the body, the previous path afterwards; yields a counter of the entry points launched meanwhile."""
    import __graft_entry__ as ge
    ge.build()
    from fastvision_amd import _lib, resnet_ops as ro
    counts = collections.Counter()
    real = _lib.call

    def counting(name, *args):
        counts[name] += 1
        return real(name, *args)
    prev = ro.set_grouped_path('mfma')
    _lib.call = counting
    try:
        yield counts
    finally:
        _lib.call = real
        ro.set_grouped_path(prev)
    assert ro.get_grouped_path() == prev


def _assert_routed(counts, s1_layers, s2_layers, steps=1):
    """resnext50 has 13 stride-1 and 3 stride-2 grouped layers: the former on the matrix units, the latter on the plain kernels."""
    assert counts['fva_gconv_mfma_pack'] == counts['fva_gconv_mfma_fwd'] == s1_layers * steps, counts
    assert counts['fva_gconv_mfma_wgrad'] == counts['fva_gconv_mfma_dgrad'] == s1_layers * steps, counts
    assert counts['fva_gconv_fwd'] == counts['fva_gconv_wgrad'] == counts['fva_gconv_dgrad'] == s2_layers * steps, counts


def test_train_step_bf16_resnext50_on_the_matrix_units():
    """X.test_train_step_bf16_resnext50 under 'mfma': the same seed, the same bars (logits within 1.3e-1 of their scale, gradient norms
    within 1.2e-1, sampled cosines above X.BF16_COSINE's bar)."""
    with mfma_path() as counts:
        ref, r64, net, rl, rloss, gl, gloss, images, labels, _ = X._both_steps(NAME, X.BF, X.SEED_BF16, adopt=False)
    _assert_routed(counts, 13, 3)
    rp, gp = dict(r64.named_parameters()), dict(net.named_parameters())
    T._emulated_bf16_step(ref.train(), images, labels)
    ep = dict(ref.named_parameters())
    herr = T.rel_err(gl, rl)
    rel, cos, bar = {}, {}, {}
    for k, p in rp.items():
        a, b = gp[k].grad.double().cpu(), p.grad.double()
        assert torch.isfinite(a).all(), k
        rel[k] = abs(a.norm().item() - b.norm().item()) / max(b.norm().item(), 1e-300)
    for k in X._grad_names():
        cos[k] = T._cosine(gp[k].grad, rp[k].grad)
        bar[k] = (X.BF16_COSINE[k][1], T._cosine(ep[k].grad, rp[k].grad))
    wk = max(rel, key=rel.get)
    print(f'\n  {NAME} bf16 64 mfma: logits {herr:.2e} of scale, loss {gloss:.5f} vs {rloss:.5f}, gradient norms median '
          f'{np.median(list(rel.values())):.2e} max {rel[wk]:.2e} ({wk}); cosine device / emulation / bar: '
          + ', '.join(f'{k} {cos[k]:.4f} / {bar[k][1]:.4f} / {bar[k][0]:.2f}' for k in cos))
    assert herr < 1.3e-1
    assert rel[wk] < 1.2e-1, wk
    for k in cos:
        assert cos[k] > bar[k][0], (k, cos[k], bar[k])


def test_same_seed_trains_to_the_same_bits():
    images, labels = T._batch(4, 64, 9)
    runs = []
    with mfma_path() as counts:
        for _ in range(2):
            net, crit, opt = T._train_parts(NAME)
            losses = [T._step(net, crit, opt, images.to(DEV), labels.to(DEV)).item() for _ in range(3)]
            torch.cuda.synchronize()
            runs.append((losses, [p.detach().clone() for p in net.parameters()], [b.detach().clone() for b in net.buffers()]))
    _assert_routed(counts, 13, 3, steps=6)
    assert runs[0][0] == runs[1][0] and len(set(runs[0][0])) == 3, runs
    for a, b in zip(runs[0][1] + runs[0][2], runs[1][1] + runs[1][2]):
        assert torch.equal(a, b)


def test_graphed_step_is_bit_identical_with_eager():
    """Three captured steps against three eager ones: the pack launch is part of the captured forward, so a replay packs the weights the
    optimizer has just written."""
    from fastvision_amd import ops
    from fastvision_amd.graphs import GraphedTrainStep
    gen = torch.Generator().manual_seed(5)
    batches = [(torch.randn(4, 3, 64, 64, generator=gen), torch.randint(0, 10, (4, 1), generator=gen).float()) for _ in range(3)]
    with mfma_path() as counts:
        prev = ops.set_wgrad_side_stream(False)
        try:
            net, crit, opt = T._train_parts(NAME)
            want = [T._step(net, crit, opt, im.to(DEV), lab.to(DEV)) for im, lab in batches]
            torch.cuda.synchronize()
        finally:
            ops.set_wgrad_side_stream(prev)
        _assert_routed(counts, 13, 3, steps=3)
        net2, crit2, opt2 = T._train_parts(NAME)
        step = GraphedTrainStep(net2, lambda p, t: crit2(p, t), opt2, batches[0][0].to(DEV), batches[0][1].to(DEV))
        got = [step(im.to(DEV), lab.to(DEV)).clone() for im, lab in batches]
        torch.cuda.synchronize()
    assert counts['fva_gconv_mfma_pack'] > 13 * 3                  # the capture launched them too
    assert len({w.item() for w in want}) == 3
    for a, b in zip(got, want):
        assert torch.equal(a, b), (a, b)
    for (k, p), q in zip(net.state_dict().items(), net2.state_dict().values()):
        assert torch.equal(p, q), k
    for p, q in zip(net.parameters(), net2.parameters()):
        assert torch.equal(opt.state[p]['momentum_buffer'], opt2.state[q]['momentum_buffer'])


def test_frozen_bn_backward_through_a_grouped_block():
    """bn.eval() in bf16: the one-pass frozen backward in front of fva_gconv_mfma_wgrad / _dgrad, against float64 autograd on the same
    bf16-valued x, weight and dz, with the DEVICE's ReLU decisions (z > 0) so that an element a rounding carries across the kink is not
    compared with its other branch.  The bars are derived, per output, from the three bf16 stores on the way (y, z and dy, each within
    E = 2^-8 of the stored value; everything else is fp32 or exact): z <= E (|y scale| + |z|), dx <= E (sum |dy w| + |dx|), dw <= E sum |dy x|,
    dgamma <= E sum |du y| rstd, as shares of the tensor's largest element (T.rel_err), plus 1e-5 for the fp32 sums."""
    import fastvision_amd
    import torch.nn.functional as F
    from fastvision_amd import resnet_ops as ro
    E = 2.0 ** -8
    gen = torch.Generator().manual_seed(18)
    conv = nn.Conv2d(128, 128, 3, 1, 1, groups=32, bias=False)
    bn = nn.BatchNorm2d(128)
    with torch.no_grad():
        conv.weight.copy_(conv.weight.bfloat16().float())
        bn.weight.copy_(torch.rand(128, generator=gen) + 0.5)
        bn.bias.copy_(torch.randn(128, generator=gen) * 0.1)
        bn.running_mean.copy_(torch.randn(128, generator=gen) * 0.1)
        bn.running_var.copy_(torch.rand(128, generator=gen) + 0.5)
    x = torch.randn(2, 128, 6, 10, generator=gen).bfloat16().float()
    dz = torch.randn(2, 128, 6, 10, generator=gen).bfloat16().float()
    c64, b64 = copy.deepcopy(conv).double(), copy.deepcopy(bn).double().eval()
    conv, bn = conv.to(DEV), bn.to(DEV).eval()
    xg = x.to(DEV).requires_grad_(True)
    with mfma_path() as counts, fastvision_amd.compute_dtype(torch.bfloat16):
        z = ro.conv_bn_relu(xg, conv, bn)
        z.backward(dz.to(DEV))
        torch.cuda.synchronize()
    assert counts['fva_gconv_mfma_pack'] == counts['fva_gconv_mfma_fwd'] == counts['fva_gconv_mfma_wgrad'] == counts['fva_gconv_mfma_dgrad'] == 1
    assert counts['fva_bn_finalize'] == 0 and counts['fva_gconv_fwd'] == 0 and bn.num_batches_tracked.item() == 0
    mask = (z.detach().cpu() > 0).double()
    x64 = x.double().requires_grad_(True)
    y64 = c64(x64)
    u64 = b64(y64)
    du = dz.double() * mask
    (u64 * du).sum().backward()
    z64 = (u64 * mask).detach()
    scale = (b64.weight / (b64.running_var + b64.eps).sqrt()).detach()[None, :, None, None]
    rstd = (1.0 / (b64.running_var + b64.eps).sqrt())[None, :, None, None]
    w_abs, dy_abs = c64.weight.detach().abs(), (du * scale).abs()
    s_dx = F.conv_transpose2d(dy_abs, w_abs, None, 1, 1, 0, 32)
    s_dw = torch.nn.grad.conv2d_weight(x.double().abs(), w_abs.shape, dy_abs, 1, 1, 1, 32)
    s_dg = (du.abs() * y64.detach().abs() * rstd).sum((0, 2, 3))
    top = lambda t: t.detach().abs().max().item()
    bars = {'z': E * (top(y64 * scale) / top(z64) + 1), 'dx': E * (top(s_dx) / top(x64.grad) + 1), 'dw': E * top(s_dw) / top(c64.weight.grad),
            'dgamma': E * top(s_dg) / top(b64.weight.grad), 'dbeta': 0.0}
    figs = {'z': T.rel_err(z, z64), 'dx': T.rel_err(xg.grad, x64.grad), 'dw': T.rel_err(conv.weight.grad, c64.weight.grad),
            'dgamma': T.rel_err(bn.weight.grad, b64.weight.grad), 'dbeta': T.rel_err(bn.bias.grad, b64.bias.grad)}
    print('\n  frozen grouped block, bf16, mfma: ' + ', '.join(f'{k} {figs[k]:.2e} (bar {bars[k] + 1e-5:.2e})' for k in figs))
    assert all(figs[k] <= bars[k] + 1e-5 for k in figs), (figs, bars)
