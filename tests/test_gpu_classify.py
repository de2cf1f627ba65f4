"""Darknet-53 classification on the device (fva_gap_fwd / fva_gap_bwd, fva_softmax_ce, fva_top1_accuracy): each kernel against
float64 CPU torch, the whole classifier (darknet53 with its top) against the CPU oracle backbone plus torch's pooling / linear /
cross-entropy with the same weights, no ATen in the top, no host synchronisation, HIP-graph capture of the train step with float
[N, 1] labels, and a short utils.Fit run."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


# ---------------------------------------------------------------------------------------------------------------- pooling
GAP_SHAPES = [(2, 1024, 7, 7), (3, 64, 13, 13), (1, 8, 1, 1), (4, 1024, 20, 20)]


def _gap_run(x, dtype, g):
    from fastvision_amd import ops
    out = ops.global_avg_pool(x, dtype)
    out.backward(g)
    return out.detach().clone()


@pytest.mark.parametrize('shape,dtype', list(itertools.product(GAP_SHAPES, [torch.float32, torch.bfloat16])))
def test_gap_forward_backward_against_float64(shape, dtype):
    from fastvision_amd import ops
    B, Cc, H, W = shape
    gen = torch.Generator().manual_seed(B * Cc + H)
    x = torch.randn(shape, generator=gen).to(dtype)                    # values the compute dtype holds exactly
    g = torch.randn(B, Cc, generator=gen)
    want = x.double().mean((2, 3))
    want_dx = (g.double() / (H * W))[:, :, None, None].expand(shape)
    for form in ('halo', 'nchw'):
        if form == 'halo':
            buf, view = ops.halo_alloc(B, Cc, H, W, dtype, DEV, 1)
            buf.zero_()
            view.copy_(x.to(DEV))
            buf.requires_grad_(True)
            xin = buf[:, 1:1 + H, 1:1 + W, :].permute(0, 3, 1, 2)
            assert ops.halo_info(xin.detach(), dtype) is not None          # the zero-copy path is what is being tested
        else:
            leaf = x.float().contiguous().to(DEV).requires_grad_(True)     # foreign fp32 NCHW: packed on entry
            xin = leaf
        runs = []
        for _ in range(2):
            if form == 'halo':
                buf.grad = None
            else:
                leaf.grad = None
            out = _gap_run(xin, dtype, g.to(DEV))
            dx = buf.grad[:, 1:1 + H, 1:1 + W, :].permute(0, 3, 1, 2) if form == 'halo' else leaf.grad
            runs.append((out, dx.detach().clone()))
        (o1, d1), (o2, d2) = runs
        assert o1.dtype == torch.float32 and tuple(o1.shape) == (B, Cc)
        assert torch.equal(o1, o2) and torch.equal(d1, d2), form              # run-to-run bit-identical
        assert rel_err(o1, want) < 1e-5, (form, rel_err(o1, want))
        tol = 1e-6 if dtype == torch.float32 else 8e-3                        # bf16: dx is stored in bf16
        assert rel_err(d1, want_dx) < tol, (form, rel_err(d1, want_dx))
        if form == 'halo':
            border = buf.grad.clone()
            border[:, 1:1 + H, 1:1 + W, :] = 0
            assert not border.any()


# ---------------------------------------------------------------------------------------------------------------- softmax CE
def _ref_ce64(z, y, w, mean):
    """reference formula in float64: -sum(onehot * log_softmax(z), 1) * w, mean over rows (or sum); and d loss / d z"""
    z = z.double().cpu()
    y = y.reshape(-1).long().cpu()
    R, Cc = z.shape
    w = torch.ones(R, dtype=torch.float64) if w is None else w.double().cpu()
    lsm = torch.log_softmax(z, 1)
    onehot = torch.zeros(R, Cc, dtype=torch.float64)
    onehot[torch.arange(R), y] = 1
    rows = -(onehot * lsm).sum(1) * w
    loss = rows.mean() if mean else rows.sum()
    grad = (lsm.exp() - onehot) * w[:, None] / (R if mean else 1)
    return loss, grad


def _logits(R, Cc, gen):
    z = torch.randn(R, Cc, generator=gen) * 4
    if R > 1:
        z[0] = (torch.rand(Cc, generator=gen) * 2 - 1) * 3e4                 # logits up to +-3e4
        z[-1, ::3] = 3e4
    return z


@pytest.mark.parametrize('Cc,R', list(itertools.product([1, 2, 21, 1000, 1001, 4097], [1, 7, 256])))
def test_softmax_ce_against_float64(Cc, R):
    from fastvision_amd.loss import CrossEntropyLoss
    gen = torch.Generator().manual_seed(Cc * 31 + R)
    z = _logits(R, Cc, gen)
    y = torch.randint(0, Cc, (R,), generator=gen)
    wts = torch.rand(R, generator=gen) + 0.25
    for mean, w, form in itertools.product((True, False), (None, wts), ('i64', 'i64_col', 'f32_col')):
        lab = {'i64': y, 'i64_col': y.view(-1, 1), 'f32_col': y.float().view(-1, 1)}[form]
        zd = z.to(DEV).requires_grad_(True)
        loss = CrossEntropyLoss('mean' if mean else 'sum')(zd, lab.to(DEV), None if w is None else w.to(DEV))
        loss.backward()
        want, want_g = _ref_ce64(z, y, w, mean)
        got = loss.detach().double().cpu()
        assert loss.shape == () and abs(got - want) <= 1e-5 * abs(want) + 1e-30, (mean, w is None, form, got.item(), want.item())
        assert (zd.grad.double().cpu() - want_g).abs().max().item() <= 1e-6, (mean, w is None, form)


def test_softmax_ce_bad_label_gives_nan_and_leaves_other_rows_alone():
    from fastvision_amd.loss import CrossEntropyLoss
    gen = torch.Generator().manual_seed(9)
    R, Cc = 7, 21
    z = torch.randn(R, Cc, generator=gen)
    y = torch.randint(0, Cc, (R,), generator=gen)
    _, want_g = _ref_ce64(z, y, None, True)
    for bad_row, bad in ((2, Cc), (5, -1), (0, 2.5)):
        lab = y.float() if isinstance(bad, float) else y.clone()
        lab[bad_row] = bad
        zd = z.to(DEV).requires_grad_(True)
        loss = CrossEntropyLoss()(zd, lab.to(DEV))
        loss.backward()
        assert torch.isnan(loss).item(), bad
        g = zd.grad.double().cpu()
        assert torch.isnan(g[bad_row]).all()
        keep = [r for r in range(R) if r != bad_row]
        assert (g[keep] - want_g[keep]).abs().max().item() <= 1e-6


def test_softmax_ce_refuses_labels_or_weights_on_another_device():
    """labels straight from a CPU loader: a RuntimeError before anything is launched (the kernel reads raw pointers), as torch's own
    ops raise for mixed devices; the same call with the labels moved gives the right loss."""
    from fastvision_amd.loss import CrossEntropyLoss
    gen = torch.Generator().manual_seed(12)
    z = torch.randn(5, 7, generator=gen)
    y = torch.randint(0, 7, (5,), generator=gen)
    w = torch.rand(5, generator=gen)
    zd = z.to(DEV).requires_grad_(True)
    with pytest.raises(RuntimeError, match='y_true is on cpu'):
        CrossEntropyLoss()(zd, y)
    with pytest.raises(RuntimeError, match='y_true is on cpu'):
        CrossEntropyLoss()(zd, y.float().view(-1, 1))
    with pytest.raises(RuntimeError, match='weights is on cpu'):
        CrossEntropyLoss()(zd, y.to(DEV), w)
    loss = CrossEntropyLoss()(zd, y.to(DEV), w.to(DEV))
    want, _ = _ref_ce64(z, y, w, True)
    assert abs(loss.item() - want.item()) <= 1e-5 * abs(want.item())


def test_softmax_ce_value_only_under_no_grad_and_weights_stay_constants():
    from fastvision_amd.loss import CrossEntropyLoss
    gen = torch.Generator().manual_seed(13)
    z = torch.randn(6, 9, generator=gen)
    y = torch.randint(0, 9, (6,), generator=gen)
    w = torch.rand(6, generator=gen)
    zd = z.to(DEV).requires_grad_(True)
    with torch.no_grad():
        loss = CrossEntropyLoss('sum')(zd, y.to(DEV), w.to(DEV))
    assert not loss.requires_grad
    want, _ = _ref_ce64(z, y, w, False)
    assert abs(loss.item() - want.item()) <= 1e-5 * abs(want.item())
    with pytest.raises(RuntimeError, match='weights'):
        CrossEntropyLoss()(zd, y.to(DEV), w.to(DEV).requires_grad_(True))


# ---------------------------------------------------------------------------------------------------------------- accuracy
def test_accuracy_against_torch_argmax():
    from fastvision_amd.metrics import Accuracy
    gen = torch.Generator().manual_seed(4)
    R, Cc = 301, 1000
    z = torch.randn(R, Cc, generator=gen)
    z[1] = 0.25                                      # all equal: index 0
    z[2, 10] = z[2, 500] = 50.                       # tie: the first
    z[3, 7] = float('nan')                           # a NaN is the maximum
    z[4, 900] = z[4, 30] = float('nan')              # the first NaN wins
    z[5] = float('nan')
    z[6, -1] = 1e30
    arg = torch.argmax(z, 1)
    y = torch.randint(0, Cc, (R,), generator=gen)
    y[: R // 2] = arg[: R // 2]                      # about half right
    y[1:7] = arg[1:7]
    y[7] = -3                                        # out of range: never right
    acc = Accuracy()
    for dt in (torch.float32, torch.bfloat16):
        zz = z.to(dt)
        ref_arg = torch.argmax(zz.float(), 1)
        for lab in (y, y.float()):
            want = (ref_arg == lab.long()).float().sum(0, keepdim=True) / R
            got = acc(zz.to(DEV), lab.to(DEV))
            assert got.device.type == 'cuda' and got.shape == (1,) and got.dtype == torch.float32
            assert torch.equal(got.cpu(), want), (dt, got.item(), want.item())
    with pytest.raises(RuntimeError):
        acc(z.to(DEV), y.view(-1, 1).to(DEV))


# ---------------------------------------------------------------------------------------------------------------- whole model
GRADS = ['conv0.conv.weight', 'res3.3.conv2.conv.weight', 'res5.3.conv2.bn.weight']


def _models(num_classes, seed=20220504):
    from fastvision_amd.classfication.models import darknet53
    from oracle.model import Backbone
    torch.manual_seed(seed)
    net = darknet53(num_classes=num_classes)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    bb = Backbone()
    bb.load_state_dict({k: v for k, v in sd.items() if not k.startswith('fc.')})
    fc = nn.Linear(1024, num_classes)
    fc.load_state_dict({'weight': sd['fc.weight'], 'bias': sd['fc.bias']})
    return net.to(DEV), bb, fc


def _oracle_step(bb, fc, images, labels):
    z = fc(torch.flatten(F.adaptive_avg_pool2d(bb(images)[0], (1, 1)), 1))
    loss = -torch.sum(F.one_hot(labels, z.shape[1]).float() * F.log_softmax(z, -1), 1).mean()
    loss.backward()
    return z.detach(), loss.detach()


@pytest.mark.parametrize('S,dtype', [(224, torch.float32), (256, torch.float32), (224, torch.bfloat16)])
def test_darknet53_classifier_step_against_oracle(S, dtype):
    import fastvision_amd
    from fastvision_amd.loss import CrossEntropyLoss
    B = 4
    gen = torch.Generator().manual_seed(S)
    images = torch.randn(B, 3, S, S, generator=gen)
    labels = torch.randint(0, 1000, (B,), generator=gen)
    net, bb, fc = _models(1000)
    net.train(); bb.train(); fc.train()
    rz, rloss = _oracle_step(bb, fc, images, labels)
    with fastvision_amd.compute_dtype(dtype):
        z = net(images.to(DEV))
        loss = CrossEntropyLoss()(z, labels.to(DEV))
        loss.backward()
    torch.cuda.synchronize()
    assert z.dtype == torch.float32 and tuple(z.shape) == (B, 1000)
    ref = dict(bb.named_parameters())
    ref.update({'fc.weight': fc.weight, 'fc.bias': fc.bias})
    got = dict(net.named_parameters())
    names = ['fc.weight', 'fc.bias'] + GRADS
    zerr, lrel = rel_err(z, rz), abs(loss.item() - rloss.item()) / abs(rloss.item())
    gerr = {k: rel_err(got[k].grad, ref[k].grad) for k in names}
    grel = {k: abs(got[k].grad.double().norm().item() - ref[k].grad.double().norm().item()) / ref[k].grad.double().norm().item() for k in names}
    cos = {k: F.cosine_similarity(got[k].grad.double().cpu().flatten(), ref[k].grad.double().flatten(), 0).item() for k in names}
    print(f'darknet53 top {dtype} {S}px: logits {zerr:.2e} loss {lrel:.2e} grads {gerr} norm-rel {grel} cos {cos}')
    if dtype == torch.float32:
        assert zerr < 1e-3 and lrel < 1e-3
        assert max(gerr.values()) < 1e-3, gerr
    else:
        # bf16 gates, the test_gpu_fullsize.py bars: heads 1.3e-1 of the scale, loss 1e-3, gradient norms 1.2e-1, cosine 0.96
        assert zerr < 1.3e-1 and lrel < 1e-3
        assert max(grel.values()) < 1.2e-1, grel
        assert min(cos.values()) > 0.96, cos


@pytest.mark.parametrize('nc', [10, 1])
def test_darknet53_few_classes_and_eval_mode(nc):
    import fastvision_amd
    B, S = 3, 96
    gen = torch.Generator().manual_seed(10)
    images = torch.randn(B, 3, S, S, generator=gen)
    labels = torch.randint(0, nc, (B,), generator=gen)
    net, bb, fc = _models(nc, seed=7)
    with fastvision_amd.compute_dtype(torch.float32):
        net.train(); bb.train()
        rz, _ = _oracle_step(bb, fc, images, labels)
        from fastvision_amd.loss import CrossEntropyLoss
        z = net(images.to(DEV))
        CrossEntropyLoss()(z, labels.to(DEV)).backward()
        assert tuple(z.shape) == (B, nc) and rel_err(z, rz) < 1e-3
        assert rel_err(net.fc.weight.grad, fc.weight.grad) < 1e-3 and rel_err(net.fc.bias.grad, fc.bias.grad) < 1e-3
        net.eval(); bb.eval()
        with torch.no_grad():
            ze = net(images.to(DEV))
            re = fc(torch.flatten(F.adaptive_avg_pool2d(bb(images)[0], (1, 1)), 1))
        assert not ze.requires_grad and rel_err(ze, re) < 1e-3


def _train_parts(num_classes=10, seed=3):
    from fastvision_amd import FusedSGD
    from fastvision_amd.classfication.models import darknet53
    from fastvision_amd.loss import CrossEntropyLoss
    torch.manual_seed(seed)
    net = darknet53(num_classes=num_classes).to(DEV).train()
    opt = FusedSGD(net.parameters(), lr=0.01, momentum=0.9, nesterov=True, weight_decay=5e-4, capturable=True)
    return net, CrossEntropyLoss(), opt


def _step(net, crit, opt, images, labels):
    pred = net(images)
    opt.zero_grad(set_to_none=True)
    loss = crit(pred, labels)
    loss.backward()
    opt.step()
    return loss.detach().clone()


def test_top_runs_without_aten_pooling_linear_or_softmax(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError('ATen op in the classifier top')
    net, crit, opt = _train_parts()
    gen = torch.Generator().manual_seed(1)
    images, labels = torch.randn(2, 3, 64, 64, generator=gen).to(DEV), torch.tensor([3, 7], device=DEV)
    for name in ('adaptive_avg_pool2d', 'linear', 'log_softmax'):
        monkeypatch.setattr(F, name, refuse)
    monkeypatch.setattr(torch.Tensor, 'scatter_', refuse)
    loss = _step(net, crit, opt, images, labels)
    monkeypatch.undo()
    assert torch.isfinite(loss).item()


def test_train_step_and_accuracy_do_not_synchronise_the_host():
    from fastvision_amd.metrics import Accuracy
    net, crit, opt = _train_parts()
    gen = torch.Generator().manual_seed(2)
    images, labels = torch.randn(4, 3, 64, 64, generator=gen).to(DEV), torch.tensor([1, 2, 3, 4], device=DEV)
    acc = Accuracy()
    _step(net, crit, opt, images, labels)                   # warm-up: packed weights, optimizer tables
    acc(net(images).detach(), labels)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        pred = net(images)
        opt.zero_grad(set_to_none=True)
        loss = crit(pred, labels)
        loss.backward()
        opt.step()
        a = acc(pred.detach(), labels)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert torch.isfinite(loss).item() and 0.0 <= a.item() <= 1.0


def test_graphed_step_with_float_labels_is_bit_identical_with_eager():
    from fastvision_amd import ops
    from fastvision_amd.graphs import GraphedTrainStep
    gen = torch.Generator().manual_seed(5)
    batches = [(torch.randn(4, 3, 64, 64, generator=gen), torch.randint(0, 10, (4, 1), generator=gen).float()) for _ in range(3)]
    prev = ops.set_wgrad_side_stream(False)                 # the single-stream capture equals the eager single-stream step
    try:
        net, crit, opt = _train_parts()
        want = [_step(net, crit, opt, im.to(DEV), lab.to(DEV)) for im, lab in batches]
        torch.cuda.synchronize()
    finally:
        ops.set_wgrad_side_stream(prev)
    net2, crit2, opt2 = _train_parts()
    step = GraphedTrainStep(net2, lambda p, t: crit2(p, t), opt2, batches[0][0].to(DEV), batches[0][1].to(DEV))
    got = [step(im.to(DEV), lab.to(DEV)).clone() for im, lab in batches]
    torch.cuda.synchronize()
    for a, b in zip(got, want):
        assert torch.equal(a, b), (a, b)
    for (k, p), q in zip(net.state_dict().items(), net2.state_dict().values()):
        assert torch.equal(p, q), k
    for p, q in zip(net.parameters(), net2.parameters()):
        assert torch.equal(opt.state[p]['momentum_buffer'], opt2.state[q]['momentum_buffer'])


def test_fit_trains_the_classifier():
    from fastvision_amd import FusedSGD
    from fastvision_amd.classfication.models import darknet53
    from fastvision_amd.loss import CrossEntropyLoss
    from fastvision_amd.utils import Fit
    gen = torch.Generator().manual_seed(11)
    labels = torch.arange(16) % 4
    images = torch.randn(16, 3, 64, 64, generator=gen) * 0.5
    for i in range(16):                                     # a learnable set: the class shows in the colour
        images[i, labels[i] % 3] += 1.0 + float(labels[i] // 3)
    torch.manual_seed(0)
    net = darknet53(num_classes=10).to(DEV)
    opt = FusedSGD(net.parameters(), lr=0.01, momentum=0.9, nesterov=True, weight_decay=5e-4)
    fit = Fit(net, torch.device(DEV), opt, None, CrossEntropyLoss(), end_epoch=20, train_loader=[(images, labels)], save_last=None)
    fit.run_epoches()
    losses = [h[0] for h in fit.history]
    print('fit losses', [round(l, 4) for l in losses])
    assert len(losses) == 20 and np.isfinite(losses).all()
    assert losses[-1] < 0.5 * losses[0], losses
