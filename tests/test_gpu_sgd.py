"""FusedSGD on the GPU (fva_sgd_clip_coef + fva_sgd_step) against torch.optim.SGD and the Faster R-CNN demo's clip_gradient
(demos/faster_rcnn/cfg/_fit.py:6-17): the update over a grid of options and sizes, device-side clipping in both regimes and for
non-finite norms, no host synchronisation, checkpoint exchange with torch's SGD, HIP-graph capture, and three demo training steps."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BIG = (1 << 24) + 5


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


class Grid:
    """Three parameter groups (sizes 1, 3, 1023, 2^24 + 5, a view at an odd storage offset, one parameter that never gets a
    gradient), with a fixed sequence of gradients (the view's gradient is a view at another odd offset)."""

    def __init__(self, wd, device, seed=0):
        g = torch.Generator().manual_seed(seed)
        base = torch.randn(1100, generator=g)
        self.sizes = [1, 3, 1023, BIG]
        vals = [torch.randn(n, generator=g) for n in self.sizes]
        self.ps = [torch.nn.Parameter(v.clone().to(device)) for v in vals]
        self.view = torch.nn.Parameter(base.to(device)[5:5 + 1000])               # storage offset 5: no 16-byte alignment
        self.none = torch.nn.Parameter(torch.randn(7, generator=g).to(device))
        self.groups = [{'params': [self.ps[0], self.ps[1]], 'lr': 0.1, 'weight_decay': wd},
                       {'params': [self.ps[2], self.view, self.none], 'lr': 0.03, 'weight_decay': 0.0},
                       {'params': [self.ps[3]], 'lr': 0.01, 'weight_decay': 1e-3 if wd else 0.0}]
        self.device = device
        self.grads = [[torch.randn(n, generator=g) for n in self.sizes + [1003]] for _ in range(3)]

    def all(self):
        return self.ps + [self.view]

    def set_grads(self, k):
        gs = self.grads[k % 3]
        s = 1.0 + 0.05 * k
        for p, gv in zip(self.ps, gs):
            p.grad = (gv * s).to(self.device)
        self.view.grad = (gs[-1] * s).to(self.device)[3:3 + 1000]
        self.none.grad = None


CONFIGS = [(m, n, d, wd) for (m, n, d), wd in itertools.product([(0.0, False, 0.0), (0.937, False, 0.0), (0.937, True, 0.0), (0.937, False, 0.1)],
                                                                 [0.0, 5e-4])]


@pytest.mark.parametrize('momentum,nesterov,dampening,wd', CONFIGS)
def test_update_matches_torch_sgd(momentum, nesterov, dampening, wd):
    from fastvision_amd import FusedSGD
    gpu, cpu = Grid(wd, DEV), Grid(wd, 'cpu')
    assert gpu.view.storage_offset() == 5
    kw = dict(momentum=momentum, dampening=dampening, nesterov=nesterov)
    opt = FusedSGD(gpu.groups, lr=0.1, **kw)
    ref = torch.optim.SGD(cpu.groups, lr=0.1, foreach=False, **kw)
    none0 = gpu.none.detach().clone()
    for k in range(20):
        gpu.set_grads(k)
        cpu.set_grads(k)
        opt.step()
        ref.step()
    torch.cuda.synchronize()
    assert gpu.view.grad.storage_offset() == 3
    for i, (a, b) in enumerate(zip(gpu.all(), cpu.all())):
        assert rel_err(a, b) <= 2e-6, (i, rel_err(a, b))
        if momentum:
            assert rel_err(opt.state[a]['momentum_buffer'], ref.state[b]['momentum_buffer']) <= 2e-6, i
        else:
            assert 'momentum_buffer' not in opt.state.get(a, {}) and not ref.state.get(b)
    assert torch.equal(gpu.none.detach(), none0) and not opt.state.get(gpu.none)      # never had a gradient: untouched, no state


# ---------------------------------------------------------------------------------------------------------------- clipping
class Params(torch.nn.Module):
    def __init__(self, seed=1, sizes=(5, 1023, 4096 * 64 + 3, 70000)):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.ws = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(n, generator=g)) for n in sizes])
        self.gs = [[torch.randn(n, generator=g) for n in sizes] for _ in range(3)]

    def set_grads(self, k, scale):
        for p, gv in zip(self.ws, self.gs[k % 3]):
            p.grad = (gv * scale * (1 + 0.1 * k)).to(p.device)


def run_clipped(scale, fused, clip=10., steps=5, mom=0.937, nesterov=True):
    from fastvision_amd import FusedSGD
    from fastvision_amd.demos.faster_rcnn.cfg._fit import clip_gradient
    m = Params().to(DEV)
    norms = []
    if fused:
        opt = FusedSGD(m.parameters(), lr=0.01, momentum=mom, nesterov=nesterov, clip_norm=clip)
    else:
        opt = torch.optim.SGD(m.parameters(), lr=0.01, momentum=mom, nesterov=nesterov, foreach=False)
    for k in range(steps):
        m.set_grads(k, scale)
        want = torch.linalg.vector_norm(torch.cat([p.grad.double().flatten() for p in m.parameters()])).item()
        if fused:
            opt.step()
            if clip is not None:
                norms.append((opt.last_grad_norm.clone(), want))
        else:
            if clip is not None:
                clip_gradient(m, clip)
            opt.step()
    torch.cuda.synchronize()
    return m, opt, norms


@pytest.mark.parametrize('scale', [1.0, 1e-3])            # global norm far above 10 / below 10
def test_clipping_matches_clip_gradient_then_torch_sgd(scale):
    got, opt, norms = run_clipped(scale, True)
    want, _, _ = run_clipped(scale, False)
    for a, b in zip(got.parameters(), want.parameters()):
        assert rel_err(a, b) <= 2e-6, rel_err(a, b)
    for n, w in norms:
        assert n.dtype == torch.float32 and n.device.type == 'cuda' and n.dim() == 0
        assert abs(n.item() - w) <= 1e-6 * w, (n.item(), w)
    assert (norms[0][1] > 10) == (scale == 1.0)


def test_unit_coefficient_is_bit_identical_to_no_clipping():
    a, opt, norms = run_clipped(1e-3, True)
    assert all(w < 10 for _, w in norms) and opt._clip_out[1].item() == 1.0
    b, _, _ = run_clipped(1e-3, True, clip=None)
    for x, y in zip(a.parameters(), b.parameters()):
        assert torch.equal(x, y)


def test_two_runs_are_bit_identical():
    a, oa, na = run_clipped(1.0, True)
    b, ob, nb = run_clipped(1.0, True)
    for x, y in zip(a.parameters(), b.parameters()):
        assert torch.equal(x, y)
    for (x, _), (y, _) in zip(na, nb):
        assert torch.equal(x, y)
    for x, y in zip(a.parameters(), b.parameters()):
        assert torch.equal(oa.state[x]['momentum_buffer'], ob.state[y]['momentum_buffer'])


def test_non_finite_norms_behave_like_the_reference():
    from fastvision_amd import FusedSGD
    from fastvision_amd.demos.faster_rcnn.cfg._fit import clip_gradient
    # a NaN gradient: the norm is NaN, max(nan, 10) is nan, every parameter becomes NaN (reference and FusedSGD alike)
    for fused in (True, False):
        m = Params().to(DEV)
        m.set_grads(0, 1.0)
        m.ws[1].grad[17] = float('nan')
        if fused:
            opt = FusedSGD(m.parameters(), lr=0.01, momentum=0.937, nesterov=True, clip_norm=10.)
            opt.step()
            assert torch.isnan(opt.last_grad_norm).item() and torch.isnan(opt._clip_out[1]).item()
        else:
            clip_gradient(m, 10.)
            torch.optim.SGD(m.parameters(), lr=0.01, momentum=0.937, nesterov=True).step()
        assert all(torch.isnan(p).all().item() for p in m.parameters()), fused
    # an infinite norm from finite gradients (fp32 overflow of the norm): coefficient 0, nothing moves
    m = Params().to(DEV)
    for p in m.parameters():
        p.grad = torch.full_like(p, 3e38)
    p0 = [p.detach().clone() for p in m.parameters()]
    opt = FusedSGD(m.parameters(), lr=0.01, clip_norm=10.)
    opt.step()
    assert torch.isinf(opt.last_grad_norm).item() and opt._clip_out[1].item() == 0.0
    for p, q in zip(m.parameters(), p0):
        assert torch.equal(p.detach(), q)


def test_clipped_step_does_not_synchronise_the_host():
    from fastvision_amd import FusedSGD
    m = Params().to(DEV)
    opt = FusedSGD(m.parameters(), lr=0.01, momentum=0.937, nesterov=True, weight_decay=5e-4, clip_norm=10.)
    m.set_grads(0, 1.0)
    opt.step()                                                     # warm-up: buffers, tables
    torch.cuda.synchronize()
    m.set_grads(1, 1.0)
    torch.cuda.set_sync_debug_mode('error')
    try:
        opt.step()
        opt.param_groups[0]['lr'] = 0.005                          # a schedule step: the hyper-parameter table is re-uploaded
        opt.step()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- checkpoints
@pytest.mark.parametrize('first_fused', [True, False])
def test_checkpoints_exchange_with_torch_sgd(first_fused):
    from fastvision_amd import FusedSGD
    kw = dict(lr=0.01, momentum=0.937, nesterov=True, weight_decay=5e-4)
    ref = Params().to(DEV)
    ref_opt = torch.optim.SGD(ref.parameters(), foreach=False, **kw)
    m = Params().to(DEV)
    make = [lambda: FusedSGD(m.parameters(), **kw), lambda: torch.optim.SGD(m.parameters(), foreach=False, **kw)]
    opt = make[0 if first_fused else 1]()
    for k in range(7):
        if k == 3:
            sd = opt.state_dict()
            opt = make[1 if first_fused else 0]()
            opt.load_state_dict(sd)
        m.set_grads(k, 1.0)
        ref.set_grads(k, 1.0)
        opt.step()
        ref_opt.step()
    torch.cuda.synchronize()
    for a, b in zip(m.parameters(), ref.parameters()):
        assert rel_err(a, b) <= 2e-6
        assert rel_err(opt.state[a]['momentum_buffer'], ref_opt.state[b]['momentum_buffer']) <= 2e-6


# ---------------------------------------------------------------------------------------------------------------- graphs
LRS = [0.01, 0.01, 0.004, 0.004, 0.002]


def _capturable():
    from fastvision_amd import FusedSGD
    m = Params().to(DEV)
    return m, FusedSGD(m.parameters(), lr=0.01, momentum=0.937, nesterov=True, weight_decay=5e-4, clip_norm=10., capturable=True)


def _fwd_bwd(m):
    x = [torch.linspace(-2, 2, p.numel(), device=DEV) for p in m.ws]
    loss = sum(((p * xi) ** 2).sum() * 0.5 + torch.sin(p).sum() for p, xi in zip(m.ws, x))
    loss.backward()


def _eager(m, opt):
    opt.zero_grad(set_to_none=True)
    _fwd_bwd(m)
    opt.step()


def _capture(m, opt):
    """Capture backward + step (after the eager step the capture needs)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        opt.zero_grad(set_to_none=True)
    torch.cuda.current_stream().wait_stream(side)
    keep = opt.begin_capture()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _fwd_bwd(m)
        opt.step()
    assert keep
    return graph, keep


def _replay(graph, opt, lr):
    opt.param_groups[0]['lr'] = lr
    opt.sync_lr()
    graph.replay()


def _assert_same(a, oa, b, ob):
    torch.cuda.synchronize()
    for p, q in zip(a.parameters(), b.parameters()):
        assert torch.equal(p, q)
        assert torch.equal(oa.state[p]['momentum_buffer'], ob.state[q]['momentum_buffer'])
    assert torch.equal(oa.last_grad_norm, ob.last_grad_norm)


def test_captured_backward_and_step_replays_like_eager_steps():
    a, oa = _capturable()
    b, ob = _capturable()
    _eager(a, oa)
    _eager(b, ob)                       # the eager step capture needs (buffers, tables, staging)
    for lr in LRS:
        oa.param_groups[0]['lr'] = lr
        _eager(a, oa)
    graph, keep = _capture(b, ob)
    for lr in LRS:
        _replay(graph, ob, lr)
    _assert_same(a, oa, b, ob)


def test_restore_to_a_pre_step_snapshot_after_capture_behaves_like_a_fresh_optimizer():
    """restore_train_state to a snapshot taken before the first step, AFTER a graph was captured on an optimizer whose buffers had
    history: the buffers are fresh again, so the next update -- a replay or an eager step -- must initialise them (torch's
    clone(grad)) exactly once, and every later update must keep their history."""
    from fastvision_amd.graphs import restore_train_state, snapshot_train_state
    a, oa = _capturable()
    for lr in LRS:                      # the reference: a fresh optimizer, five eager steps
        oa.param_groups[0]['lr'] = lr
        _eager(a, oa)
    b, ob = _capturable()
    snap = snapshot_train_state(b, ob)  # no momentum buffers yet
    ob.param_groups[0]['lr'] = LRS[0]
    _eager(b, ob)
    _eager(b, ob)                       # buffers with history when the graph is captured
    graph, keep = _capture(b, ob)
    # (1) replays only
    restore_train_state(b, ob, snap)
    for lr in LRS:
        _replay(graph, ob, lr)
    _assert_same(a, oa, b, ob)
    # (2) an eager step first, then replays
    restore_train_state(b, ob, snap)
    ob.param_groups[0]['lr'] = LRS[0]
    _eager(b, ob)
    for lr in LRS[1:]:
        _replay(graph, ob, lr)
    _assert_same(a, oa, b, ob)
    # (3) replays first, then eager steps (the eager steps must not re-initialise the buffers)
    restore_train_state(b, ob, snap)
    for lr in LRS[:2]:
        _replay(graph, ob, lr)
    for lr in LRS[2:]:
        ob.param_groups[0]['lr'] = lr
        _eager(b, ob)
    _assert_same(a, oa, b, ob)


def test_clip_coefficient_uses_the_double_clip_value():
    """clip / max(norm, clip) as the reference's Python computes it, with the clip value kept in double (none of these clip values
    has an exact fp32 form; an fp32 clip would move the rounded coefficient by one ulp for some of them)."""
    from fastvision_amd import FusedSGD
    m = Params().to(DEV)
    for clip in (0.3, 0.7, 1.1, 2.3, 3.7, 5.9, 7.3, 0.13, 0.37, 0.51, 9.1, 4.3):
        m.set_grads(0, 1.0)
        opt = FusedSGD(m.parameters(), lr=0.0, clip_norm=clip)
        opt.step()
        norm = opt.last_grad_norm.item()
        assert norm > clip
        assert opt._clip_out[1].item() == float(np.float32(clip / max(norm, clip))), clip


def _yolo(seed=20220504):
    from fastvision_amd.classfication.models import darknet53
    from fastvision_amd.detection.head import yolov3head
    from fastvision_amd.detection.models import yolov3
    from fastvision_amd.detection.neck import yolov3neck
    from fastvision_amd.synthetic import coco_anchors_px
    torch.manual_seed(seed)
    m = yolov3(backbone=darknet53, neck=yolov3neck, head=yolov3head, anchors=coco_anchors_px(), num_anchors_per_level=[3, 3, 3],
               in_channels=3, num_classes=80, training=True)
    return m.to(DEV).train()


def test_graphed_train_step_with_fused_sgd_is_bit_identical_with_eager():
    import fastvision_amd
    from fastvision_amd import FusedSGD
    from fastvision_amd.graphs import GraphedTrainStep
    from fastvision_amd.loss import Yolov3Loss
    from fastvision_amd.synthetic import synthetic_batch
    batches = [synthetic_batch(2, 128, seed=s) for s in (1234, 7, 99)]
    cap = max(t.shape[0] for _, t in batches) + 5
    lrs = [1e-3, 1e-3, 3e-4, 3e-4]
    order = [0, 1, 2, 0]

    def make():
        net = _yolo()
        crit = Yolov3Loss(net, 0.5, 0.05, 1.0, 0.5)
        opt = FusedSGD(net.parameters(), lr=1e-3, momentum=0.937, nesterov=True, weight_decay=5e-4, clip_norm=10., capturable=True)
        return net, crit, opt

    def state_of(net, opt):
        out = {k: v.detach().clone() for k, v in net.state_dict().items()}
        for i, p in enumerate(net.parameters()):
            out[f'buf{i}'] = opt.state[p]['momentum_buffer'].clone()
        return out
    with fastvision_amd.compute_dtype(torch.float32):
        net, crit, opt = make()
        want = []
        for i, lr in zip(order, lrs):
            opt.param_groups[0]['lr'] = lr
            im, tg = batches[i]
            pred = net(im.to(DEV))
            opt.zero_grad()
            loss = crit(pred, tg.to(DEV))
            loss.backward()
            opt.step()
            want.append(loss.detach().clone())
        want_state = state_of(net, opt)
        torch.cuda.synchronize()

        net2, crit2, opt2 = make()
        im0, tg0 = batches[0]
        step = GraphedTrainStep(net2, lambda p, t: crit2(p, t), opt2, im0.to(DEV), tg0.to(DEV), max_targets=cap)
        got = []
        for i, lr in zip(order, lrs):
            opt2.param_groups[0]['lr'] = lr
            im, tg = batches[i]
            got.append(step(im.to(DEV), tg.to(DEV)).clone())
        got_state = state_of(net2, opt2)
        torch.cuda.synchronize()
    for a, b in zip(got, want):
        assert torch.equal(a, b), (a, b)
    for k in want_state:
        assert torch.equal(got_state[k], want_state[k]), k


# ---------------------------------------------------------------------------------------------------------------- Faster R-CNN
def test_faster_rcnn_train_steps_with_fused_sgd_match_clip_gradient_and_torch_sgd():
    """The small setup of test_gpu_faster.py::test_training_step_vs_cpu_oracle_other_seed_and_size, three _Train steps on the GPU:
    FusedSGD(clip_norm=10) against torch's SGD after clip_gradient (the demo's step), fp32."""
    import fastvision_amd
    from fastvision_amd import FusedSGD
    from fastvision_amd.demos.faster_rcnn.cfg import _fit
    from fastvision_amd.demos.faster_rcnn.models import Faster_Rcnn
    B, H, W, T, NC = 2, 112, 144, 5, 7
    g = torch.Generator().manual_seed(5)
    images = torch.rand(B, 3, H, W, generator=g)
    tb = torch.sort(torch.cat([torch.arange(B), torch.randint(0, B, (T - B,), generator=g)]))[0].float()
    wh = torch.exp(np.log(0.25) + (np.log(0.7) - np.log(0.25)) * torch.rand(T, 2, generator=g))
    xy = wh / 2 + (1 - wh) * torch.rand(T, 2, generator=g)
    targets = torch.cat([tb[:, None], torch.randint(0, NC, (T, 1), generator=g).float(), xy, wh], 1)
    base = torch.tensor([[45.3, 22.6], [90.5, 45.3], [32, 32], [64, 64], [22.6, 45.3], [45.3, 90.5]])

    def run(fused):
        torch.manual_seed(99)
        model = Faster_Rcnn(training=True, num_classes=NC, base_anchors=base, rpn_positives_per_image=12, rpn_negatives_per_image=20,
                            fast_positives_per_image=6, fast_negatives_per_image=10, fast_multi_reg_head=True)
        for m in model.modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = 0.0
        for m in model.backbone.modules():
            if isinstance(m, torch.nn.Conv2d):
                m.weight.data *= 1.7
        model = model.to(DEV)
        if fused:
            opt = FusedSGD(model.parameters(), lr=1e-3, momentum=0.937, nesterov=True, clip_norm=_fit.CLIP_NORM)
        else:
            opt = torch.optim.SGD(model.parameters(), lr=1e-3, momentum=0.937, nesterov=True)
        logged = []
        torch.manual_seed(7)
        with fastvision_amd.compute_dtype(torch.float32):
            _fit._Train(model, [(images, targets)] * 3, opt, log=lambda *v: logged.append(v))
        torch.cuda.synchronize()
        return model, np.array(logged)
    got, gl = run(True)
    want, wl = run(False)
    print('losses', gl, 'reference', wl)
    assert gl.shape == (3, 5)
    np.testing.assert_allclose(gl[:, 1:], wl[:, 1:], rtol=1e-5)
    for (k, a), (_, b) in zip(got.named_parameters(), want.named_parameters()):
        assert rel_err(a, b) <= 1e-5, (k, rel_err(a, b))
