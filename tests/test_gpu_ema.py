"""ModelEMA on the GPU (fva_ema_update): one update element by element against float64 at the chunk seams and at unaligned addresses,
the ramp of the device counter, fifty updates against the float64 recurrence, the averaged model evaluating what it holds (packed
weights and eval BatchNorm coefficients rebuilt), training left untouched, no host synchronisation, the captured training step,
checkpoints, and the fit loop.  The restatement and the bound are in tests/ema_restatement.py (pinned by tests/test_ema_cpu.py)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import ema_restatement as er

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
PAD = 64                                     # sentinel elements on each side of an EMA tensor (256 B of fp32: keeps slices 16-byte aligned)
F_SENT, I_SENT = 12288.0, 77                 # (exact in bf16 too)


# ---------------------------------------------------------------------------------------------------------------- helpers
def values(n, gen):
    """+-[1, 2) * 2^[-10, 4], about 2 % exact zeros: no denormals, fourteen binades."""
    v = (1.0 + torch.rand(n, generator=gen)) * torch.exp2(torch.randint(-10, 5, (n,), generator=gen).float())
    v = v * (torch.randint(0, 2, (n,), generator=gen).float() * 2 - 1)
    v[torch.rand(n, generator=gen) < 0.02] = 0.0
    return v.float()


def guarded(vals, shift=0):
    """``vals`` on the device as a slice of a larger buffer filled with sentinels; ``shift`` moves the slice off 16-byte alignment."""
    sent = F_SENT if vals.dtype.is_floating_point else I_SENT
    n = vals.numel()
    buf = torch.full((n + 2 * PAD,), sent, dtype=vals.dtype) if vals.dtype != torch.bool else torch.ones(n + 2 * PAD, dtype=torch.bool)
    buf = buf.to(DEV)
    view = buf[PAD + shift:PAD + shift + n]
    view.copy_(vals.reshape(-1).to(DEV))
    return buf, view.reshape(vals.shape)


def sentinels_intact(buf, shift, n):
    sent = True if buf.dtype == torch.bool else (F_SENT if buf.dtype.is_floating_point else I_SENT)
    return bool((buf[:PAD + shift] == sent).all()) and bool((buf[PAD + shift + n:] == sent).all())


def launch(pairs, decay, tau, state):
    from fastvision_amd import _lib
    from fastvision_amd.ema import build_tables
    from fastvision_amd.ops import _stream
    tab, n, chunks, nchunks, keep = build_tables(pairs)
    _lib.call('fva_ema_update', C.c_void_p(tab.data_ptr()), n, C.c_void_p(chunks.data_ptr()), nchunks, decay, tau,
              C.c_void_p(state.data_ptr()), _stream())
    torch.cuda.synchronize()
    return n, nchunks


def chunk_elems():
    from fastvision_amd import _lib
    return _lib.call('fva_ema_chunk_elems')


def check_step(name, got, ref, bound):
    err = np.abs(got.astype(np.float64) - ref)
    worst = float((err / np.where(bound > 0, bound, 1.0)).max()) if err.size else 0.0
    print(f'{name}: n={err.size} largest error / bound {worst:.5f}, elements with bound 0: {int((bound == 0).sum())}')
    assert np.array_equal(got[bound == 0].astype(np.float64), ref[bound == 0]), name
    assert (err <= bound).all(), (name, worst)


# ---------------------------------------------------------------------------------------------------------------- 1: one update
@pytest.mark.parametrize('decay,tau,updates', [(0.9999, 2000.0, 0), (0.9999, 2000.0, 99999), (0.5, 0.0, 3)])
def test_one_update_element_by_element(decay, tau, updates):
    Cn = chunk_elems()
    gen = torch.Generator().manual_seed(20240607 + updates)
    sizes = [1, 3, 1023, Cn - 1, Cn, Cn + 1, 2 * Cn + 5]
    cases = []                                   # (name, e values, p values, shift of the EMA slice, offset of the model view)
    for n in sizes:
        cases.append((f'n{n}', values(n, gen), values(n, gen), 0, 0))
    cases.append(('model_view_at_5', values(Cn + 1, gen), values(Cn + 1, gen), 0, 5))
    cases.append(('ema_view_at_1', values(1023 + Cn, gen), values(1023 + Cn, gen), 1, 0))
    same = values(2 * Cn + 5, gen)
    cases.append(('p_equals_e', same, same.clone(), 0, 0))
    held, pairs = [], []
    for name, e, p, shift, off in cases:
        buf, ev = guarded(e, shift)
        base = torch.cat([torch.full((off,), -1.0), p]).to(DEV)
        pv = base[off:]
        assert pv.storage_offset() == off and ev.data_ptr() % 16 == 4 * shift % 16
        held.append((name, e, p, shift, buf, ev, pv))
        pairs.append((name, ev, pv))
    raw = [('count', torch.tensor(41, dtype=torch.int64), torch.tensor(1234567890123, dtype=torch.int64), 0),
           ('bytes', torch.tensor([1, 2, 3], dtype=torch.uint8), torch.tensor([200, 0, 255], dtype=torch.uint8), 7),
           ('flags', torch.tensor([True, False, True, False, False]), torch.tensor([False, False, True, True, True]), 3),
           ('wide', torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64), torch.tensor([math.pi, -1e300, 5e-324], dtype=torch.float64), 1),
           # beyond the issue's four: more than one chunk of bytes at aligned addresses (the 16-byte copy path and its 6-byte tail)
           ('half', torch.zeros(2 * Cn + 3, dtype=torch.bfloat16), values(2 * Cn + 3, gen).to(torch.bfloat16), 0)]
    raw_held = []
    for name, e, p, shift in raw:
        buf, ev = guarded(e, shift)
        pv = p.to(DEV)
        raw_held.append((name, e, shift, buf, ev, pv))
        pairs.append((name, ev, pv))
    state = torch.tensor([float(updates), 0.0], dtype=torch.float64, device=DEV)
    n, nchunks = launch(pairs, decay, tau, state)
    assert n == len(pairs)
    assert nchunks == sum(-(-c[1].numel() // Cn) for c in cases) + sum(-(-r[1].numel() * r[1].element_size() // (4 * Cn)) for r in raw)
    k, w = state.cpu().tolist()
    assert k == updates + 1 and abs(w - er.weight(updates + 1, decay, tau)) <= 2.0 ** -50
    wf = er.w32(w)
    for name, e, p, shift, buf, ev, pv in held:
        ref = er.step(e.numpy(), p.numpy(), wf)
        check_step(name, ev.cpu().numpy(), ref, er.step_bound(ref, e.numpy(), p.numpy(), wf))
        assert sentinels_intact(buf, shift, e.numel()), name
        assert torch.equal(pv.cpu(), p), name                       # the model side is only read
    for name, e, shift, buf, ev, pv in raw_held:
        assert torch.equal(ev, pv), name
        assert sentinels_intact(buf, shift, e.numel()), name


# ---------------------------------------------------------------------------------------------------------------- 2: the ramp
def small_net(seed=0):
    torch.manual_seed(seed)
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3), torch.nn.BatchNorm2d(8), torch.nn.Conv2d(8, 8, 1))
    for b in net[1].buffers():
        if b.dtype.is_floating_point:
            b.uniform_(0.5, 1.5)
    net[1].num_batches_tracked.fill_(11)
    return net.to(DEV)


@pytest.mark.parametrize('updates,decay,tau', [(0, 0.9999, 2000.0), (1, 0.9999, 2000.0), (1999, 0.9999, 2000.0), (99999, 0.9999, 2000.0),
                                               (0, 0.9999, 0.0), (7, 0.9, 0.0)])
def test_ramp_of_the_device_counter(updates, decay, tau):
    from fastvision_amd import ModelEMA
    net = small_net()
    ema = ModelEMA(net, decay=decay, tau=tau, updates=updates)
    assert ema.updates == updates
    ema.update(net)
    k, w = ema._state.cpu().tolist()
    want = 1 - decay * (1 - math.exp(-(updates + 1) / tau)) if tau > 0 else 1 - decay
    print(f'updates {updates} tau {tau}: state[1] - python = {w - want:.3e} (limit {2.0 ** -50:.3e})')
    assert k == float(updates + 1) and ema.updates == updates + 1
    assert abs(w - want) <= 2.0 ** -50


# ---------------------------------------------------------------------------------------------------------------- 3: fifty updates
def test_fifty_updates_follow_the_float64_recurrence():
    Cn = chunk_elems()
    n = Cn + 1023
    gen = torch.Generator().manual_seed(50)
    e0, p = values(n, gen), values(n, gen)
    buf, ev = guarded(e0)
    pv = p.clone().to(DEV)
    state = torch.tensor([0.0, 0.0], dtype=torch.float64, device=DEV)
    ref, total = e0.numpy().astype(np.float64), np.zeros(n)
    worst_step = 0.0
    for t in range(50):
        if t % 3 == 2:
            pv.copy_(ev)                                           # every third step the model IS the average
        else:
            p = (p + 0.25 * values(n, gen)).float()               # a moving model
            pv.copy_(p.to(DEV))
        p_now = pv.cpu().numpy()
        launch([('x', ev, pv)], 0.9, 5.0, state)
        wf = er.w32(state[1].item())
        (ref, bound), = er.follow(ref, [p_now], [wf])
        total += bound
        err = np.abs(ev.cpu().numpy().astype(np.float64) - ref)
        assert (err <= total).all(), (t, float((err / np.where(total > 0, total, 1.0)).max()))
        worst_step = max(worst_step, float((err / np.where(total > 0, total, 1.0)).max()))
    print(f'fifty updates: largest error / summed bound {float((err / np.where(total > 0, total, 1.0)).max()):.4f} at the end, {worst_step:.4f} at any step')
    assert state[0].item() == 50.0 and sentinels_intact(buf, 0, n)


# ---------------------------------------------------------------------------------------------------------------- the library model
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


def make(capturable=True):
    from fastvision_amd import FusedAdam
    from fastvision_amd.loss import Yolov3Loss
    net = lib_model()
    crit = Yolov3Loss(net, 0.5, 0.05, 1.0, 0.5)
    opt = FusedAdam(net.parameters(), lr=1e-4, betas=(0.937, 0.999), weight_decay=5e-4, capturable=capturable)
    return net, crit, opt


def eager_step(net, crit, opt, images, tg, ema=None):
    pred = net(images)
    opt.zero_grad()
    loss = crit(pred, tg)
    loss.backward()
    opt.step()
    if ema is not None:
        ema.update(net)
    return loss.detach().clone()


def state_of(net, opt):
    out = {k: v.detach().clone() for k, v in net.state_dict().items()}
    for i, p in enumerate(net.parameters()):
        out[f'm{i}'] = opt.state[p]['exp_avg'].clone()
        out[f'v{i}'] = opt.state[p]['exp_avg_sq'].clone()
    return out


def flat(out):
    if torch.is_tensor(out):
        return [out]
    return [t for o in out for t in flat(o)]


@functools.lru_cache(maxsize=None)
def batches():
    from fastvision_amd.synthetic import synthetic_batch
    return tuple(synthetic_batch(2, 128, seed=s) for s in (1234, 7, 99))


# ---------------------------------------------------------------------------------------------------------------- 4: caches
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_averaged_model_evaluates_what_it_holds(dtype):
    import fastvision_amd
    from fastvision_amd import ModelEMA
    images = batches()[0][0].to(DEV)
    with fastvision_amd.compute_dtype(dtype), torch.no_grad():
        net = lib_model()
        ema = ModelEMA(net, decay=0.9, tau=0.0)
        before = [t.clone() for t in flat(ema.module(images, val=True))]       # packed weights and eval coefficients now exist
        gen = torch.Generator(device=DEV).manual_seed(4)
        for k, v in net.state_dict().items():
            if k.endswith('running_var'):
                v.mul_(1.0 + 0.5 * torch.rand(v.shape, generator=gen, device=DEV))
            elif v.dtype.is_floating_point:
                v.add_(0.05 * torch.randn(v.shape, generator=gen, device=DEV))
            else:
                v.add_(3)
        ema.update(net)
        got = flat(ema.module(images, val=True))
        fresh = lib_model(seed=1)
        fresh.load_state_dict(ema.module.state_dict())
        want = flat(fresh.eval()(images, val=True))
        torch.cuda.synchronize()
    assert len(got) == len(want) == len(before) and len(got) >= 2
    assert any(not torch.equal(a, b) for a, b in zip(got, before))              # the update changed what the model computes
    for a, b in zip(got, want):
        assert a.shape == b.shape and torch.isfinite(a.float()).all() and torch.equal(a, b)
    for k, v in ema.module.state_dict().items():
        if not v.dtype.is_floating_point:
            assert torch.equal(v, net.state_dict()[k]), k                       # copied, not averaged


# ---------------------------------------------------------------------------------------------------------------- 5: training
def test_training_is_untouched_by_the_average():
    import fastvision_amd
    from fastvision_amd import ModelEMA
    with fastvision_amd.compute_dtype(torch.float32):
        res = []
        for with_ema in (False, True):
            net, crit, opt = make(capturable=False)
            ema = ModelEMA(net) if with_ema else None
            for im, tg in batches():
                eager_step(net, crit, opt, im.to(DEV), tg.to(DEV), ema)
            res.append(state_of(net, opt))
        torch.cuda.synchronize()
    assert ema.updates == 3
    for k in res[0]:
        assert torch.equal(res[0][k], res[1][k]), k
    moved = [k for k, v in ema.module.state_dict().items() if v.dtype.is_floating_point and not torch.equal(v, res[1][k])]
    assert moved                                                                 # (the average lags behind the model)


# ---------------------------------------------------------------------------------------------------------------- 6: no sync
def test_update_does_not_synchronise_the_host():
    from fastvision_amd import ModelEMA
    net = small_net()
    ema = ModelEMA(net)
    ema.update(net)                                                # warm-up: tables
    torch.cuda.synchronize()
    with torch.no_grad():
        net[0].weight.add_(1.0)
    torch.cuda.set_sync_debug_mode('error')
    try:
        ema.update(net)
        ema.update(net)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert ema.updates == 3


# ---------------------------------------------------------------------------------------------------------------- 7: captured steps
def test_graphed_step_with_an_average_is_bit_identical_with_eager():
    import fastvision_amd
    from fastvision_amd import ModelEMA
    from fastvision_amd.graphs import GraphedTrainStep
    bs = batches()
    cap = max(t.shape[0] for _, t in bs) + 5
    lrs = [1e-4, 1e-4, 3e-5, 3e-5]
    order = [0, 1, 2, 0]
    with fastvision_amd.compute_dtype(torch.bfloat16):
        net, crit, opt = make()
        ema = ModelEMA(net, decay=0.99, tau=3.0)
        want = []
        for i, lr in zip(order, lrs):
            opt.param_groups[0]['lr'] = lr
            im, tg = bs[i]
            want.append(eager_step(net, crit, opt, im.to(DEV), tg.to(DEV), ema))
        torch.cuda.synchronize()

        net2, crit2, opt2 = make()
        ema2 = ModelEMA(net2, decay=0.99, tau=3.0)
        start = {k: v.clone() for k, v in ema2.module.state_dict().items()}
        im0, tg0 = bs[0]
        step = GraphedTrainStep(net2, lambda p, t: crit2(p, t), opt2, im0.to(DEV), tg0.to(DEV), max_targets=cap, ema=ema2)
        assert ema2.updates == 0                                    # warm-up and capture left the average and its counter alone
        for k, v in ema2.module.state_dict().items():
            assert torch.equal(v, start[k]), k
        got = []
        for i, lr in zip(order, lrs):
            opt2.param_groups[0]['lr'] = lr
            im, tg = bs[i]
            got.append(step(im.to(DEV), tg.to(DEV)).clone())
        torch.cuda.synchronize()
    for a, b in zip(got, want):
        assert torch.equal(a, b), (a, b)
    for (k, a), (_, b) in zip(net2.state_dict().items(), net.state_dict().items()):
        assert torch.equal(a, b), k
    sd, sd2 = ema.module.state_dict(), ema2.module.state_dict()
    assert any(v.dtype.is_floating_point and not torch.equal(v, start[k]) for k, v in sd2.items())
    for k in sd:
        assert torch.equal(sd2[k], sd[k]), k
    assert ema.updates == 4 and ema2.updates == 4
    assert torch.equal(ema._state, ema2._state)
    # the averaged model after replays must evaluate its new weights (versions advanced after each replay)
    with torch.no_grad(), fastvision_amd.compute_dtype(torch.bfloat16):
        a = ema.module(bs[1][0].to(DEV), val=True)[1]
        b = ema2.module(bs[1][0].to(DEV), val=True)[1]
    assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------- 8: checkpoints
def test_checkpoint_round_trip(tmp_path):
    from fastvision_amd import ModelEMA
    net = small_net()
    a = ModelEMA(net, decay=0.999, tau=10.0)
    with torch.no_grad():
        for _ in range(3):
            for p in net.parameters():
                p.mul_(1.01).add_(0.01)
            net[1].num_batches_tracked.add_(1)
            a.update(net)
    torch.save(a.state_dict(), tmp_path / 'ema.pth')
    sd = torch.load(tmp_path / 'ema.pth', weights_only=False)
    assert set(sd) == {'module', 'updates', 'decay', 'tau'} and sd['updates'] == 3 and sd['decay'] == 0.999 and sd['tau'] == 10.0
    b = ModelEMA(small_net(seed=9))                                 # other weights, other hyper-parameters
    b.load_state_dict(sd)
    assert b.updates == 3 and b.decay == 0.999 and b.tau == 10.0
    with torch.no_grad():
        net[0].weight.add_(0.5)
    a.update(net)
    b.update(net)
    assert torch.equal(a._state, b._state) and a.updates == 4
    for (k, x), (_, y) in zip(a.module.state_dict().items(), b.module.state_dict().items()):
        assert torch.equal(x, y), k
    # snapshot / restore: device copies that keep addresses
    ptrs = [t.data_ptr() for t in a.module.state_dict().values()]
    snap = a.snapshot_state()
    a.update(net)
    a.restore_state(snap)
    assert a.updates == 4 and ptrs == [t.data_ptr() for t in a.module.state_dict().values()]
    for (k, x), (_, y) in zip(a.module.state_dict().items(), b.module.state_dict().items()):
        assert torch.equal(x, y), k


def test_tied_and_replaced_tensors():
    """A tensor that appears under two keys is updated once; a parameter that moved gets a new table."""
    from fastvision_amd import ModelEMA

    class Tied(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a = torch.nn.Linear(4, 4, bias=False)
            self.b = torch.nn.Linear(4, 4, bias=False)
            self.b.weight = self.a.weight
    net = Tied().to(DEV)
    ema = ModelEMA(net, decay=0.5, tau=0.0)
    assert ema.module.a.weight is ema.module.b.weight
    e0, p0 = ema.module.a.weight.clone(), net.a.weight.detach().clone()
    with torch.no_grad():
        net.a.weight.add_(1.0)
    ema.update(net)
    assert ema._tab['n'] == 1                                          # one table row for the two keys
    assert torch.equal(ema.module.a.weight, e0 + 0.5 * ((p0 + 1.0) - e0))
    net.a.weight = net.b.weight = torch.nn.Parameter(torch.full((4, 4), 3.0, device=DEV))
    before = ema.module.a.weight.clone()
    ema.update(net)
    assert torch.equal(ema.module.a.weight, before + 0.5 * (3.0 - before)) and ema.updates == 2
    with pytest.raises(RuntimeError, match='contiguous'):
        bad = torch.nn.Linear(4, 4).to(DEV)
        bad.weight = torch.nn.Parameter(torch.zeros(4, 8, device=DEV)[:, ::2])
        ModelEMA(bad)


# ---------------------------------------------------------------------------------------------------------------- 9: the fit loop
def test_fit_validates_and_checkpoints_the_average(tmp_path):
    import fastvision_amd
    from fastvision_amd import ModelEMA
    from fastvision_amd.utils import Fit
    loader = [(im, tg) for im, tg in batches()[:2]]
    path = str(tmp_path / 'last.pth')
    with fastvision_amd.compute_dtype(torch.float32):
        net, crit, opt = make(capturable=False)
        ema = ModelEMA(net, decay=0.9, tau=0.0)
        fit = Fit(net, torch.device(DEV), opt, None, crit, end_epoch=1, train_loader=loader, val_loader=loader, save_last=path, ema=ema)
        fit.run_epoches()
        assert ema.updates == 2
        want, raw = [], []
        with torch.no_grad():
            for im, tg in loader:
                want.append(crit(ema.module(im.to(DEV), val=True)[0], tg.to(DEV)).float().item())
                raw.append(crit(net.eval()(im.to(DEV), val=True)[0], tg.to(DEV)).float().item())
    assert fit.last_val['loss'] == want and want != raw
    assert not ema.module.training
    ckpt = torch.load(path, weights_only=False)
    assert set(ckpt) == {'model', 'optimizer', 'date', 'ema'}
    assert set(ckpt['ema']) == {'module', 'updates', 'decay', 'tau'} and ckpt['ema']['updates'] == 2
    for k, v in ema.module.state_dict().items():
        assert torch.equal(ckpt['ema']['module'][k], v), k
    assert any(not torch.equal(ckpt['ema']['module'][k], ckpt['model'][k]) for k in ckpt['model'])


def test_demo_fit_validates_and_saves_the_average(tmp_path, monkeypatch):
    """demos/yolov3_u/cfg/_fit.py with ``ema=``: validation runs the averaged model, the criterion receives it, the best-epoch file holds it."""
    import types
    from fastvision_amd import ModelEMA
    from fastvision_amd.demos.yolov3_u.cfg import _fit as demo
    monkeypatch.chdir(tmp_path)

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.ones(2))

        def forward(self, x):
            return (x * self.w).sum()
    net = Net().to(DEV)
    ema = ModelEMA(net, decay=0.5, tau=0.0)
    opt = torch.optim.SGD(net.parameters(), lr=0.5)
    seen = []

    def criterion(predict, target, model):
        seen.append(model)
        return predict + target.sum()
    loader = [(torch.ones(2), torch.zeros(1))]
    demo.Fit(net, types.SimpleNamespace(start_epoch=0, max_epochs=1), opt, criterion, None, loader, loader, ema=ema)
    assert seen == [net, ema.module] and net.training and not ema.module.training
    # model: w = 1 - 0.5 = 0.5; average: 1 + 0.5 * (0.5 - 1) = 0.75; validation loss = 2 * 0.75
    assert torch.equal(ema.module.w.cpu(), torch.full((2,), 0.75)) and ema.updates == 1
    saved = torch.load(tmp_path / 'epoch_1_loss_1.5.pth')
    assert torch.equal(saved['w'].cpu(), torch.full((2,), 0.75))
