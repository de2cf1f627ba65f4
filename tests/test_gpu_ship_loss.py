"""The ship demo on the device (fastvision_amd.demos.yolov3_huaweiShip): fva_demo_ciou_loss, fva_scale_head_groups and fva_yolo_decode
variant 2 element by element against tests/ship_restatement.py (the formula in float64, torch.autograd for the gradient), with the
measure of tests/streaming_measure.py (FACTOR = 4) and the limits as tests/loss_restatement.py builds them; against the reference's own
vectors (tests/golden/ship_loss.npz); and one training step captured in a HIP graph against the same step issued eagerly.
Every worst err / limit is printed (pytest -s); DESIGN.md section 4 holds the table.
"""
import os

import numpy as np
import pytest
import torch

import detect_restatement as dr
import loss_restatement as lr
import ship_restatement as sr
import streaming_measure as sm

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F64, F32 = torch.float64, torch.float32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ship_loss.npz')


def report(what, **worst):
    print(f'{what}: worst err / limit ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= 1.0, f'{what}: {k} worst err / limit = {v:.3f}'


def close32(got, want, rtol, atol, what):
    got, want = got.detach().cpu().float().reshape(want.shape), want.detach().float()
    assert torch.isfinite(got).all() and torch.isfinite(want).all(), what
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=rtol, atol=atol, err_msg=what)


class Shell:
    def __init__(self, anchors):
        self.anchors = tuple(a.to(DEV) for a in anchors)


def device_layers(layers, form, grad=True):
    ld = [l.to(DEV) for l in layers]
    if form == 'nhwc':
        ld = [l.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2) for l in ld]
    return [l.detach().requires_grad_(grad) for l in ld]


def run_ship(layers, tg, anchors, form, weights=(1.0, 1.0, 1.0), only=None):
    """-> (values [3] on the CPU, gradients per level on the CPU) of weights . (box, cls, conf), or of the part ``only`` alone."""
    from fastvision_amd.demos.yolov3_huaweiShip.utils import ComputeLoss
    ld = device_layers(layers, form)
    crit = ComputeLoss()
    parts = crit(ld, tg.to(DEV), Shell(anchors))
    assert all(p.shape == (1,) for p in parts)
    if only is not None:
        parts[only].backward()
    elif weights == (1.0, 1.0, 1.0):
        (parts[0] + parts[1] + parts[2]).backward()
    else:
        (parts[0] * weights[0] + parts[1] * weights[1] + parts[2] * weights[2]).backward()
    assert torch.equal(crit.last_parts, torch.cat([p.detach() for p in parts]))
    return torch.cat([p.detach() for p in parts]).cpu(), [l.grad.cpu() for l in ld]


_REFS = {}


def reference(name):
    """the case and its float64 reference, computed once and shared (never modified)"""
    if name not in _REFS:
        case = lr.demo_case(name)
        _REFS[name] = (case, sr.ship_reference(*case))
    return _REFS[name]


# ================================================================================================ values and gradients
@pytest.mark.parametrize('name,form', [(n, 'nchw') for n in lr.DEMO_CASES] + [(n, 'nhwc') for n in ('c80', 'c1', 'empty+200')])
def test_ship_loss(name, form):
    (layers, tg, anchors), ref = reference(name)
    assert ref['undecidable'] == 0
    vals, grads = run_ship(layers, tg, anchors, form)
    w = {'values': lr.worst(vals, ref['vals64'], ref['val_limits'])}
    ignored = 0
    for l, g in enumerate(grads):
        w[f'grad{l}'] = lr.worst(g, ref['grads64'][l], ref['grad_limits'][l])
        Bn, ch, H, W = g.shape
        A = anchors[l].shape[0]
        obj = g.permute(0, 2, 3, 1).reshape(Bn, H, W, A, ch // A)[..., 4]
        ign = ref['masks'][l] == -1
        ignored += int(ign.sum())
        assert (obj[ign] == 0).all()                       # ignored cells: exactly 0
    if name in ('c80', 'empty+200'):                       # the cases meant for the ignore mask hold ignored background cells
        assert ignored > (lr.DEMO_PLANTED if name == 'empty+200' else 0), ignored
    report(f'ship {name} {form} (ignored cells {ignored})', **w)


@pytest.mark.parametrize('name', ['c65', 'c1', 'c80'])
def test_ship_loss_against_the_reference_vectors(name):
    gold = np.load(GOLD)
    layers, tg, anchors = lr.demo_case(name)
    vals, grads = run_ship(layers, tg, anchors, 'nchw')
    np.testing.assert_allclose(vals.numpy(), gold[f'{name}_values'], rtol=1e-5, atol=0)
    for l in range(1 if name == 'c80' else len(layers)):
        np.testing.assert_allclose(grads[l].numpy(), gold[f'{name}_grad{l}'], rtol=1e-3, atol=1e-6)


def test_ship_saturated_logits():
    """Objectness and class logits of +-30 / +-100 (the box logits stay inside |z| <= 8: exp(100) * anchor is inf in the reference too):
    finite, and the fp32 restatement's values (rtol 1e-5) and gradients (rtol 1e-4, atol 1e-6), as test_demo_saturated_logits."""
    layers, tg, anchors = lr.demo_case('c65')
    layers = [l.clone() for l in layers]
    g = torch.Generator().manual_seed(172)
    K = 70
    vals4 = torch.tensor([30.0, -30.0, 100.0, -100.0])
    for a in range(3):
        t = layers[0][:, a * K + 4:(a + 1) * K]
        pick = torch.rand(t.shape, generator=g) < 0.1
        layers[0][:, a * K + 4:(a + 1) * K] = torch.where(pick, vals4[torch.randint(0, 4, t.shape, generator=g)], t)
        assert layers[0][:, a * K:a * K + 4].abs().max() <= 8
    assert (layers[0].abs() >= 30).sum() > 100
    leaves = [l.clone().requires_grad_(True) for l in layers]
    parts, _ = sr.ship_terms(leaves, tg, anchors, F32)
    (parts[0] + parts[1] + parts[2]).backward()
    vals, grads = run_ship(layers, tg, anchors, 'nchw')
    close32(vals, torch.stack([p.detach() for p in parts]), 1e-5, 0, 'saturated ship values')
    close32(grads[0], leaves[0].grad, 1e-4, 1e-6, 'saturated ship gradients')


# ================================================================================================ three-part backward
def group_factors(shape, A, weights):
    """[1, A * K, 1, 1] float64: the factor of every channel (k < 4 box, k == 4 objectness, k >= 5 class)"""
    K = shape[1] // A
    per = torch.tensor([weights[0]] * 4 + [weights[2]] + [weights[1]] * (K - 5), dtype=F64)
    return per.repeat(A).view(1, A * K, 1, 1)


def at_most_two_per_cell(layers, tg, anchors):
    """the targets of a case without those that would be the third in their (cell, anchor) on some level: the stored gradient is then the
    same in every run, bit for bit -- fp32 addition of two terms commutes, of three it does not, and the order of atomicAdd is not fixed"""
    keep = []
    lr.demo_terms(layers, tg, anchors, F64, keep=keep)
    ok = torch.ones(tg.shape[0], dtype=torch.bool)
    for info in keep:
        seen = {}
        for t, c in enumerate(info['cell'].tolist()):
            seen[c] = seen.get(c, 0) + 1
            if seen[c] > 2:
                ok[t] = False
    return tg[ok]


@pytest.mark.parametrize('name,form', [('c1', 'nchw'), ('c1', 'nhwc'), ('c80', 'nchw'), ('c80', 'nhwc'), ('cells', 'nchw'), ('cells', 'nhwc')])
def test_three_part_backward(name, form):
    """K = 6 (c1, cells) and K = 85 (c80); 'cells' holds 264600 cells x 6 channels: the scale kernel's grid-stride loop runs more than once."""
    layers, tg, anchors = lr.demo_case(name)
    tg = at_most_two_per_cell(layers, tg, anchors)
    assert tg.shape[0] >= 6
    _, unit = run_ship(layers, tg, anchors, form)
    assert any((u != 0).any() for u in unit)
    # powers of two: exact
    _, got = run_ship(layers, tg, anchors, form, weights=(0.5, 2.0, 0.25))
    for l, (g, u) in enumerate(zip(got, unit)):
        want = (u.double() * group_factors(u.shape, anchors[l].shape[0], (0.5, 2.0, 0.25))).float()
        assert torch.equal(g, want), (name, form, l)
    # one part alone: the other groups exactly 0, its own group the unit-weight gradient
    _, got = run_ship(layers, tg, anchors, form, only=0)
    for l, (g, u) in enumerate(zip(got, unit)):
        A = anchors[l].shape[0]
        sel = group_factors(u.shape, A, (1.0, 0.0, 0.0)).expand(u.shape) == 1
        assert (g[~sel] == 0).all() and torch.equal(g[sel], u[sel]) and (g[sel] != 0).any()
    # general weights: one rounding of the float64 product
    wts = (0.3, 1.7, 0.9)
    _, got = run_ship(layers, tg, anchors, form, weights=wts)
    worst = 0.0
    for l, (g, u) in enumerate(zip(got, unit)):
        f32w = tuple(float(np.float32(w)) for w in wts)            # the upstream scalars are fp32 tensors
        want = u.double() * group_factors(u.shape, anchors[l].shape[0], f32w)
        err = (g.double() - want).abs()
        assert (err <= 2.0 ** -23 * want.abs()).all(), (name, form, l)
        worst = max(worst, (err / want.abs().clamp_min(1e-300)).max().item() / 2.0 ** -23)
    print(f'three-part backward {name} {form}: worst relative error / 2^-23 = {worst:.3f}')


def test_three_part_backward_fallback_multiplies_per_group():
    """A gradient buffer that does not meet the in-place conditions (here: a view that starts inside its storage) takes the plain multiply
    per channel group and is left as it was; a buffer that meets them is scaled where it stands.  Both give the same numbers."""
    import types
    from fastvision_amd import ops
    g = torch.Generator().manual_seed(4)
    full = torch.randn(3, 18, 5, 7, generator=g).to(DEV)
    scal = [torch.tensor([w], device=DEV) for w in (0.5, 2.0, 0.25)]            # box, cls, conf
    want = (full[1:].double().cpu() * group_factors(full[1:].shape, 3, (0.5, 2.0, 0.25))).float()
    view, own = full[1:], full[1:].clone()
    assert view.storage_offset() != 0 and own.storage_offset() == 0
    for buf, in_place in ((view, False), (own, True)):
        before = buf.clone()
        ctx = types.SimpleNamespace(grads=[buf], dtypes=[torch.float32], anchors_per_level=[3])
        out, = ops.scale_head_group_grads(ctx, *scal)
        assert torch.equal(out.cpu(), want)
        assert (out.data_ptr() == buf.data_ptr()) == in_place
        assert in_place or torch.equal(buf, before)
        with pytest.raises(RuntimeError):                                        # the buffers are spent
            ops.scale_head_group_grads(ctx, *scal)


# ================================================================================================ value-only path
def test_value_only_path_allocates_no_gradient_buffer():
    from fastvision_amd.demos.yolov3_huaweiShip.utils import ComputeLoss
    layers, tg, anchors = lr.demo_case('cells')
    vals, _ = run_ship(layers, tg, anchors, 'nchw')
    ld = device_layers(layers, 'nchw', grad=False)
    tgd, shell, crit = tg.to(DEV), Shell(anchors), ComputeLoss()
    head_bytes = ld[0].numel() * 4
    with torch.no_grad():
        crit(ld, tgd, shell)                               # allocator warm-up
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        parts = crit(ld, tgd, shell)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
    assert all(not p.requires_grad for p in parts)
    assert torch.equal(torch.cat(parts).cpu(), vals)
    assert peak < head_bytes // 2, (peak, head_bytes)     # workspace (one byte per cell and the per-target rows) only: no head-sized buffer
    # the same under requires_grad inputs but no_grad mode
    ld = device_layers(layers, 'nchw', grad=True)
    with torch.no_grad():
        parts = crit(ld, tgd, shell)
    assert torch.equal(torch.cat(parts).cpu(), vals) and all(p.grad_fn is None for p in parts)


# ================================================================================================ decode variant 2
@pytest.mark.parametrize('name', list(dr.DECODE_CASES))
@pytest.mark.parametrize('letterbox', [False, True])
def test_decode_variant2_every_element(name, letterbox):
    from fastvision_amd.detect_ops import yolo_decode
    heads, anchors, strides, lb = dr.decode_case(name)
    box = lb if letterbox else None
    r64, mag, e64 = sr.decode_rows2(heads, anchors, strides, box, F64)
    r32, _, e32 = sr.decode_rows2(heads, anchors, strides, box, F32)
    dev = [h.to(DEV) for h in heads]
    got = yolo_decode(dev, anchors, strides, variant=2, letterbox=box)
    assert torch.equal(got, yolo_decode([dr.nhwc_view(h) for h in dev], anchors, strides, variant=2, letterbox=box))
    got = got.cpu()
    if box is not None:
        ex = dr.decode_excused(e64, e32, box[5])
        assert ex.double().mean().item() <= dr.MAX_EXCUSED
        got[..., 4] = torch.where(ex, r64[..., 4].float(), got[..., 4])
        assert torch.equal(got[..., 4] == -1, r64[..., 4] == -1)
    w = sm.check(got, r64, r32, mag, False, factor=sm.FACTOR, what=f'{name} variant 2')
    print(f'decode {name} variant 2 letterbox {letterbox}: worst err / limit {w:.3f}')


@pytest.mark.parametrize('variant,name', [(0, 'four_levels_k85'), (1, 'two_levels_k7')])
def test_decode_variants_0_and_1_are_unchanged(variant, name):
    from fastvision_amd.detect_ops import yolo_decode
    heads, anchors, strides, lb = dr.decode_case(name)
    box = lb if variant == 1 else None
    r64, mag, e64 = dr.decode_rows(heads, anchors, strides, variant, box, F64)
    r32, _, e32 = dr.decode_rows(heads, anchors, strides, variant, box, F32)
    got = yolo_decode([h.to(DEV) for h in heads], anchors, strides, variant=variant, letterbox=box).cpu()
    if box is not None:
        ex = dr.decode_excused(e64, e32, box[5])
        got[..., 4] = torch.where(ex, r64[..., 4].float(), got[..., 4])
        assert torch.equal(got[..., 4] == -1, r64[..., 4] == -1)
    sm.check(got, r64, r32, mag, False, factor=sm.FACTOR, what=f'{name} variant {variant}')


def test_postprocess_uses_variant_2():
    """postProcess = decode variant 2 with the letterbox tail + the demo NMS, on one image"""
    from fastvision_amd.demos.yolov3_huaweiShip.inference import postProcess
    from fastvision_amd.detect_ops import NMS_DEMO, nms_batch, yolo_decode
    g = torch.Generator().manual_seed(8)
    C_, sizes, strides = 2, (2, 4, 8), [32, 16, 8]
    anchors = [torch.tensor([[3.0, 2.0], [1.5, 2.5], [1.0, 1.0]]) for _ in sizes]
    layers = [(torch.randn(1, 3 * (5 + C_), s, s, generator=g) * 1.5).to(DEV) for s in sizes]
    args = (0.8, 2.0, 6.0, 70.0, 60.0)
    scores, cats, boxes = postProcess(layers, strides, [a.to(DEV) for a in anchors], 0.25, 0.45, *args)
    heads = [l.unflatten(1, (3, 5 + C_)).permute(0, 1, 3, 4, 2) for l in layers]
    rows = yolo_decode(heads, [[tuple(p) for p in a.tolist()] for a in anchors], strides, variant=2, letterbox=args + (5.0,))
    det, _ = nms_batch(rows, 0.25, 0.45, 300, NMS_DEMO)[0]
    assert det.shape[0] > 0 and torch.equal(torch.cat([boxes, scores, cats], 1), det)


# ================================================================================================ one graphed step
def three_groups(model):
    """the script's parameter groups (train.py:70-87): BatchNorm weights, other weights (decayed), biases"""
    g0, g1, g2 = [], [], []
    for v in model.modules():
        if hasattr(v, 'bias') and isinstance(v.bias, torch.nn.Parameter):
            g2.append(v.bias)
        if isinstance(v, torch.nn.BatchNorm2d):
            g0.append(v.weight)
        elif hasattr(v, 'weight') and isinstance(v.weight, torch.nn.Parameter):
            g1.append(v.weight)
    return [{'params': g0}, {'params': g1, 'weight_decay': 5e-4}, {'params': g2}]


def test_graphed_ship_step_is_bit_identical_with_eager():
    import fastvision_amd
    from fastvision_amd import FusedSGD, ops
    from fastvision_amd.demos.yolov3_huaweiShip.inference import anchor_fn
    from fastvision_amd.demos.yolov3_huaweiShip.models import YoloV3
    from fastvision_amd.demos.yolov3_huaweiShip.utils import ComputeLoss
    from fastvision_amd.graphs import GraphedTrainStep
    from fastvision_amd.synthetic import synthetic_batch
    im, _ = synthetic_batch(2, 64, seed=5)
    # four targets per image, one per quadrant: no (cell, anchor) of the 2 x 2, 4 x 4 and 8 x 8 grids receives more than one target, so the
    # atomicAdd'ed head gradient does not depend on the order in which the wavefronts arrive (three or more fp32 terms would)
    g = torch.Generator().manual_seed(6)
    quad = torch.tensor([[0.25, 0.25], [0.75, 0.25], [0.25, 0.75], [0.75, 0.75]])
    tg = torch.cat([torch.cat([torch.full((4, 1), float(b)), torch.randint(0, 2, (4, 1), generator=g).float(),
                               quad + (torch.rand(4, 2, generator=g) - 0.5) * 0.1, 0.1 + 0.5 * torch.rand(4, 2, generator=g)], 1) for b in range(2)])
    zeros = [torch.zeros(2, 21, s, s) for s in (2, 4, 8)]
    assert at_most_two_per_cell(zeros, tg, [a.cpu() for a in anchor_fn('cpu')]).shape[0] == 8
    im, tg = im.to(DEV), tg.to(DEV)
    lrs = [1e-3, 3e-4]

    def make():
        torch.manual_seed(3)
        net = YoloV3(num_classes=2, anchors=anchor_fn(DEV)).to(DEV).train()
        groups = three_groups(net)
        assert all(len(g['params']) > 0 for g in groups) and sum(len(g['params']) for g in groups) == len(list(net.parameters()))
        crit = ComputeLoss()
        opt = FusedSGD(groups, lr=lrs[0], momentum=0.937, nesterov=True, capturable=True)

        def loss_fn(pred, t):
            box, cls, conf = crit(pred, t, net)
            return box + cls + conf
        return net, loss_fn, opt

    was = ops.set_wgrad_side_stream(False)   # the eager steps on ONE stream, as the capture is
    try:
        with fastvision_amd.compute_dtype(torch.float32):
            net, loss_fn, opt = make()
            want = []
            for lr_ in lrs:
                for g in opt.param_groups:
                    g['lr'] = lr_
                pred = net(im)
                opt.zero_grad()
                loss = loss_fn(pred, tg)
                loss.backward()
                opt.step()
                want.append(loss.detach().clone())
            torch.cuda.synchronize()
            net2, loss_fn2, opt2 = make()
            step = GraphedTrainStep(net2, loss_fn2, opt2, im, tg)
            got = []
            for lr_ in lrs:
                for g in opt2.param_groups:
                    g['lr'] = lr_
                got.append(step(im, tg).clone())
            torch.cuda.synchronize()
    finally:
        ops.set_wgrad_side_stream(was)
    print('graphed', [repr(a.item()) for a in got], 'eager', [repr(b.item()) for b in want])
    for a, b in zip(got, want):
        assert torch.isfinite(a).all() and torch.equal(a, b), (a, b)
    for (k, a), (_, b) in zip(net2.state_dict().items(), net.state_dict().items()):
        assert torch.equal(a, b), k
    for p, q in zip(net.parameters(), net2.parameters()):
        assert torch.equal(opt.state[p]['momentum_buffer'], opt2.state[q]['momentum_buffer'])
