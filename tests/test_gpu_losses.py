"""The kernels of csrc/loss.hip element by element against float64: every loss value, every part and EVERY gradient element against
tests/loss_restatement.py (the formula in float64, torch.autograd for the gradient) on the operands the kernel reads, in the regimes the
golden vectors never reach: grid-stride loops that run twice (more than 262144 cells / elements, more than 8192 matches or targets), the
matcher's 1024-slot pass, class counts around the 64-lane loop, strided NHWC-backed heads, duplicates, the data-parallel form.

Measure (tests/streaming_measure.py, FACTOR = 4: loss.hip uses expf / logf, not the fast intrinsics):
  element:  |got - ref64| <= 4 * (e32 + 2^-24 * mag),  e32 = |restatement in fp32 - restatement in float64|,
            mag = the largest magnitude among the terms of the element's last addition, times the condition of the cancelling step in
            front of it.  The derivations sit where the mags are built:
              * BCE on probabilities, -t log(p + 1e-8) - (1 - t) log(1 - p + 1e-8) (loss_restatement.bce_prob_mag): 1 - p inherits p's absolute
                error 2^-24 * p, i.e. p / (1 - p + 1e-8) relative; the log turns that into as much ABSOLUTE error; in the gradient
                dl/dp * p (1 - p) the term (1 - t) p (1 - p) / (1 - p + 1e-8) carries the condition 1 / (1 - p + 1e-8).
              * IoU family (loss_restatement.box_condition): a width, an intersection or a hull side is a difference d of two corners of
                size c: c / d relative; the largest such ratio of the pair multiplies the sum of the |terms| (IoU, rho^2 / c^2, alpha v).
                Gradients w.r.t. a centre are the last addition of the two corner gradients (loss_restatement.yolov3_reference).
              * softmax rows: the kernel's denominator is one chain of C fp32 additions: (C + 6) * 2^-24 instead of 4 * 2^-24.
  atomicAdd: elements that m > 1 matches add into additionally get sum_limit(m, sum |term|).
  scalars:   sum_limit(n, sum |term|, sum e32) + 4 * 2^-24 * sum mag(term), n = the thread's own chain + 64 (wave) + 4 (block); the block
             partials are added in double.
Logits are drawn with |z| <= 8; the saturated cases (+-30, +-100) are compared with the fp32 restatement, the reference's own arithmetic.
Every worst err / limit is printed (pytest -s); DESIGN.md section 4 holds the table.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import loss_restatement as lr
import streaming_measure as sm

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F64, F32 = torch.float64, torch.float32
RATIOS = (0.05, 1.0, 0.5)


def report(what, **worst):
    print(f'{what}: worst err / limit ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= 1.0, f'{what}: {k} worst err / limit = {v:.3f}'


def nhwc_view(h):
    """[B, A, H, W, K] view of an NHWC buffer, as the head kernels hand it to the loss (test_decode_kernel_matches_reference)."""
    B, A, H, W, K = h.shape
    buf = h.permute(0, 2, 3, 1, 4).reshape(B, H, W, A * K).contiguous()
    return buf.view(B, H, W, A, K).permute(0, 3, 1, 2, 4)


# ================================================================================================ library loss
def lib_crit(shell):
    from fastvision_amd.loss import Yolov3Loss
    return Yolov3Loss(shell, 0.5, *RATIOS)


def lib_device(heads, form, grad=True):
    hd = [h.to(DEV) for h in heads]
    if form == 'nhwc':
        hd = [nhwc_view(h) for h in hd]
        assert not hd[0].is_contiguous() or hd[0].shape[1] == 1
    return [h.detach().requires_grad_(grad) for h in hd]


def check_lib(name, heads, tg, shell, form='contig'):
    crit = lib_crit(shell)
    hd = lib_device(heads, form)
    tgd = tg.to(DEV)
    matches, matched = lr.split_matches(crit.build_target(hd, tgd))
    ref = lr.yolov3_reference(heads, matches, matched, RATIOS)
    loss = crit(hd, tgd)
    parts = crit.last_parts
    loss.backward()
    vals = torch.cat([loss.detach().view(1), parts.view(3)]).cpu()
    w = {'values': lr.worst(vals, ref['vals64'], ref['val_limits'])}
    for l, h in enumerate(hd):
        assert torch.isfinite(h.grad).all()
        w[f'grad{l}'] = lr.worst(h.grad, ref['grads64'][l], ref['grad_limits'][l])
    report(f'library {name} {form} (matches {[m[0].numel() for m in matches]})', **w)
    return matches, vals, [h.grad.cpu() for h in hd]


@pytest.mark.parametrize('form', ['contig', 'nhwc'])
def test_library_nonsquare_c80(form):
    heads, tg, shell = lr.lib_case(101, 2, 3, 80, [(3, 5), (6, 10), (12, 20)], 40)
    matches, _, _ = check_lib('3x5 6x10 12x20 C80 T40', heads, tg, shell, form)
    assert all(m[0].numel() > 0 for m in matches)


@pytest.mark.parametrize('C_', [1, 17, 64, 65, 130])
def test_library_class_counts(C_):
    heads, tg, shell = lr.lib_case(110 + C_, 2, 3, C_, [(5, 7)], 40)
    check_lib(f'C{C_}', heads, tg, shell, 'nhwc' if C_ == 65 else 'contig')


@pytest.mark.parametrize('A', [1, 8])
def test_library_anchor_counts(A):
    heads, tg, shell = lr.lib_case(120 + A, 2, A, 1, [(5, 7)], 40)
    check_lib(f'A{A}', heads, tg, shell)


@pytest.mark.parametrize('T_', [341, 342, 700, 3000])
def test_library_matcher_passes_and_duplicates(T_):
    """T * A = 1023 / 1026 / 2100 across the matcher's 1024-slot pass.  B = 4 on 8 x 8: 768 cells for hundreds to thousands of matches --
    duplicates, last write wins, atomicMax, atomicAdd.  match_loss_kernel runs at most 2048 blocks of 4 waves and strides over the ACTUAL
    match count, so its loop takes a second trip only beyond 8192 matches: at T = 3000 the target sizes are drawn so that every target
    passes ratio < 4 against all three anchors (lr.ALL_THREE), 9000 matches."""
    heads, tg, shell = lr.lib_case(130 + T_, 4, 3, 1, [(8, 8)], T_, sizes=lr.ALL_THREE if T_ == 3000 else (0.02, 0.8))
    matches, _, _ = check_lib(f'T{T_}', heads, tg, shell)
    n = matches[0][0].numel()
    assert n > 8192 if T_ == 3000 else n > 300, n


def test_library_more_than_262144_cells():
    heads, tg, shell = lr.lib_case(140, 2, 3, 1, [(210, 210)], 6)
    assert 2 * 3 * 210 * 210 > 262144
    check_lib('264600 cells', heads, tg, shell)


def test_library_no_targets_and_target_on_the_right_edge():
    heads, tg, shell = lr.lib_case(150, 2, 3, 1, [(5, 7)], 0)
    matches, vals, grads = check_lib('T0', heads, tg, shell)
    assert matches[0][0].numel() == 0 and vals[1] == 0 and vals[3] == 0 and (grads[0][..., :4] == 0).all() and (grads[0][..., 5:] == 0).all()
    heads, tg, shell = lr.lib_case(151, 2, 3, 1, [(5, 7)], 12)
    tg[:, 4:] = torch.tensor([0.5, 0.4])                   # matches anchor 0 at every target
    tg[0, 2] = 1.0                                          # x = 1.0 exactly: cell W before the clamp, offset taken from it
    matches, _, _ = check_lib('x = 1.0', heads, tg, shell)
    b, gx, gy, a, cls, xywh = matches[0]
    assert gx[0] == 6 and xywh[0, 0] == 0.0                # 7.0 - floor(7.0), then clamped to W - 1


def test_library_value_without_gradients():
    heads, tg, shell = lr.lib_case(101, 2, 3, 80, [(3, 5), (6, 10), (12, 20)], 40)
    crit = lib_crit(shell)
    with_grad = crit(lib_device(heads, 'contig'), tg.to(DEV))
    parts = crit.last_parts.clone()
    hd = lib_device(heads, 'contig', grad=False)
    before = [h.clone() for h in hd]
    plain = crit(hd, tg.to(DEV))
    assert not plain.requires_grad and torch.equal(plain, with_grad.detach()) and torch.equal(crit.last_parts, parts)
    assert all(torch.equal(a, b) for a, b in zip(hd, before))


def test_library_data_parallel_form_direct():
    """fva_yolov3_loss_dp through the C ABI with invented job-wide numbers: match counts doubled, batch tripled (no process group)."""
    from fastvision_amd import _lib
    from fastvision_amd.loss.yolov3_loss import make_level
    from fastvision_amd.ops import _p, _stream
    heads, tg, shell = lr.lib_case(160, 2, 3, 5, [(5, 7), (8, 8)], 60)
    crit = lib_crit(shell)
    hd = [h.to(DEV) for h in heads]
    tgd = tg.to(DEV)
    matches, matched = lr.split_matches(crit.build_target(hd, tgd))
    counts = [2 * m[0].numel() for m in matches]
    norm_batch = 3 * heads[0].shape[0]
    ref = lr.yolov3_reference(heads, matches, matched, RATIOS, norm_counts=counts, norm_batch=norm_batch)
    grads = [torch.zeros_like(h) for h in hd]
    levels = (_lib.HeadLevel * len(hd))()
    for i, h in enumerate(hd):
        levels[i] = make_level(h, grads[i], crit._anchors_px[i], crit.backbone_stride_levels[i])
    T_ = tg.shape[0]
    wsb = _lib.load().fva_yolov3_loss_workspace(T_, levels, len(hd))
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    out = torch.empty(4, dtype=F32, device=DEV)
    cnt = torch.tensor(counts, dtype=torch.int32, device=DEV)
    _lib.call('fva_yolov3_loss_dp', _p(tgd), T_, levels, len(hd), *RATIOS, _p(cnt), norm_batch, _p(out), _p(ws), wsb, _stream())
    w = {'values': lr.worst(out, ref['vals64'], ref['val_limits'])}
    for l, g in enumerate(grads):
        w[f'grad{l}'] = lr.worst(g, ref['grads64'][l], ref['grad_limits'][l])
    report('library data-parallel form', **w)


def close32(got, want, rtol, atol, what):
    got, want = got.detach().cpu().float().reshape(want.shape), want.detach().float()
    assert torch.isfinite(got).all() and torch.isfinite(want).all(), what
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=rtol, atol=atol, err_msg=what)


def saturate(t, g):
    """+-30 and +-100 at random places of a logit tensor (about one element in ten)."""
    vals = torch.tensor([30.0, -30.0, 100.0, -100.0])
    pick = torch.rand(t.shape, generator=g) < 0.1
    return torch.where(pick, vals[torch.randint(0, 4, t.shape, generator=g)], t)


def test_library_saturated_logits():
    """Objectness and class logits of +-30 / +-100 at matched and background cells (the box logits stay inside |z| <= 8: exp(100) * anchor
    is inf in the reference too): finite, and the fp32 restatement's values (rtol 1e-5) and gradients (rtol 1e-4, atol 1e-6)."""
    heads, tg, shell = lr.lib_case(170, 2, 3, 5, [(5, 7)], 40)
    g = torch.Generator().manual_seed(171)
    heads[0][..., 4:] = saturate(heads[0][..., 4:], g)
    crit = lib_crit(shell)
    hd = lib_device(heads, 'contig')
    matches, matched = lr.split_matches(crit.build_target(hd, tg.to(DEV)))
    sat_matched = heads[0][matches[0][0], matches[0][3], matches[0][2], matches[0][1]][:, 4:].abs() >= 30
    assert sat_matched.any() and (heads[0][..., 4].abs() >= 30).sum() > sat_matched[:, 0].sum()
    leaves = [h.clone().requires_grad_(True) for h in heads]
    vals = lr.yolov3_terms(leaves, matches, matched, RATIOS, F32)
    vals[0].backward()
    loss = crit(hd, tg.to(DEV))
    loss.backward()
    close32(torch.cat([loss.detach().view(1), crit.last_parts]), torch.stack([v.detach() for v in vals]), 1e-5, 0, 'saturated library values')
    close32(hd[0].grad, leaves[0].grad, 1e-4, 1e-6, 'saturated library gradients')


# ================================================================================================ demo loss
def run_demo(layers, tg, anchors, form):
    from fastvision_amd.demos.yolov3_u.utils import ComputeLoss

    class M:
        pass
    M.anchors = tuple(a.to(DEV) for a in anchors)
    ld = [l.to(DEV) for l in layers]
    if form == 'nhwc':
        ld = [l.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2) for l in ld]
    ld = [l.detach().requires_grad_(True) for l in ld]
    crit = ComputeLoss()
    loss = crit(ld, tg.to(DEV), M())
    loss.backward()
    return torch.cat([loss.detach().view(1), crit.last_parts.view(4)]).cpu(), [l.grad.cpu() for l in ld]


@pytest.mark.parametrize('name,form', [(n, 'nchw') for n in lr.DEMO_CASES] + [(n, 'nhwc') for n in ('c80', 'c1', 'empty+200')])
def test_demo_loss(name, form):
    layers, tg, anchors = lr.demo_case(name)
    ref = lr.demo_reference(layers, tg, anchors)
    assert ref['undecidable'] == 0
    vals, grads = run_demo(layers, tg, anchors, form)
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
    report(f'demo {name} {form} (ignored cells {ignored})', **w)


def test_demo_saturated_logits():
    layers, tg, anchors = lr.demo_case('c65')
    g = torch.Generator().manual_seed(172)
    K = 70
    for a in range(3):
        layers[0][:, a * K + 4:(a + 1) * K] = saturate(layers[0][:, a * K + 4:(a + 1) * K], g)
    leaves = [l.clone().requires_grad_(True) for l in layers]
    total, parts, _ = lr.demo_terms(leaves, tg, anchors, F32)
    total.backward()
    vals, grads = run_demo(layers, tg, anchors, 'nchw')
    close32(vals, torch.stack([total.detach()] + [p.detach() for p in parts]), 1e-5, 0, 'saturated demo values')
    close32(grads[0], leaves[0].grad, 1e-4, 1e-6, 'saturated demo gradients')


# ================================================================================================ stand-alone BCE
# The stored gradient w * (-t / (p + eps) + (1 - t) / (1 - p + eps)) * p (1 - p) * scale is the end of a chain of fp32 roundings, counted in
# units of 2^-24 of the live term: the sigmoid 4 (expf to an ulp 2, 1 + e 1, the division 1), p + eps 1, the quotient 1, 1 - p 1, p (1 - p) 1,
# the product 1, the weight 1, the mean's 1 / numel 2 (the constant's own rounding and the product): 12 with labels, where the other term
# is an exact 0 and so is the addition; with a dense target the addition 1 and the other term's sigmoid-to-quotient chain at up to the
# same size on top: 16.  The plain factor 4 does not cover that, and it is the roundings, not the kernel: the kernel's operation sequence
# evaluated with fp32 torch ops on the CPU (tests/test_loss_restatement_cpu.py::test_bce_kernel_sequence_needs_more_than_factor_four)
# gives 1.226 of the factor-4 limit at 600000 dense targets with weights and the mean -- the figure the first MI355X run gave, on the same
# element -- and 1.160 at 52429 x 5 labels with logits, weights and the mean.  The gradient of the stand-alone BCE therefore gets 12 with
# labels and 16 with dense targets; its value and everything else keep 4.
BCE_LABEL_GRAD_FACTOR = 12.0
BCE_DENSE_GRAD_FACTOR = 16.0


def bce_direct(yd, lab, C_, weights, already, mean):
    """fva_bce_loss through the C ABI, as BiCrossEntropyLoss calls it: (value, stored gradient times the backward's scale).  The class
    routes a last dimension of 1 to dense targets, so LABELS with C = 1 (row = i, k = 0, every target 1) are reached only here."""
    from fastvision_amd import _lib
    from fastvision_amd.ops import _p, _stream
    numel = yd.numel()
    out, grad = torch.empty(1, dtype=F32, device=DEV), torch.empty(numel, dtype=F32, device=DEV)
    ws = torch.empty(1024, dtype=F32, device=DEV)
    w = None if weights is None else weights.to(DEV).float().contiguous().view(-1)
    yd, labd = yd.contiguous(), lab.to(DEV).long().contiguous()
    assert labd.numel() * C_ == numel and int(labd.min()) >= 0 and int(labd.max()) < C_
    _lib.call('fva_bce_loss', _p(yd), _p(labd), _p(None), _p(w), 0 if w is None else w.numel(), numel, C_,
              1 if already else 0, 1 if mean else 0, _p(out), _p(grad), _p(ws), _stream())
    return out.view(()), (grad * torch.tensor(1.0 / numel if mean else 1.0, dtype=F32, device=DEV)).view(yd.shape)


def check_bce(y, target, C_, weights, already, mean, grad_factor, direct=False):
    from fastvision_amd.loss import BiCrossEntropyLoss
    numel = y.numel()
    res = {}
    for dt in (F64, F32):
        leaf = y.detach().to(dt).clone().requires_grad_(True)
        keep = {}
        v = lr.bce(leaf, target, C_, dt, weights, already, mean, keep)
        v.backward()
        res[dt] = (v.detach(), leaf.grad, keep)
    (v64, g64, k64), (v32, g32, k32) = res[F64], res[F32]
    wexp = torch.ones(numel, dtype=F64) if weights is None else weights.double().reshape(-1).expand(numel)
    denom = numel if mean else 1
    vmag, gmag = lr.bce_prob_mag(k64['p'], k64['t'])
    if already:                                             # dl/dp itself: -t / (p + eps) + (1 - t) / (1 - p + eps), the second with 1 - p's condition
        p, t = k64['p'].detach(), k64['t']
        c = 1 / (1 - p + lr.BCE_EPS)
        gmag = torch.maximum(t / (p + lr.BCE_EPS), (1 - t) * c * c)
    blocks = min((numel + 255) // 256, lr.CONF_BLOCKS)
    vlim = lr.scalar_limit(lr.chain_of(numel, blocks * 256), k64['terms'], k32['terms'], wexp * vmag, denom) + sm.EPS32 * v64.abs()
    glim = sm.limit_of(g64, g32, (wexp * gmag / denom).view(g64.shape), grad_factor)
    if direct:
        got, grad = bce_direct(y.to(DEV), target, C_, weights, already, mean)
    else:
        yd = y.to(DEV).requires_grad_(True)
        got = BiCrossEntropyLoss('mean' if mean else 'sum')(yd, target.to(DEV), already_sigmoid=already, weights=None if weights is None else weights.to(DEV))
        got.backward()
        grad = yd.grad
    return lr.worst(got, v64, vlim), lr.worst(grad, g64, glim)


@pytest.mark.parametrize('numel', [1, 255, 256, 257, 65537, 262144, 262145, 600000])
def test_bce_dense_targets(numel):
    g = torch.Generator().manual_seed(numel)
    z = lr.logits((numel, 1), g)
    t = torch.rand(numel, 1, generator=g)
    wv, wg = 0.0, 0.0
    for weights in (None, torch.tensor([0.7]), torch.rand(numel, generator=g) + 0.1):
        for already in (False, True):
            for mean in (False, True):
                y = torch.sigmoid(z) if already else z
                a, b = check_bce(y, t, 1, weights, already, mean, BCE_DENSE_GRAD_FACTOR)
                wv, wg = max(wv, a), max(wg, b)
    report(f'bce dense numel {numel} (weights none / scalar / per element, logits and probabilities, sum and mean)', value=wv, grad=wg)


@pytest.mark.parametrize('rows,C_', [(1, 1), (257, 1), (262145, 1), (1, 5), (51, 5), (52429, 5), (13, 80), (3277, 80), (7500, 80)])
def test_bce_labels(rows, C_):
    """Labels (one-hot targets) with C = 1 / 5 / 80, each with no / scalar / per-element weights, logits and probabilities, sum and mean.
    C = 1 goes through the C ABI (bce_direct): BiCrossEntropyLoss takes a last dimension of 1 for a dense target."""
    g = torch.Generator().manual_seed(rows + C_)
    z = lr.logits((rows, C_), g)
    lab = torch.randint(0, C_, (rows,), generator=g)
    wv, wg = 0.0, 0.0
    for weights in (None, torch.tensor([1.3]), torch.rand(rows * C_, generator=g) + 0.1):
        for already in (False, True):
            for mean in (False, True):
                y = torch.sigmoid(z) if already else z
                a, b = check_bce(y, lab, C_, weights, already, mean, BCE_LABEL_GRAD_FACTOR, direct=(C_ == 1))
                wv, wg = max(wv, a), max(wg, b)
    report(f'bce labels {rows} x {C_}', value=wv, grad=wg)


def test_bce_saturated_logits():
    from fastvision_amd.loss import BiCrossEntropyLoss
    g = torch.Generator().manual_seed(173)
    z = saturate(lr.logits((300, 5), g), g)
    lab = torch.randint(0, 5, (300,), generator=g)
    leaf = z.clone().requires_grad_(True)
    want = lr.bce(leaf, lab, 5, F32, mean=True)
    want.backward()
    zd = z.to(DEV).requires_grad_(True)
    got = BiCrossEntropyLoss('mean')(zd, lab.to(DEV))
    got.backward()
    close32(got, want, 1e-5, 0, 'saturated bce value')
    close32(zd.grad, leaf.grad, 1e-4, 1e-6, 'saturated bce gradient')


# ================================================================================================ row losses of the two-stage head
def row_logits(R, C_, g):
    """Rows whose winning margin (label's logit minus the best other) is 0, small (0.01) and 15, in turn."""
    z = lr.logits((R, C_), g, lim=6.0)
    y = torch.randint(0, C_, (R,), generator=g)
    others = z.scatter(1, y.view(-1, 1), -1e30).max(1)[0]
    margin = torch.tensor([0.0, 0.01, 15.0])[torch.arange(R) % 3]
    keep = torch.arange(R) % 4 == 3                          # every fourth row stays random (the label need not win)
    z[torch.arange(R), y] = torch.where(keep, z[torch.arange(R), y], others + margin)
    return z, y


def check_rows(z, y, mode, gamma):
    from fastvision_amd.fc_ops import cross_entropy_mean, focal_mean
    R, C_ = z.shape
    res = {}
    for dt in (F64, F32):
        leaf = z.detach().to(dt).clone().requires_grad_(True)
        keep = {}
        v = lr.row_loss(leaf, y, mode, gamma, dt, keep)
        v.backward()
        res[dt] = (v.detach(), leaf.grad, keep)
    (v64, g64, k64), (v32, g32, k32) = res[F64], res[F32]
    logp, soft = k64['logp'].detach(), k64['soft'].detach()
    onehot = torch.zeros(R, C_, dtype=F64).scatter_(1, y.view(-1, 1), 1.0)
    zy = z.double().gather(1, y.view(-1, 1)).squeeze(1) - z.double().max(1)[0]
    if mode == 0:
        rmag = torch.stack([zy.abs(), torch.log(k64['den'].detach()).abs(), torch.ones(R, dtype=F64)]).amax(0)
        dmag = torch.ones(R, dtype=F64)
    else:
        # -(1 - p)^g log p, p = exp(log p): q = 1 - p carries p / q relative; d/dlogp = (g q^(g-1) log p - q^g / p) p, both terms with q's condition
        p = torch.exp(logp)
        q = (1 - p).clamp_min(1e-300)
        rmag = q ** gamma * (logp.abs() * (1 + gamma * p / q) + 1)
        dmag = (gamma * q ** (gamma - 1) * logp.abs() * p * (1 + (gamma - 1) * p / q) + q ** gamma * (1 + gamma * p / q))
    unit = (C_ + 6) * sm.EPS32                              # the kernel's softmax denominator: one chain of C fp32 additions
    rows32, rows64 = k32['rows'].detach().double(), k64['rows'].detach()
    vlim = (sm.FACTOR * (rows32 - rows64).abs() + unit * rmag).sum() / R + sm.EPS32 * v64.abs()
    glim = sm.FACTOR * (g32.double() - g64).abs() + unit * (dmag[:, None] * torch.maximum(onehot, soft) / R)
    zd = z.to(DEV).requires_grad_(True)
    got = cross_entropy_mean(zd, y.to(DEV)) if mode == 0 else focal_mean(zd, y.to(DEV), gamma)
    got.backward()
    return lr.worst(got, v64, vlim), lr.worst(zd.grad, g64, glim)


@pytest.mark.parametrize('R', [1, 255, 256, 257, 70000])
def test_row_losses(R):
    """Cross-entropy (fast.py) and the RPN's focal loss at its gamma = 2 (rpn.py:25; the only value the two-stage demo uses)."""
    w = {}
    for C_ in (2, 21, 81):
        g = torch.Generator().manual_seed(R * 100 + C_)
        z, y = row_logits(R, C_, g)
        w[f'ce C{C_} value'], w[f'ce C{C_} grad'] = check_rows(z, y, 0, 0.0)
        w[f'focal C{C_} value'], w[f'focal C{C_} grad'] = check_rows(z, y, 1, 2.0)
    report(f'row losses R {R}', **w)


def test_row_losses_saturated_logits():
    from fastvision_amd.fc_ops import cross_entropy_mean, focal_mean
    g = torch.Generator().manual_seed(174)
    z = saturate(lr.logits((300, 21), g), g)
    y = torch.randint(0, 21, (300,), generator=g)
    for mode in (0, 1):
        leaf = z.clone().requires_grad_(True)
        want = lr.row_loss(leaf, y, mode, 2.0, F32)
        want.backward()
        zd = z.to(DEV).requires_grad_(True)
        got = cross_entropy_mean(zd, y.to(DEV)) if mode == 0 else focal_mean(zd, y.to(DEV), 2.0)
        got.backward()
        close32(got, want, 1e-5, 0, f'saturated row loss {mode} value')
        close32(zd.grad, leaf.grad, 1e-4, 1e-6, f'saturated row loss {mode} gradient')


# ================================================================================================ smooth-L1
@pytest.mark.parametrize('n', [1, 255, 256, 257, 262144, 262145, 600000])
def test_smooth_l1(n):
    """Differences of exactly 0, +-1 and the fp32 neighbours of +-1 sit on b = 0, where a - b is exact: the branch |d| < 1 is then the same
    decision in fp32 and float64.  mag: the operands of a - b for the gradient (|d| < 1) or 1; value max(term, 1/2, |a|, |b|)."""
    from fastvision_amd.fc_ops import smooth_l1_mean
    g = torch.Generator().manual_seed(n)
    a, b = torch.randn(n, generator=g) * 1.5, torch.randn(n, generator=g)
    one = torch.tensor(1.0)
    special = torch.stack([torch.tensor(0.0), one, -one, torch.nextafter(one, torch.tensor(2.0)), torch.nextafter(one, torch.tensor(0.0)),
                           -torch.nextafter(one, torch.tensor(2.0)), -torch.nextafter(one, torch.tensor(0.0))])
    k = min(n, 7)
    a[:k], b[:k] = special[:k], 0.0
    res = {}
    for dt in (F64, F32):
        leaf = a.detach().to(dt).clone().requires_grad_(True)
        keep = {}
        v = lr.smooth_l1(leaf, b, dt, keep)
        v.backward()
        res[dt] = (v.detach(), leaf.grad, keep)
    (v64, g64, k64), (v32, g32, k32) = res[F64], res[F32]
    assert torch.equal(k64['d'].detach().abs() < 1, k32['d'].detach().abs() < 1)
    ab = torch.maximum(a.abs(), b.abs()).double()
    blocks = min((n + 255) // 256, lr.CONF_BLOCKS)
    vmag = torch.maximum(k64['terms'].detach(), ab).clamp_min(0.5)
    vlim = lr.scalar_limit(lr.chain_of(n, blocks * 256), k64['terms'], k32['terms'], vmag, n) + sm.EPS32 * v64.abs()
    glim = sm.limit_of(g64, g32, torch.where(k64['d'].detach().abs() < 1, ab, torch.ones_like(ab)) / n)
    ad = a.to(DEV).requires_grad_(True)
    got = smooth_l1_mean(ad, b.to(DEV))
    got.backward()
    report(f'smooth-L1 n {n}', value=lr.worst(got, v64, vlim), grad=lr.worst(ad.grad, g64, glim))


# ================================================================================================ IoU family
PAIR = [(0, 'xyxy', 0), (0, 'xywh', 0), (0, 'wh', 0), (1, 'xyxy', 0), (1, 'xywh', 0),
        (2, 'xyxy', 0), (2, 'xywh', 0), (2, 'xyxy', 1), (2, 'xywh', 1), (3, 'xyxy', 0), (3, 'xywh', 0), (3, 'xyxy', 1), (3, 'xywh', 1)]


def random_boxes(n, mode, g):
    wh = torch.rand(n, 2, generator=g) * 3 + 0.05
    c = torch.rand(n, 2, generator=g) * 4
    return wh if mode == 'wh' else torch.cat([c, wh], 1) if mode == 'xywh' else torch.cat([c - wh / 2, c + wh / 2], 1)


def surface(kind, mode, variant, batch):
    from fastvision_amd.detection.tools import IOU as L
    fn = L._batch if batch else L._pair
    return lambda a, b: fn(a, b, kind, mode, 1e-7, variant=variant)


def iou_limits(kind, mode, variant, a, b, batch):
    """(ref64, limit) of the values; pairwise also (grad64, limit) w.r.t. the first box.  mag = cond * (1 + |iou| + |rho^2 / c^2| + |alpha v|)
    (every piece is a quotient of conditioned differences, and (convex - union) / convex is good to cond * 2^-24 ABSOLUTE); gradient:
    cond * the sum of the |pieces| per corner (the IoU, GIoU and DIoU pieces with their quotient rules opened: loss_restatement.iou_open_grad_mag, term_open_grad_mag,
    and CIoU's alpha v with the cancelling difference of its arc tangents opened: av_open_grad_mag; GIoU's IoU
    uses plain areas, a 1e-7 difference in mag), a centre's gradient being the sum of its two corners'."""
    res = {}
    for dt in (F64, F32):
        leaf = a.to(dt).detach().clone().requires_grad_(not batch)
        v = lr.iou_any(kind, mode, variant, leaf, b, dt, batch=batch)
        gr = None if batch else torch.autograd.grad(v.sum(), leaf)[0]
        res[dt] = (v.detach(), gr)
    (v64, g64), (v32, g32) = res[F64], res[F32]
    if mode == 'wh':
        cond = torch.ones_like(v64)
    elif batch:
        cond = lr.box_condition(a[:, None, :], b[None, :, :], mode)
    else:
        cond = lr.box_condition(a, b, mode)
    pieces = [lr.iou_any(0 if mode == 'wh' else k, mode, variant, a, b, F64, batch=batch) for k in ((0,) if kind == 0 else (0, 2, 3) if kind == 3 else (0, kind))]
    mag = cond * (1 + sum(p.abs() for p in pieces))
    vl = sm.limit_of(v64, v32, mag)
    if batch:
        return v64, vl, None, None
    if mode == 'wh':
        gmag = lr.iou_open_grad_mag(a, b, 'wh', False)
    else:
        c4 = torch.stack(lr._corners(a.double(), mode), 1)
        t4 = torch.stack(lr._corners(b.double(), mode), 1)
        tot = torch.zeros_like(c4)
        for k in ((0,) if kind == 0 else (0, 2, 3) if kind == 3 else (0, kind)):
            tot = tot + (lr.iou_open_grad_mag(c4, t4, 'xyxy', True) if k == 0 else lr.term_open_grad_mag(k, variant, c4, t4) if k < 3 else lr.av_open_grad_mag(c4, t4))
        gmag = tot if mode == 'xyxy' else torch.stack([tot[:, 0] + tot[:, 2], tot[:, 1] + tot[:, 3], (tot[:, 0] + tot[:, 2]) / 2, (tot[:, 1] + tot[:, 3]) / 2], 1)
        gmag = gmag * cond[:, None]
    return v64, vl, g64, sm.limit_of(g64, g32, gmag)


@pytest.mark.parametrize('N', [1, 257, 600000])
def test_iou_pairwise_values_and_gradients(N):
    w = {}
    for kind, mode, variant in PAIR:
        g = torch.Generator().manual_seed(N + 10 * kind + variant)
        a, b = random_boxes(N, mode, g), random_boxes(N, mode, g)
        if N > 1:
            b[::3] = a[::3] * (1 + 0.05 * torch.randn(a[::3].shape, generator=g))      # a third overlaps heavily
        v64, vl, g64, gl = iou_limits(kind, mode, variant, a, b, False)
        ad = a.to(DEV).requires_grad_(True)
        got = surface(kind, mode, variant, False)(ad, b.to(DEV))
        got.sum().backward()
        w[f'k{kind} {mode} v{variant}'] = lr.worst(got, v64, vl)
        w[f'k{kind} {mode} v{variant} grad'] = lr.worst(ad.grad, g64, gl)
    report(f'IoU pairwise N {N}', **w)


def test_iou_batch_800_by_700():
    w = {}
    for kind, mode, variant in PAIR:
        g = torch.Generator().manual_seed(900 + 10 * kind + variant)
        a, b = random_boxes(800, mode, g), random_boxes(700, mode, g)
        v64, vl, _, _ = iou_limits(kind, mode, variant, a, b, True)
        got = surface(kind, mode, variant, True)(a.to(DEV), b.to(DEV))
        w[f'k{kind} {mode} v{variant}'] = lr.worst(got, v64, vl)
    report('IoU batch 800 x 700', **w)


DEGENERATE = torch.tensor([   # xyxy pairs: identical, disjoint, touching edges, nested, same centre, zero width (coordinates exact in fp32)
    [[1, 1, 3, 2], [1, 1, 3, 2]], [[0, 0, 1, 1], [2, 2, 3, 3]], [[0, 0, 1, 1], [1, 0, 2, 1]], [[0, 0, 4, 4], [1, 1, 2, 3]],
    [[1, 1, 3, 3], [0, 1.5, 4, 2.5]], [[1, 0, 1, 2], [0, 0, 2, 2]], [[1, 0, 1, 2], [1, 0, 1, 2]]], dtype=torch.float32)


def test_iou_degenerate_pairs():
    a, b = DEGENERATE[:, 0], DEGENERATE[:, 1]
    to = {'xyxy': lambda t: t, 'xywh': lambda t: torch.cat([(t[:, :2] + t[:, 2:]) / 2, t[:, 2:] - t[:, :2]], 1), 'wh': lambda t: t[:, 2:] - t[:, :2]}
    w = {}
    for kind, mode, variant in PAIR:
        pa, pb = to[mode](a), to[mode](b)
        for batch in (False, True):
            v64, vl, _, _ = iou_limits(kind, mode, variant, pa, pb, batch)
            got = surface(kind, mode, variant, batch)(pa.to(DEV), pb.to(DEV)).cpu().double().reshape(v64.shape)
            fin = torch.isfinite(v64)
            assert torch.equal(torch.isnan(got), torch.isnan(v64)) and torch.equal(torch.isinf(got), torch.isinf(v64)), (kind, mode, variant, batch)
            assert torch.equal(torch.sign(got[~fin & ~torch.isnan(v64)]), torch.sign(v64[~fin & ~torch.isnan(v64)]))
            w[f'k{kind} {mode} v{variant} {"batch" if batch else "pair"}'] = lr.worst(got[fin], v64[fin], vl[fin])
    report('IoU degenerate pairs', **w)


# ================================================================================================ in-place gradient scale
@pytest.mark.parametrize('n', [1, 2, 3, 4, 5, 1023, 4 * 256 * 2048 + 3])
def test_scale_by_device_scalar(n):
    """Vector body, the n & 3 tail and the early exit at exactly 1.0; buffers straight from torch.empty (16-byte aligned, as the callers
    guarantee)."""
    from fastvision_amd import _lib
    from fastvision_amd.ops import _p, _stream
    g = torch.Generator().manual_seed(n)
    src = torch.randn(n, generator=g)
    x = torch.empty(n, dtype=F32, device=DEV)
    assert x.data_ptr() % 16 == 0
    x.copy_(src)
    _lib.call('fva_scale_by_device_scalar', _p(x), n, _p(torch.tensor([0.5], device=DEV)), _stream())
    assert torch.equal(x.cpu(), src * 0.5)
    src[0] = float('nan')
    src[-1] = -0.0
    x.copy_(src)
    _lib.call('fva_scale_by_device_scalar', _p(x), n, _p(torch.tensor([1.0], device=DEV)), _stream())
    assert torch.equal(x.cpu().view(torch.int32), src.view(torch.int32))
