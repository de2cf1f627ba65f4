"""The loss formulas of csrc/loss.hip, written once with plain differentiable torch ops and parameterised by ``dt`` (torch.float64: the
reference of tests/test_gpu_losses.py; torch.float32: e32, what an honest fp32 evaluation costs) in the manner of
streaming_measure.silu_apply.  torch.autograd on the float64 evaluation is the reference gradient.  Not a test module (pytest does not
collect it); tests/test_loss_restatement_cpu.py pins it without a GPU against oracle/losses.py and torch.nn.functional.  Written from the
formulas quoted in the comments of loss.hip; imports nothing but torch and the measure (tests/streaming_measure.py).

Python scalars (1e-8, 1e-7, 4 / pi^2) are used as they stand: torch rounds them to ``dt``, so the fp32 evaluation works with the constants
the kernels hold and the float64 one with the exact ones (the difference is part of e32).

Every function returns plain tensors of dtype ``dt``; the ``keep`` dictionaries carry the intermediate terms from which the GPU tests build
``mag`` and the sum limits.  ``wrong`` selects a deliberately wrong variant (tests/test_loss_restatement_cpu.py shows that the measure
rejects each of them); '' is the formula.
"""
import math

import torch

import streaming_measure as sm

BCE_EPS = 1e-8
IOU_EPS = 1e-7


# ---------------------------------------------------------------------------------------------------------------- IoU family
def _corners(b, mode):
    if mode == 'xywh':                                   # BOX.py:4-10
        hw, hh = b[..., 2] / 2, b[..., 3] / 2
        return b[..., 0] - hw, b[..., 1] - hh, b[..., 0] + hw, b[..., 1] + hh
    return b[..., 0], b[..., 1], b[..., 2], b[..., 3]


def iou_any(kind, mode, variant, a, b, dt, eps=IOU_EPS, batch=False):
    """kind 0 IoU / 1 GIoU / 2 DIoU / 3 CIoU; mode 'xyxy' / 'xywh' / 'wh' (IoU only); variant 0 library / 1 demo (centre sums not
    halved, minus sign).  Pairwise ([N, w] x [N, w] -> [N]) or batch ([N, w] x [M, w] -> [N, M]).  The reference's quirks: the pairwise
    IoU carries eps inside the height factor of both areas, the batch forms and GIoU use plain areas; library DIoU = iou + rho^2 / c^2;
    GIoU_batch = iou + (convex - union) / convex; CIoU's alpha is a constant (no_grad)."""
    a, b = a.to(dt), b.to(dt)
    if batch:
        a, b = a[:, None, :], b[None, :, :]
    if mode == 'wh':
        inter = torch.minimum(a[..., 0], b[..., 0]) * torch.minimum(a[..., 1], b[..., 1])
        return inter / (a[..., 0] * a[..., 1] + b[..., 0] * b[..., 1] - inter + eps)
    ax1, ay1, ax2, ay2 = _corners(a, mode)
    bx1, by1, bx2, by2 = _corners(b, mode)
    iw = (torch.minimum(ax2, bx2) - torch.maximum(ax1, bx1)).clamp(0)
    ih = (torch.minimum(ay2, by2) - torch.maximum(ay1, by1)).clamp(0)
    inter = iw * ih
    uni_plain = (ax2 - ax1) * (ay2 - ay1) + (bx2 - bx1) * (by2 - by1) - inter + eps
    uni_quirk = (ax2 - ax1) * (ay2 - ay1 + eps) + (bx2 - bx1) * (by2 - by1 + eps) - inter + eps
    cw = torch.maximum(ax2, bx2) - torch.minimum(ax1, bx1)
    ch = torch.maximum(ay2, by2) - torch.minimum(ay1, by1)
    if kind == 0:
        return inter / (uni_plain if batch else uni_quirk)
    if kind == 1:
        convex = cw * ch + eps
        term = (convex - uni_plain) / convex
        return inter / uni_plain + term if batch else inter / uni_plain - term
    iou = inter / (uni_plain if batch else uni_quirk)
    c2 = cw ** 2 + ch ** 2 + eps
    cxa, cya, cxb, cyb = ax1 + ax2, ay1 + ay2, bx1 + bx2, by1 + by2
    if not variant:
        cxa, cya, cxb, cyb = cxa * 0.5, cya * 0.5, cxb * 0.5, cyb * 0.5
    term = ((cxa - cxb) ** 2 + (cya - cyb) ** 2) / c2
    diou = iou - term if variant else iou + term
    if kind == 2:
        return diou
    wa, ha, wb, hb = ax2 - ax1, ay2 - ay1, bx2 - bx1, by2 - by1
    v = (4 / math.pi ** 2) * torch.pow(torch.atan(wb / (hb + eps)) - torch.atan(wa / (ha + eps)), 2)
    alpha = (v / (v - iou + (1 + eps))).detach()
    return diou - alpha * v


def iou_open_grad_mag(a, b, mode, quirk):
    """Per-parameter mag of d IoU / d a (a: 'xyxy' corners [N, 4] or 'wh' sizes [N, 2]; float64): the quotient rule opened up,
    d (I / U) = dI / U - (I / U) (dA - dI) / U  ->  (|dI| + iou * (|dA| + |dI|)) / U,  I the intersection, A the first box's area (with the
    pairwise form's eps in its height when quirk), U the union: where dI / U and iou * dU / U cancel, |d IoU| alone would understate what
    the terms of the last subtraction carry."""
    a = a.detach().double().clone().requires_grad_(True)
    b = b.detach().double()
    if mode == 'wh':
        inter = torch.minimum(a[:, 0], b[:, 0]) * torch.minimum(a[:, 1], b[:, 1])
        area_a, area_b = a[:, 0] * a[:, 1], b[:, 0] * b[:, 1]
    else:
        iw = (torch.minimum(a[:, 2], b[:, 2]) - torch.maximum(a[:, 0], b[:, 0])).clamp(0)
        ih = (torch.minimum(a[:, 3], b[:, 3]) - torch.maximum(a[:, 1], b[:, 1])).clamp(0)
        inter = iw * ih
        e = IOU_EPS if quirk else 0.0
        area_a, area_b = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1] + e), (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1] + e)
    uni = (area_a + area_b - inter + IOU_EPS).detach()
    d_i, = torch.autograd.grad(inter.sum(), a, retain_graph=True)
    d_a, = torch.autograd.grad(area_a.sum(), a)
    iou = (inter.detach() / uni)[:, None]
    return (d_i.abs() + iou * (d_a.abs() + d_i.abs())) / uni[:, None]


def term_open_grad_mag(kind, variant, a, b):
    """The same for the second piece of GIoU and DIoU w.r.t. the first box's 'xyxy' corners [N, 4] (float64):
    GIoU  (C - U) / C, C the hull's area:  ((dC - dU) - term dC) / C  ->  (|dC| + |dA| + |dI| + |term| |dC|) / C  (C - U cancels where the
          boxes nearly coincide, and so does dC - dU);
    DIoU  rho^2 / c^2:  (d rho^2 - term d c^2) / c^2  ->  (|d rho^2| + term |d c^2|) / c^2."""
    a = a.detach().double().clone().requires_grad_(True)
    b = b.detach().double()
    grad = lambda y: torch.autograd.grad(y.sum(), a, retain_graph=True)[0].abs()
    cw = torch.maximum(a[:, 2], b[:, 2]) - torch.minimum(a[:, 0], b[:, 0])
    ch = torch.maximum(a[:, 3], b[:, 3]) - torch.minimum(a[:, 1], b[:, 1])
    if kind == 1:
        iw = (torch.minimum(a[:, 2], b[:, 2]) - torch.maximum(a[:, 0], b[:, 0])).clamp(0)
        ih = (torch.minimum(a[:, 3], b[:, 3]) - torch.maximum(a[:, 1], b[:, 1])).clamp(0)
        inter = iw * ih
        area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
        uni = area_a + (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]) - inter + IOU_EPS
        convex = cw * ch + IOU_EPS
        term = ((convex - uni) / convex).detach().abs()[:, None]
        return (grad(convex) * (1 + term) + grad(area_a) + grad(inter)) / convex.detach()[:, None]
    c2 = cw ** 2 + ch ** 2 + IOU_EPS
    k = 1.0 if variant else 0.5
    rho2 = (k * (a[:, 0] + a[:, 2]) - k * (b[:, 0] + b[:, 2])) ** 2 + (k * (a[:, 1] + a[:, 3]) - k * (b[:, 1] + b[:, 3])) ** 2
    term = (rho2 / c2).detach()[:, None]
    return (grad(rho2) + term * grad(c2)) / c2.detach()[:, None]


def av_open_grad_mag(a, b):
    """The same for CIoU's third piece alpha * v, v = (4 / pi^2) D^2, D = atan(wb / (hb + eps)) - atan(wa / (ha + eps)), alpha a constant:
    d (alpha v) = alpha (8 / pi^2) D dD.  D is a difference of two arc tangents that nearly cancel where the boxes have nearly the same
    aspect ratio: it carries 2^-24 * (|atan_a| + |atan_b|) of absolute error, so the product is good to
    alpha (8 / pi^2) (|atan_a| + |atan_b|) |dD|, not to 2^-24 of itself."""
    a = a.detach().double().clone().requires_grad_(True)
    b = b.detach().double()
    ta = torch.atan((a[:, 2] - a[:, 0]) / (a[:, 3] - a[:, 1] + IOU_EPS))
    tb = torch.atan((b[:, 2] - b[:, 0]) / (b[:, 3] - b[:, 1] + IOU_EPS))
    d_ta, = torch.autograd.grad(ta.sum(), a)
    v = (4 / math.pi ** 2) * (tb - ta.detach()) ** 2
    iou = iou_any(0, 'xyxy', 0, a.detach(), b, torch.float64)
    alpha = v / (v - iou + (1 + IOU_EPS))
    return (alpha * (8 / math.pi ** 2) * (ta.detach().abs() + tb.abs()))[:, None] * d_ta.abs()


def box_condition(a, b, mode):
    """Condition of the edge differences behind an IoU of the pair (float64, no gradient): the largest |corner coordinate| over the
    smallest POSITIVE difference among the widths and heights of both boxes, of their intersection and of their convex hull (a
    difference d of two fp32 corners of size c carries 2^-24 * c of absolute, c / d of relative error), at least 1."""
    a, b = a.detach().double(), b.detach().double()
    a, b = torch.broadcast_tensors(a, b)
    A, Bx = _corners(a, mode), _corners(b, mode)
    big = torch.stack([c.abs() for c in A + Bx]).amax(0)
    ds = [A[2] - A[0], A[3] - A[1], Bx[2] - Bx[0], Bx[3] - Bx[1],
          torch.minimum(A[2], Bx[2]) - torch.maximum(A[0], Bx[0]), torch.minimum(A[3], Bx[3]) - torch.maximum(A[1], Bx[1]),
          torch.maximum(A[2], Bx[2]) - torch.minimum(A[0], Bx[0]), torch.maximum(A[3], Bx[3]) - torch.minimum(A[1], Bx[1])]
    d = torch.stack([torch.where(x > 0, x, torch.full_like(x, float('inf'))) for x in ds]).amin(0)
    return (big / d).clamp_min(1.0)


# ---------------------------------------------------------------------------------------------------------------- BCE on probabilities
def bce_prob_terms(p, t, wrong=''):
    """-t log(p + 1e-8) - (1 - t) log(1 - p + 1e-8), element-wise (classification_loss.py:54)."""
    if wrong == 'eps_outside':
        return -t * (torch.log(p) + BCE_EPS) - (1 - t) * (torch.log(1 - p) + BCE_EPS)
    return -t * torch.log(p + BCE_EPS) - (1 - t) * torch.log(1 - p + BCE_EPS)


def bce_prob_mag(p, t):
    """mag of one BCE term and of its gradient factor dl/dp * p (1 - p), float64 tensors without gradient.
    Value: the two products of the subtraction, and what the logs inherit from their arguments: p + 1e-8 is good to 2^-24 relative (1 of
    absolute error in the log), 1 - p + 1e-8 carries p's 2^-24 * p of absolute error, p / (1 - p + 1e-8) relative (that much absolute
    error in the log).  Gradient dl/dp * p (1 - p) = -t (1 - p) p / (p + eps) + (1 - t) p (1 - p) / (1 - p + eps): the two terms of the
    addition, the second times the condition 1 / (1 - p + 1e-8) of its 1 - p."""
    p, t = p.detach().double(), t.detach().double()
    c = 1.0 / (1 - p + BCE_EPS)
    val = torch.stack([(t * torch.log(p + BCE_EPS)).abs(), ((1 - t) * torch.log(1 - p + BCE_EPS)).abs(), t.abs(), (1 - t).abs() * p * c]).amax(0)
    grad = torch.maximum(t.abs() * (1 - p) * p / (p + BCE_EPS), (1 - t).abs() * p * (1 - p) * c * c)
    return val, grad


def bce(y, target, C, dt, weights=None, already_sigmoid=False, mean=True, keep=None):
    """Stand-alone BiCrossEntropyLoss (classification_loss.py:36-65).  y: any shape, numel = rows * C; target: integer labels [rows] when it
    is an integer tensor (one-hot over C), else a dense float target of y's numel; weights: None, 1 or numel values."""
    y = y.to(dt).reshape(-1)
    if target.is_floating_point():
        t = target.to(dt).reshape(-1)
    else:
        t = torch.zeros(y.numel() // C, C, dtype=dt).scatter_(1, target.reshape(-1, 1).long(), 1.0).reshape(-1)
    p = y if already_sigmoid else torch.sigmoid(y)
    terms = bce_prob_terms(p, t)
    if weights is not None:
        terms = terms * weights.to(dt).reshape(-1)
    if keep is not None:
        keep.update(p=p, t=t, terms=terms)
    return terms.sum() / y.numel() if mean else terms.sum()


# ---------------------------------------------------------------------------------------------------------------- two-stage head
def row_loss(logits, labels, mode, gamma, dt, keep=None):
    """mode 0: F.cross_entropy(mean); mode 1: mean of -(1 - p_t)^gamma log p_t, p = softmax (rpn.py:8-64)."""
    z = logits.to(dt)
    m = z.max(1, keepdim=True)[0].detach()
    den = torch.exp(z - m).sum(1)
    logp = (z.gather(1, labels.view(-1, 1).long()) - m).squeeze(1) - torch.log(den)
    rows = -logp if mode == 0 else -torch.pow(1 - torch.exp(logp), gamma) * logp
    if keep is not None:
        keep.update(rows=rows, logp=logp, den=den, soft=torch.exp(z - m) / den[:, None])
    return rows.mean()


def smooth_l1(a, b, dt, keep=None):
    """F.smooth_l1_loss(a, b, reduction='mean'), beta = 1."""
    d = a.to(dt) - b.to(dt)
    ad = d.abs()
    terms = torch.where(ad < 1, 0.5 * d * d, ad - 0.5)
    if keep is not None:
        keep.update(terms=terms, d=d)
    return terms.sum() / d.numel()


# ---------------------------------------------------------------------------------------------------------------- library loss
def last_write_mask(cell, ncell, first=False):
    """True for the match that index_put leaves in its cell: the LAST of the matches that share it (first=True: the wrong variant)."""
    order = torch.arange(cell.numel())
    if first:
        win = torch.full((ncell,), cell.numel(), dtype=torch.long).scatter_reduce(0, cell, order, 'amin')
    else:
        win = torch.full((ncell,), -1, dtype=torch.long).scatter_reduce(0, cell, order, 'amax')
    return win[cell] == order


def yolov3_terms(heads, matches, anchors, ratios, dt, norm_counts=None, norm_batch=None, keep=None, wrong=''):
    """Yolov3Loss.forward (yolov3_loss.py:29-72) on given matches.  heads: per level [B, A, H, W, 5 + C]; matches: per level
    (b, gx, gy, a, cls, xywh) as build_target returns them (int64 [M] x 5, fp32 [M, 4] = offsets and feature-scale sizes); anchors: per
    level the matched feature-scale anchors [M, 2]; ratios = (box, conf, cls).  Returns (total, box, conf, cls), scalars of dtype dt.
      class term:  sum of BCE(sigmoid(z_cls), one-hot) over the matches / (n * C)
      box term:    sum of 1 - CIoU(pred, target; xywh) / n,  pred = (sigmoid(z_xy), exp(z_wh) * anchor)
      objectness:  sum over EVERY cell of BCE(sigmoid(z_4), tau) / ncell,  tau = IoU(pred, target) of the LAST match in the cell, else 0;
                   tau is NOT detached, and (index_put's backward) every match of a cell receives the cell's d loss / d tau
      total = (box * r_box + conf * r_conf + cls * r_cls) * B
    Data parallel (norm_counts [levels], norm_batch): n is the job's match count, and
      total = (box * r_box + cls * r_cls) * norm_batch + conf * r_conf * B   (this rank's share; the cell mean is local).
    keep: a list that receives one dict of intermediate terms per level."""
    rb, rc, rcl = ratios
    zero = torch.zeros((), dtype=dt)
    l_box, l_conf, l_cls = zero, zero, zero
    B = heads[0].shape[0]
    for lvl, head in enumerate(heads):
        h = head.to(dt)
        Bh, A, H, W, K = h.shape
        C = K - 5
        b, gx, gy, a, cls, xywh = matches[lvl]
        n = b.numel()
        nn = int(norm_counts[lvl]) if norm_counts is not None else n
        ncell = Bh * A * H * W
        tau = torch.zeros(ncell, dtype=dt)
        info = dict(n=n, nn=nn, ncell=ncell, C=C)
        if n > 0 and nn > 0:
            rows = h[b, a, gy, gx]
            if keep is not None:
                rows.retain_grad() if rows.requires_grad else None
            pc = torch.sigmoid(rows[:, 5:])
            onehot = torch.zeros(n, C, dtype=dt).scatter_(1, cls.view(-1, 1), 1.0)
            cls_terms = bce_prob_terms(pc, onehot, wrong)
            l_cls = l_cls + cls_terms.sum() / (nn if wrong == 'cls_mean_n' else nn * C)
            pbox = torch.cat([torch.sigmoid(rows[:, 0:2]), torch.exp(rows[:, 2:4]) * anchors[lvl].to(dt)], 1)
            tbox = xywh.to(dt)
            box_terms = 1 - iou_any(3, 'xywh', 0, pbox, tbox, dt)
            l_box = l_box + box_terms.sum() / nn
            iou = iou_any(0, 'xywh', 0, pbox, tbox, dt)
            if wrong == 'detach_iou':
                iou = iou.detach()
            cell = ((b * A + a) * H + gy) * W + gx
            win = last_write_mask(cell, ncell, first=(wrong == 'first_write'))
            tau = tau.index_add(0, cell, torch.where(win, iou, iou - iou.detach()))
            info.update(rows=rows, pc=pc, onehot=onehot, cls_terms=cls_terms, pbox=pbox, tbox=tbox, box_terms=box_terms, iou=iou, cell=cell, win=win)
        po = torch.sigmoid(h[..., 4]).reshape(-1)
        conf_terms = bce_prob_terms(po, tau, wrong)
        l_conf = l_conf + conf_terms.sum() / ncell
        info.update(po=po, tau=tau, conf_terms=conf_terms)
        if keep is not None:
            keep.append(info)
    if norm_counts is None:
        total = (l_box * rb + l_conf * rc + l_cls * rcl) * B
    else:
        total = (l_box * rb + l_cls * rcl) * norm_batch + l_conf * rc * (norm_batch if wrong == 'conf_job_batch' else B)
    return total, l_box, l_conf, l_cls


# ---------------------------------------------------------------------------------------------------------------- demo loss
def bce_logits_terms(z, t):
    """F.binary_cross_entropy_with_logits, element-wise: max(z, 0) - z t + log(1 + exp(-|z|))."""
    return z.clamp(min=0) - z * t + torch.log1p(torch.exp(-z.abs()))


def demo_terms(layers, targets, anchors, dt, keep=None):
    """ComputeLoss.forward (demos/yolov3_u/utils/lossv3.py:18-119).  layers: per level raw [B, A * (5 + C), H, W]; targets [T, 6] fp32 =
    (image, class, xc, yc, w, h) normalised; anchors: per level [A, 2] feature scale.  Returns (total, (xy, wh, cls, conf), undecidable).
      per target: best anchor = FIRST maximum of wh-IoU(target size, anchors); cell = floor(target centre)
        xy:  BCE-with-logits(z_xy, centre - cell), mean over 2T;  wh: (z_wh - log(size / anchor + 1e-14))^2, mean over 2T
        cls: BCE-with-logits(z_cls, one-hot), mean over T * C
      mask: a predicted box whose best IoU with the targets of its image is > 0.5 is ignored (-1), positives (cell, best anchor) override: 1
      conf: BCE-with-logits(z_4, mask) over the cells with mask != -1, mean over their number
      total = 2 xy + wh + cls + conf
    The discrete decisions (arg-max, iou > 0.5) are evaluated in float64 whatever dt is: dt only changes the arithmetic of the terms.
    undecidable = number of cells with |best IoU - 0.5| < 1e-4 plus number of (target, level) whose two best anchor IoUs differ by less
    than 1e-6: a condition on the inputs (it must be 0), not a tolerance."""
    T = targets.shape[0]
    zero = torch.zeros((), dtype=dt)
    l_xy, l_wh, l_cls, l_conf = zero, zero, zero, zero
    undecidable = 0
    for lvl, raw in enumerate(layers):
        anc64 = anchors[lvl].double()
        A = anc64.shape[0]
        Bn, ch, H, W = raw.shape
        K = ch // A
        C = K - 5
        pred = raw.to(dt).permute(0, 2, 3, 1).reshape(Bn, H, W, A, K)
        # ---- decisions, float64 on the fp32 operands the kernel forms (target * grid size in fp32)
        tg32 = targets.float() * torch.tensor([1, 1, W, H, W, H], dtype=torch.float32)
        tg = tg32.double()
        aiou = iou_any(0, 'wh', 0, tg[:, 4:6], anc64, torch.float64, batch=True)
        best = aiou.max(1)[1]
        if A > 1:
            top = aiou.topk(2, dim=1)[0]
            undecidable += int(((top[:, 0] - top[:, 1]) < 1e-6).sum())
        gxy = torch.floor(tg[:, 2:4])
        bi, gx, gy = tg[:, 0].long(), gxy[:, 0].long(), gxy[:, 1].long()
        p64 = pred.detach().double()
        cellxy = torch.stack(torch.meshgrid(torch.arange(H), torch.arange(W), indexing='ij')[::-1], -1).double().view(1, H, W, 1, 2)
        pbox = torch.cat([torch.sigmoid(p64[..., 0:2]) + cellxy, torch.exp(p64[..., 2:4]) * anc64.view(1, 1, 1, A, 2)], -1)
        mask = torch.zeros(Bn, H, W, A, dtype=dt)
        for img in range(Bn):
            t_img = tg[bi == img][:, 2:6]
            if t_img.shape[0] == 0:
                continue
            flat = pbox[img].reshape(-1, 4)
            bestiou = torch.full((flat.shape[0],), -1.0, dtype=torch.float64)
            for s in range(0, t_img.shape[0], 64):
                bestiou = torch.maximum(bestiou, iou_any(0, 'xywh', 0, flat, t_img[s:s + 64], torch.float64, batch=True).max(1)[0])
            undecidable += int(((bestiou - 0.5).abs() < 1e-4).sum())
            mask[img] = torch.where(bestiou > 0.5, -1.0, 0.0).to(dt).view(H, W, A)
        mask[bi, gy, gx, best] = 1
        valid = mask != -1
        # ---- terms in dt
        tgd = tg32.to(dt)
        rows = pred[bi, gy, gx, best]
        if keep is not None and rows.requires_grad:
            rows.retain_grad()
        off = tgd[:, 2:4] - gxy.to(dt)
        twh = torch.log(tgd[:, 4:6] / anchors[lvl].to(dt)[best] + 1e-14)
        onehot = torch.zeros(T, C, dtype=dt).scatter_(1, tg[:, 1].long().view(-1, 1), 1.0)
        xy_terms = bce_logits_terms(rows[:, 0:2], off)
        wh_terms = (rows[:, 2:4] - twh) ** 2
        cls_terms = bce_logits_terms(rows[:, 5:], onehot)
        zo = pred[..., 4]
        conf_terms = torch.where(valid, bce_logits_terms(zo, mask), torch.zeros_like(zo))
        nvalid = int(valid.sum())
        l_xy = l_xy + xy_terms.sum() / (2 * T)
        l_wh = l_wh + wh_terms.sum() / (2 * T)
        l_cls = l_cls + cls_terms.sum() / (T * C)
        l_conf = l_conf + conf_terms.sum() / nvalid
        if keep is not None:
            keep.append(dict(rows=rows, off=off, twh=twh, onehot=onehot, xy_terms=xy_terms, wh_terms=wh_terms, cls_terms=cls_terms,
                             conf_terms=conf_terms, mask=mask, valid=valid, nvalid=nvalid, zo=zo, T=T, C=C, A=A,
                             cell=((bi * H + gy) * W + gx) * A + best))
    total = l_xy * 2.0 + l_wh + l_cls + l_conf
    return total, (l_xy, l_wh, l_cls, l_conf), undecidable


# ---------------------------------------------------------------------------------------------------------------- the measure
# limit = FACTOR * (e32 + 2^-24 * mag) per element (streaming_measure.limit_of), plus sum_limit(m, sum |term|) where the kernel adds m > 1
# terms with atomicAdd in unspecified order.  Scalars: sum_limit(n, sum |term|, sum e32) + FACTOR * 2^-24 * sum mag(term), n = the longest
# chain of fp32 additions in the code (the thread's own chain + 64 for the wave + 4 for the block; the partials are added in double).
F64, F32 = torch.float64, torch.float32
CONF_BLOCKS = 1024


def chain_of(n_items, per_pass):
    """Longest fp32 chain of a grid-stride sum: items a thread adds + 64 (wave) + 4 (block)."""
    return -(-n_items // per_pass) + 64 + 4


def scalar_limit(n, t64, t32, mag, denom):
    """Limit of sum(terms) / denom."""
    t64 = t64.detach().double()
    return (sm.sum_limit(n, t64.abs().sum(), (t32.detach().double() - t64).abs().sum()) + sm.FACTOR * sm.EPS32 * mag.double().sum()) / denom


def _cell_scatter(shape, idx, val):
    """Sum of val [M, k] into zeros(shape + (k,)) at the cells idx (tuple of index vectors)."""
    out = torch.zeros(*shape, val.shape[1], dtype=torch.float64)
    return out.index_put(idx, val.double(), accumulate=True)


def yolov3_reference(heads, matches, anchors, ratios, norm_counts=None, norm_batch=None, wrong32=''):
    """Float64 reference, fp32 evaluation and limits of the library loss on CPU copies of the operands.  Returns a dict:
    vals64 / vals32 (total, box, conf, cls), grads64 / grads32 per level, val_limits [4], grad_limits per level.
      mag, objectness column (conf_kernel, a plain store):  g * p (1 - p) * max(t / (p + eps), (1 - t) / (1 - p + eps)^2), g = r_conf B / ncell
        (bce_prob_mag: the two terms of the addition, the second times the condition of its 1 - p).
      mag, class columns, per match: the same with g = r_cls Bn / (n C).
      mag, box columns, per match: cond * (|gtau dIoU| + gb (|dIoU| + |d rho^2/c^2| + |d alpha v|)) * dp/dz, the terms of
        (gtau * iou.d - gb * ciou.d) with CIoU's own three-term sum and the IoU's quotient rule (iou_open_grad_mag) opened up; cond = box_condition (edge differences) and, for the xy
        columns, 1 / (1 - p) of the sigmoid derivative p (1 - p).  Each |d . / d x| is |d . / d x1| + |d . / d x2| (and |d . / d w| half of it):
        reverse-mode autograd, the reference's arithmetic, forms the centre's gradient as the last addition of the two CORNER gradients,
        which cancel where one box contains the other (found on the CPU: the oracle's fp32 x-gradient of a prediction that contains its
        target is 2.8e-5 off, 600 times the corner terms' 2^-24; the kernel's forward-mode duals do not have this cancellation).
      Elements that m > 1 matches add into (atomicAdd) additionally get sum_limit(m, sum |term|)."""
    rb, rc, rcl = ratios
    res = {}
    for dt, wrong in ((F64, ''), (F32, wrong32)):
        leaves = [h.detach().to(dt).requires_grad_(True) for h in heads]
        keep = []
        vals = yolov3_terms(leaves, matches, anchors, ratios, dt, norm_counts, norm_batch, keep=keep, wrong=wrong)
        vals[0].backward()
        res[dt] = ([v.detach() for v in vals], [l.grad for l in leaves], keep)
    (v64, g64, k64), (v32, g32, k32) = res[F64], res[F32]
    B = heads[0].shape[0]
    Bn = norm_batch if norm_counts is not None else B
    lim_box = lim_conf = lim_cls = torch.zeros((), dtype=F64)
    grad_limits = []
    for lvl, (i64, i32) in enumerate(zip(k64, k32)):
        Bh, A, H, W, K = heads[lvl].shape
        n, nn, ncell, C = i64['n'], i64['nn'], i64['ncell'], i64['C']
        mag = torch.zeros(Bh, A, H, W, K, dtype=F64)
        extra = torch.zeros(Bh, A, H, W, K, dtype=F64)
        g = rc * B / ncell
        vmag, gmag = bce_prob_mag(i64['po'], i64['tau'])
        mag[..., 4] = (g * gmag).view(Bh, A, H, W)
        blocks = min((ncell + 255) // 256, CONF_BLOCKS)
        lim_conf = lim_conf + scalar_limit(chain_of(ncell, blocks * 256), i64['conf_terms'], i32['conf_terms'], vmag, ncell)
        if 'rows' in i64:
            b, gx, gy, a, cls, xywh = matches[lvl]
            idx = (b, a, gy, gx)
            vm, gm = bce_prob_mag(i64['pc'], i64['onehot'])
            lim_cls = lim_cls + scalar_limit(chain_of(C, 64), i64['cls_terms'], i32['cls_terms'], vm, nn * C)
            cond = box_condition(i64['pbox'], i64['tbox'], 'xywh')
            lim_box = lim_box + scalar_limit(1, i64['box_terms'], i32['box_terms'], cond * i64['box_terms'].detach().abs().clamp_min(1.0), nn)
            # per-match pieces of the box gradient
            pbd = i64['pbox'].detach()
            pc4 = torch.stack(_corners(pbd, 'xywh'), 1).requires_grad_(True)
            tc4 = torch.stack(_corners(i64['tbox'].detach(), 'xywh'), 1)
            diou = iou_any(2, 'xyxy', 0, pc4, tc4, F64)
            ciou = iou_any(3, 'xyxy', 0, pc4, tc4, F64)
            d_av, = torch.autograd.grad((diou - ciou).sum(), pc4)
            fold = lambda d: torch.stack([d[:, 0].abs() + d[:, 2].abs(), d[:, 1].abs() + d[:, 3].abs(),
                                          (d[:, 0].abs() + d[:, 2].abs()) / 2, (d[:, 1].abs() + d[:, 3].abs()) / 2], 1)
            d_iou, d_term, d_av = fold(iou_open_grad_mag(pc4, tc4, 'xyxy', True)), fold(term_open_grad_mag(2, 0, pc4, tc4)), fold(d_av)
            po = i64['po'].detach()[i64['cell']]
            gtau = (g * (-torch.log(po + BCE_EPS) + torch.log(1 - po + BCE_EPS))).abs()[:, None]
            gb = rb * Bn / nn
            dpdz = torch.cat([pbd[:, :2] * (1 - pbd[:, :2]), pbd[:, 2:]], 1)
            cxy = torch.cat([1 / (1 - pbd[:, :2]), torch.ones_like(pbd[:, 2:])], 1)
            bmag = cond[:, None] * cxy * (gtau * d_iou.abs() + gb * (d_iou.abs() + d_term.abs() + d_av.abs())) * dpdz
            cmag = (rcl * Bn / (nn * C)) * gm
            mmag = torch.cat([bmag, torch.zeros(n, 1, dtype=F64), cmag], 1)
            terms = i64['rows'].grad.double().abs()
            mag = mag + _cell_scatter((Bh, A, H, W), idx, mmag)
            cnt = _cell_scatter((Bh, A, H, W), idx, torch.ones(n, 1))
            tsum = _cell_scatter((Bh, A, H, W), idx, terms)
            extra = torch.where(cnt > 1, sm.sum_limit(1, tsum) + (cnt - 1) * sm.EPS32 * tsum, torch.zeros_like(tsum))   # = sum_limit(m, tsum)
            extra[..., 4] = 0
        grad_limits.append(sm.limit_of(g64[lvl], g32[lvl], mag) + extra)
    if norm_counts is None:
        lim_total = (lim_box * rb + lim_conf * rc + lim_cls * rcl) * B
    else:
        lim_total = (lim_box * rb + lim_cls * rcl) * norm_batch + lim_conf * rc * B
    lims = [lim_total + 4 * sm.EPS32 * v64[0].abs(), lim_box + sm.EPS32 * v64[1].abs(), lim_conf + sm.EPS32 * v64[2].abs(),
            lim_cls + sm.EPS32 * v64[3].abs()]
    return dict(vals64=torch.stack(v64), vals32=torch.stack(v32).double(), grads64=g64, grads32=g32, val_limits=torch.stack(lims),
                grad_limits=grad_limits)


def worst(got, ref64, limit):
    """Largest err / limit (streaming_measure.worst_f32) of a CPU copy of a device result."""
    return sm.worst_f32(got.detach().cpu().float().reshape(ref64.shape), ref64, limit)


def demo_reference(layers, targets, anchors):
    """The same for the demo loss: vals64 / vals32 (total, xy, wh, cls, conf), grads64 / grads32 per level, val_limits [5], grad_limits,
    undecidable, masks (per level [B, H, W, A]).
      mag of BCE-with-logits max(z, 0) - z t + log1p(exp(-|z|)): max(|z|, |z t|, 1) (the log1p is good to its own rounding, at most log 2).
      mag of its gradient (sigmoid(z) - t) * g: g * max(p, |t|).   mag of the wh gradient 2 (z - twh) * g: g * 2 * max(|z|, |twh|, 1): twh is a
      logarithm of an fp32 quotient, good to 2^-24 absolute.  Objectness: (sigmoid(z) - mask) / nvalid, a plain store; ignored cells exactly 0.
      The xy / wh / class gradients are atomicAdd'ed per target: sum_limit(m, sum |term|) where m > 1 targets share (cell, anchor)."""
    res = {}
    for dt in (F64, F32):
        leaves = [h.detach().to(dt).requires_grad_(True) for h in layers]
        keep = []
        total, parts, und = demo_terms(leaves, targets, anchors, dt, keep=keep)
        total.backward()
        res[dt] = ([total.detach()] + [p.detach() for p in parts], [l.grad for l in leaves], keep, und)
    (v64, g64, k64, und), (v32, g32, k32, _) = res[F64], res[F32]
    T = targets.shape[0]
    lim = [torch.zeros((), dtype=F64) for _ in range(4)]
    grad_limits, masks = [], []
    for lvl, (i64, i32) in enumerate(zip(k64, k32)):
        Bn, ch, H, W = layers[lvl].shape
        A, C = i64['A'], i64['C']
        K = C + 5
        rows = i64['rows'].detach()
        ncell = Bn * H * W * A
        blm = lambda z, t: torch.stack([z.abs(), (z * t).abs(), torch.ones_like(z)]).amax(0)
        lim[0] = lim[0] + scalar_limit(1, i64['xy_terms'], i32['xy_terms'], blm(rows[:, :2], i64['off']), 2 * T)
        whm = torch.maximum(rows[:, 2:4].abs(), i64['twh'].abs()).clamp_min(1.0)
        lim[1] = lim[1] + scalar_limit(1, i64['wh_terms'], i32['wh_terms'], 2 * whm * (rows[:, 2:4] - i64['twh']).abs() + i64['wh_terms'].detach(), 2 * T)
        lim[2] = lim[2] + scalar_limit(chain_of(C, 64), i64['cls_terms'], i32['cls_terms'], blm(rows[:, 5:], i64['onehot']), T * C)
        blocks = min((ncell + 255) // 256, CONF_BLOCKS)
        zo = i64['zo'].detach()
        cm = torch.where(i64['valid'], blm(zo, i64['mask']), torch.zeros_like(zo))
        # nvalid itself is an fp32 count (exact below 2^24)
        lim[3] = lim[3] + scalar_limit(chain_of(ncell, blocks * 256), i64['conf_terms'], i32['conf_terms'], cm, i64['nvalid'])
        # gradients, in the [B, H, W, A, K] view
        mag = torch.zeros(Bn, H, W, A, K, dtype=F64)
        mag[..., 4] = torch.where(i64['valid'], torch.maximum(torch.sigmoid(zo), i64['mask'].abs()), torch.zeros_like(zo)) / i64['nvalid']
        g2, gc = 1.0 / (2 * T), 1.0 / (T * C)
        mm = torch.cat([2 * g2 * torch.maximum(torch.sigmoid(rows[:, :2]), i64['off'].abs()), 2 * g2 * whm,
                        torch.zeros(T, 1, dtype=F64), gc * torch.maximum(torch.sigmoid(rows[:, 5:]), i64['onehot'])], 1)
        terms = i64['rows'].grad.double().abs()
        terms[:, 4] = 0
        cell = i64['cell']
        flat = lambda v: torch.zeros(ncell, K, dtype=F64).index_add(0, cell, v.double()).view(Bn, H, W, A, K)
        mag = mag + flat(mm)
        cnt, tsum = flat(torch.ones(T, K)), flat(terms)
        extra = torch.where(cnt > 1, (cnt + 2) * sm.EPS32 * tsum, torch.zeros_like(tsum))
        extra[..., 4] = 0
        to_nchw = lambda v: v.reshape(Bn, H, W, A * K).permute(0, 3, 1, 2)
        grad_limits.append(sm.limit_of(g64[lvl], g32[lvl], to_nchw(mag)) + to_nchw(extra))
        masks.append(i64['mask'])
    lim_total = 2 * lim[0] + lim[1] + lim[2] + lim[3] + 4 * sm.EPS32 * v64[0].abs()
    lims = [lim_total] + [l + sm.EPS32 * v.abs() for l, v in zip(lim, v64[1:])]
    return dict(vals64=torch.stack(v64), vals32=torch.stack(v32).double(), grads64=g64, grads32=g32, val_limits=torch.stack(lims),
                grad_limits=grad_limits, undecidable=und, masks=masks)


# ---------------------------------------------------------------------------------------------------------------- seeded inputs
def logits(shape, g, lim=8.0, scale=2.5):
    """Logits with |z| <= lim: beyond 8, 1 - sigmoid(z) rounds to 0 in fp32 and the reference's own fp32 arithmetic defines the answer."""
    return (torch.randn(shape, generator=g) * scale).clamp(-lim, lim)


def random_targets(T, B, C, g, lo=0.02, hi=0.8):
    """[T, 6] = (image, class, xc, yc, w, h), normalised, boxes inside the image."""
    img = torch.randint(0, B, (T,), generator=g).float()
    cls = torch.randint(0, C, (T,), generator=g).float()
    wh = torch.exp(math.log(lo) + (math.log(hi) - math.log(lo)) * torch.rand(T, 2, generator=g))
    xy = (wh / 2 + torch.rand(T, 2, generator=g) * (1 - wh)).clamp(max=1.0 - 1e-4)
    return torch.cat([img[:, None], cls[:, None], xy, wh], 1)


# name -> (seed, B, A, C, grids [(H, W)], T, images that get no target)
DEMO_CASES = {
    'c80':     (11, 2, 3, 80, [(3, 5), (6, 10), (12, 20)], 24, ()),
    'c65':     (12, 2, 3, 65, [(5, 4)], 12, ()),
    'c1':      (13, 2, 3, 1, [(7, 9)], 12, ()),
    'empty+200': (14, 3, 3, 1, [(16, 16)], 200, (0, 2)),     # image 1 holds all 200 targets, images 0 and 2 none
    't8200':   (15, 2, 3, 1, [(4, 4)], 8200, ()),
    'cells':   (16, 2, 3, 1, [(210, 210)], 6, ()),           # 264600 cells > 262144
}
DEMO_ANCHORS = torch.tensor([[3.6, 2.8], [1.9, 4.1], [1.1, 0.9]])
DEMO_PLANTED = 16            # 'empty+200': at least so many background predictions are made to coincide with a target


def demo_case(name):
    """(layers [B, A * (5 + C), H, W] contiguous NCHW, targets [T, 6], anchors per level) of a named demo case.  'empty+200' is the case
    for the mask loop (200 targets of one image, taken 64 at a time): for every eighth target, all along the list, the box logits of a
    background prediction (the target's cell, the anchor after its best one, no target's positive) are set so that the predicted box is
    the target itself.  Such a cell is ignored only if the loop reaches that target, wherever the image's list holds it."""
    seed, B, A, C, grids, T, empty = DEMO_CASES[name]
    g = torch.Generator().manual_seed(seed)
    layers = [logits((B, A * (5 + C), H, W), g) for H, W in grids]
    tg = random_targets(T, B, C, g)
    if empty:
        keepimg = [i for i in range(B) if i not in empty]
        tg[:, 0] = torch.tensor(keepimg, dtype=torch.float32)[torch.randint(0, len(keepimg), (T,), generator=g)]
    anchors = [DEMO_ANCHORS[:A] * (0.5 ** i) * max(H, W) / 8 for i, (H, W) in enumerate(grids)]
    if name == 'empty+200':
        (H, W), K, anc = grids[0], 5 + C, anchors[0]
        t = tg.double() * torch.tensor([1, 1, W, H, W, H], dtype=torch.float64)
        best = iou_any(0, 'wh', 0, t[:, 4:6], anc.double(), torch.float64, batch=True).max(1)[1]
        slot = lambda j, a: (int(t[j, 0]), int(t[j, 3]), int(t[j, 2]), a)
        taken = {slot(j, int(best[j])) for j in range(T)}
        planted = []
        for j in range(T - 1, -1, -8):
            s = slot(j, (int(best[j]) + 1) % A)
            if s in taken:
                continue
            taken.add(s)
            planted.append(s)
            img, gy, gx, a = s
            off = (t[j, 2:4] - torch.floor(t[j, 2:4])).clamp(0.02, 0.98)
            layers[0][img, a * K:a * K + 2, gy, gx] = torch.log(off / (1 - off)).float()
            layers[0][img, a * K + 2:a * K + 4, gy, gx] = torch.log(t[j, 4:6] / anc[a].double()).float()
        assert len(planted) >= DEMO_PLANTED
    return layers, tg, anchors


LIB_ANCHORS = torch.tensor([[0.55, 0.45], [0.22, 0.3], [0.09, 0.07], [0.35, 0.12], [0.12, 0.4], [0.7, 0.7], [0.04, 0.05], [0.16, 0.16]])
LIB_STRIDE = 8


class LibShell:
    """What Yolov3Loss reads of a model: pixel anchors per level and the strides.  Level anchors are LIB_ANCHORS[:A] * max(H, W) in feature
    units, so that a fair share of random targets passes the ratio < 4 test at every level."""

    def __init__(self, A, grids):
        self.anchors_per_level = [LIB_ANCHORS[:A] * max(H, W) * LIB_STRIDE for H, W in grids]
        self.backbone_strides_per_level = [LIB_STRIDE] * len(grids)


ALL_THREE = (0.14, 0.27)    # target sizes inside (0.55 / 4, 4 * 0.07): ratio < 4 against each of LIB_ANCHORS[:3], so every target matches thrice


def lib_case(seed, B, A, C, grids, T, lim=8.0, sizes=(0.02, 0.8)):
    """(heads [B, A, H, W, 5 + C] contiguous, targets [T, 6], LibShell) from one seeded generator; sizes = range of the target sizes."""
    g = torch.Generator().manual_seed(seed)
    heads = [logits((B, A, H, W, 5 + C), g, lim) for H, W in grids]
    tg = random_targets(T, B, C, g, *sizes) if T else torch.zeros(0, 6)
    return heads, tg, LibShell(A, grids)


def split_matches(built):
    """build_target's (locs, cats, xywhs, matched) -> (matches, anchors) of yolov3_terms, on the CPU."""
    locs, cats, xywhs, matched = built
    matches = [(b.cpu(), gxy[:, 0].cpu(), gxy[:, 1].cpu(), a.cpu(), c.cpu(), x.cpu()) for (b, gxy, a), c, x in zip(locs, cats, xywhs)]
    return matches, [m.cpu() for m in matched]
