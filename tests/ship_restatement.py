"""The ship demo's loss (fva_demo_ciou_loss) and decode (fva_yolo_decode variant 2) written with plain differentiable torch ops and
parameterised by ``dt``, in the manner of tests/loss_restatement.py, from which everything shared is imported: the IoU family, the demo
loss's discrete decisions and its class and objectness terms (loss_restatement.demo_terms), the measure.  Not a test module (pytest does
not collect it); tests/test_ship_restatement_cpu.py pins it without a GPU against vectors of the reference's own ComputeLoss
(tests/golden/ship_loss.npz).

  ComputeLoss.forward (demos/yolov3_huaweiShip/utils/lossv3.py:35-120), per level:
    best anchor, cell, class term, ignore mask and objectness term: as demos/yolov3_u (loss_restatement.demo_terms)
    box term:  mean over T of 1 - CIoU(pred, target; 'xywh', eps 1e-7),  pred = (sigmoid(z_xy) + cell, exp(z_wh) * anchor),
               CIoU the demo's: iou_any(3, 'xywh', 1, ...) (centre sums not halved, minus sign, alpha a constant)
  returns (box, cls, conf), each summed over the levels.
``wrong`` selects a deliberately wrong box term (tests/test_ship_restatement_cpu.py shows that the measure rejects each); '' is the formula.
"""
import math

import torch

import detect_restatement as dr
import loss_restatement as lr
import streaming_measure as sm

F64, F32 = torch.float64, torch.float32
WRONG = ('halved', 'plus', 'alpha_grad')


def _ciou(pbox, tbox, dt, wrong=''):
    if not wrong:
        return lr.iou_any(3, 'xywh', 1, pbox, tbox, dt)
    iou = lr.iou_any(0, 'xywh', 0, pbox, tbox, dt)
    d_demo = lr.iou_any(2, 'xywh', 1, pbox, tbox, dt)                 # iou - rho^2 / c^2, centre sums as they are
    av = d_demo - lr.iou_any(3, 'xywh', 1, pbox, tbox, dt)           # alpha v, alpha a constant
    if wrong == 'halved':                                             # the library's halved centre sums under the demo's minus sign
        return iou - (lr.iou_any(2, 'xywh', 0, pbox, tbox, dt) - iou) - av
    if wrong == 'plus':                                               # the library's sign on the demo's distance term
        return iou + (iou - d_demo) - av
    assert wrong == 'alpha_grad'                                      # alpha differentiated
    ax1, ay1, ax2, ay2 = lr._corners(pbox.to(dt), 'xywh')
    bx1, by1, bx2, by2 = lr._corners(tbox.to(dt), 'xywh')
    v = (4 / math.pi ** 2) * torch.pow(torch.atan((bx2 - bx1) / (by2 - by1 + lr.IOU_EPS)) - torch.atan((ax2 - ax1) / (ay2 - ay1 + lr.IOU_EPS)), 2)
    return d_demo - v / (v - iou + (1 + lr.IOU_EPS)) * v


def ship_terms(layers, targets, anchors, dt, keep=None, wrong=''):
    """layers: per level raw [B, A * (5 + C), H, W]; targets [T, 6] fp32 = (image, class, xc, yc, w, h) normalised; anchors: per level [A, 2]
    feature scale.  Returns ((box, cls, conf), undecidable).  keep: a list that receives one dict per level, demo_terms' own (rows with their
    gradient retained, onehot, cls_terms, conf_terms, mask, valid, nvalid, zo, cell, ...) plus pbox, tbox, sxy, box_terms."""
    own = [] if keep is None else keep
    _, (_, _, l_cls, l_conf), und = lr.demo_terms(layers, targets, anchors, dt, keep=own)
    T = targets.shape[0]
    l_box = torch.zeros((), dtype=dt)
    for lvl, info in enumerate(own):
        Bn, ch, H, W = layers[lvl].shape
        A = info['A']
        cell = info['cell']
        best, gx, gy = cell % A, (cell // A) % W, (cell // (A * W)) % H
        rows = info['rows']
        tgd = (targets.float() * torch.tensor([1, 1, W, H, W, H], dtype=torch.float32)).to(dt)      # target * grid size in fp32, as the kernel forms it
        sxy = torch.sigmoid(rows[:, 0:2])
        pbox = torch.cat([sxy + torch.stack([gx, gy], 1).to(dt), torch.exp(rows[:, 2:4]) * anchors[lvl].to(dt)[best]], 1)
        tbox = tgd[:, 2:6]
        box_terms = 1 - _ciou(pbox, tbox, dt, wrong)
        l_box = l_box + box_terms.sum() / T
        info.update(pbox=pbox, tbox=tbox, sxy=sxy, box_terms=box_terms)
    return (l_box, l_cls, l_conf), und


def ship_reference(layers, targets, anchors, wrong32=''):
    """Float64 reference, fp32 evaluation and limits: vals64 / vals32 [3] = (box, cls, conf), grads64 / grads32 per level (of box + cls +
    conf), val_limits [3], grad_limits per level, undecidable, masks (per level [B, H, W, A]).
      mag, box columns, per target (the recipe of loss_restatement.yolov3_reference): cond * g * (|dIoU| + |d rho^2/c^2| + |d alpha v|) * dp/dz,
        g = 1 / T, the IoU's quotient rule (iou_open_grad_mag), the distance term (term_open_grad_mag(2, 1, ...)) and alpha v opened up, each
        |d . / d x| = |d . / d x1| + |d . / d x2| folded from the corners (and |d . / d w| half of it); cond = box_condition (edge differences;
        it also carries the fp32 sum sigmoid + cell: a corner of size c next to a width d); dp/dz = s (1 - s) for xy, with the condition
        1 / (1 - s) of the sigmoid derivative, and the size itself for wh.
      mag, class columns and objectness: as loss_restatement.demo_reference.
      Elements that m > 1 targets add into (atomicAdd) additionally get sum_limit(m, sum |term|)."""
    res = {}
    for dt, wrong in ((F64, ''), (F32, wrong32)):
        leaves = [h.detach().to(dt).requires_grad_(True) for h in layers]
        keep = []
        parts, und = ship_terms(leaves, targets, anchors, dt, keep=keep, wrong=wrong)
        (parts[0] + parts[1] + parts[2]).backward()
        res[dt] = ([p.detach() for p in parts], [l.grad for l in leaves], keep, und)
    (v64, g64, k64, und), (v32, g32, k32, _) = res[F64], res[F32]
    T = targets.shape[0]
    lim = [torch.zeros((), dtype=F64) for _ in range(3)]
    grad_limits, masks = [], []
    for lvl, (i64, i32) in enumerate(zip(k64, k32)):
        Bn, ch, H, W = layers[lvl].shape
        A, C = i64['A'], i64['C']
        K = C + 5
        rows = i64['rows'].detach()
        ncell = Bn * H * W * A
        blm = lambda z, t: torch.stack([z.abs(), (z * t).abs(), torch.ones_like(z)]).amax(0)
        cond = lr.box_condition(i64['pbox'], i64['tbox'], 'xywh')
        lim[0] = lim[0] + lr.scalar_limit(1, i64['box_terms'], i32['box_terms'], cond * i64['box_terms'].detach().abs().clamp_min(1.0), T)
        lim[1] = lim[1] + lr.scalar_limit(lr.chain_of(C, 64), i64['cls_terms'], i32['cls_terms'], blm(rows[:, 5:], i64['onehot']), T * C)
        blocks = min((ncell + 255) // 256, lr.CONF_BLOCKS)
        zo = i64['zo'].detach()
        cm = torch.where(i64['valid'], blm(zo, i64['mask']), torch.zeros_like(zo))
        lim[2] = lim[2] + lr.scalar_limit(lr.chain_of(ncell, blocks * 256), i64['conf_terms'], i32['conf_terms'], cm, i64['nvalid'])
        # gradients, in the [B, H, W, A, K] view
        mag = torch.zeros(Bn, H, W, A, K, dtype=F64)
        mag[..., 4] = torch.where(i64['valid'], torch.maximum(torch.sigmoid(zo), i64['mask'].abs()), torch.zeros_like(zo)) / i64['nvalid']
        pbd, sxy = i64['pbox'].detach(), i64['sxy'].detach()
        pc4 = torch.stack(lr._corners(pbd, 'xywh'), 1).requires_grad_(True)
        tc4 = torch.stack(lr._corners(i64['tbox'].detach(), 'xywh'), 1)
        d_av, = torch.autograd.grad((lr.iou_any(2, 'xyxy', 1, pc4, tc4, F64) - lr.iou_any(3, 'xyxy', 1, pc4, tc4, F64)).sum(), pc4)
        fold = lambda d: torch.stack([d[:, 0].abs() + d[:, 2].abs(), d[:, 1].abs() + d[:, 3].abs(),
                                      (d[:, 0].abs() + d[:, 2].abs()) / 2, (d[:, 1].abs() + d[:, 3].abs()) / 2], 1)
        d_iou, d_term, d_av = fold(lr.iou_open_grad_mag(pc4, tc4, 'xyxy', True)), fold(lr.term_open_grad_mag(2, 1, pc4, tc4)), fold(d_av)
        dpdz = torch.cat([sxy * (1 - sxy), pbd[:, 2:]], 1)
        cxy = torch.cat([1 / (1 - sxy), torch.ones_like(pbd[:, 2:])], 1)
        bmag = cond[:, None] * cxy * ((1.0 / T) * (d_iou + d_term + d_av)) * dpdz
        gc = 1.0 / (T * C)
        mm = torch.cat([bmag, torch.zeros(T, 1, dtype=F64), gc * torch.maximum(torch.sigmoid(rows[:, 5:]), i64['onehot'])], 1)
        terms = i64['rows'].grad.double().abs()
        terms[:, 4] = 0
        cell = i64['cell']
        flat = lambda v: torch.zeros(ncell, K, dtype=F64).index_add(0, cell, v.double()).view(Bn, H, W, A, K)
        mag = mag + flat(mm)
        cnt, tsum = flat(torch.ones(T, K)), flat(terms)
        extra = torch.where(cnt > 1, sm.sum_limit(cnt, tsum), torch.zeros_like(tsum))
        extra[..., 4] = 0
        to_nchw = lambda v: v.reshape(Bn, H, W, A * K).permute(0, 3, 1, 2)
        grad_limits.append(sm.limit_of(g64[lvl], g32[lvl], to_nchw(mag)) + to_nchw(extra))
        masks.append(i64['mask'])
    lims = [l + sm.EPS32 * v.abs() for l, v in zip(lim, v64)]
    return dict(vals64=torch.stack(v64), vals32=torch.stack(v32).double(), grads64=g64, grads32=g32, val_limits=torch.stack(lims),
                grad_limits=grad_limits, undecidable=und, masks=masks)


# ---------------------------------------------------------------------------------------------------------------- decode variant 2
def decode_rows2(heads, anchors, strides, letterbox, dt):
    """postProcess of the ship demo (demos/yolov3_huaweiShip/inference.py:107-136).  heads: per level [B, A, H, W, K] fp32; anchors: per
    level A pairs (w, h), feature scale; letterbox: None or (resize_ratio, pad_left, pad_top, ori_w, ori_h, min_wh).
    -> (rows [B, sum A*H*W, K] in (y, x, a) order, mag, extent), aligned with the kernel's output as detect_restatement.decode_rows is: every
    row is kept, with objectness -1 where the reference drops the box.  mag: the value itself for (sigmoid + cell) * stride (one sum, then an
    exact product), exp(t) * anchor * stride and the sigmoids; the letterboxed corners as in detect_restatement."""
    outs = []
    for h, anc, stride in zip(heads, anchors, strides):
        B, A, H, W, K = h.shape
        t = h.to(dt).permute(0, 1, 4, 2, 3).contiguous().permute(0, 3, 4, 1, 2)    # [B, H, W, A, K] over NCHW memory, as the demo's model emits it
        anc = torch.tensor([[dr.f32(a[0]), dr.f32(a[1])] for a in anc], dtype=F64).to(dt).view(1, 1, 1, A, 2)
        stride = dr.f32(stride)
        ys = torch.arange(H).view(H, 1).expand(H, W)
        xs = torch.arange(W).view(1, W).expand(H, W)
        cell = torch.stack([xs, ys], dim=2).to(dt).view(1, H, W, 1, 2)
        o = torch.empty_like(t)
        o[..., 0:2] = (torch.sigmoid(t[..., 0:2]) + cell) * stride
        o[..., 2:4] = (torch.exp(t[..., 2:4]) * anc) * stride
        o[..., 4:] = torch.sigmoid(t[..., 4:])
        outs.append(o.reshape(B, -1, K))
    out = torch.cat(outs, 1)
    mag = out.abs()
    if letterbox is None:
        return out, mag, None
    rr, pl, pt, ow, oh, mn = (dr.f32(v) for v in letterbox)
    pad, lim = torch.tensor([pl, pt], dtype=dt), torch.tensor([ow, oh], dtype=dt)
    ctr = torch.minimum(((out[..., 0:2] - pad) / rr).clamp_min(0), lim - 1)           # :119-125
    ext = torch.minimum((out[..., 2:4] / rr).clamp_min(0), lim)                         # :121-127
    keep = (ext[..., 0] > mn) & (ext[..., 1] > mn)                                      # :129
    half = ext / 2
    res = out.clone()
    res[..., 0:2] = torch.minimum((ctr - half).clamp_min(0), lim - 1)                   # :132-136
    res[..., 2:4] = torch.minimum((ctr + half).clamp_min(0), lim - 1)
    res[..., 4] = torch.where(keep, out[..., 4], torch.full_like(out[..., 4], -1.0))
    mg = torch.maximum(torch.maximum(out[..., 0:2].abs(), pad.abs().expand_as(half)) / rr, half.abs())
    mag = mag.clone()
    mag[..., 0:2] = mg
    mag[..., 2:4] = mg
    mag[..., 4] = torch.ones_like(mag[..., 4])
    return res, mag, ext
