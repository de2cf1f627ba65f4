"""The matching rule of the validation mAP restated in numpy, and the inputs its tests are made of.

The reference (metrics/map.py:17-83) lists every (target, prediction) pair of equal class whose IoU exceeds the first threshold, sorts the
list by IoU, keeps the first row of every prediction (np.unique) and then, of what is left, the first row of every target.  np.unique
returns its rows ordered by the key, so after the first cut the rows stand in prediction order and the second cut keeps the LOWEST
prediction of a target, not the best one.  As two arg-reductions:

1. a prediction picks, among the targets with its class and fp32 IoU > float32(thr[0]), the one with the highest IoU -- equal IoUs: the
   lowest target index (what a stable sort leaves first; the library class sorts unstably, which leaves exact ties open);
2. a target goes to the lowest-indexed prediction that picked it, and every other prediction gets nothing;
3. a winner's flag at threshold k is float64(IoU) > thr[k].

``fva_map_match`` (csrc/loss.hip) computes this per image of a batch; the functions here are what its tests compare with.
"""
import numpy as np
import torch

THR10 = np.linspace(0.5, 0.95, 10)


def match_rule(iou, tcls, pcls, thr):
    """iou [N,M] float32 (target x prediction), tcls [N], pcls [M] float32, thr [n] float64 -> flags [M,n] bool."""
    iou, tcls, pcls = np.asarray(iou, np.float32), np.asarray(tcls, np.float32), np.asarray(pcls, np.float32)
    thr = np.asarray(thr, np.float64)
    N, M = iou.shape
    flags = np.zeros((M, len(thr)), dtype=bool)
    winner = np.full(N, -1, dtype=np.int64)
    pick = np.full(M, -1, dtype=np.int64)
    for p in range(M):
        best = -1
        for t in range(N):
            if tcls[t] == pcls[p] and iou[t, p] > np.float32(thr[0]) and (best < 0 or iou[t, p] > iou[best, p]):
                best = t                                   # strictly greater: the lowest index of equal IoUs stays
        pick[p] = best
    for p in range(M):                                     # ascending: the first prediction to arrive keeps the target
        if pick[p] >= 0 and winner[pick[p]] < 0:
            winner[pick[p]] = p
    for t in range(N):
        if winner[t] >= 0:
            flags[winner[t]] = np.float64(iou[t, winner[t]]) > thr
    return flags


def rows_from_rule(pred, target, thr, iou=None):
    """What process_one appends for pred [M,6] = class, confidence, xyxy and target [N,5] = class, xyxy (torch, fp32): the
    [M, 2 + n] float64 matrix, from the rule.  iou: the [N,M] matrix to use (default: the oracle's fp32 one)."""
    from oracle.boxes import cal_iou_batch
    M = pred.size(0)
    out = np.zeros((M, 2 + len(thr)), dtype=np.float64)
    out[:, 0], out[:, 1] = pred[:, 1].numpy(), pred[:, 0].numpy()
    if target.size(0) and M:
        if iou is None:
            iou = cal_iou_batch(target[:, 1:], pred[:, 2:], mode='xyxy').numpy()
        out[:, 2:] = match_rule(iou, target[:, 0].numpy(), pred[:, 0].numpy(), thr)
    return out


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def random_image(gen, n_cls=3, max_targets=11, size=300.0):
    """(pred [M,6] = class, confidence, xyxy; target [N,5] = class, xyxy): 0..max_targets targets, for most of them one or two jittered
    copies as predictions (some with a changed class), and a few boxes that match nothing."""
    nt = int(torch.randint(0, max_targets + 1, (1,), generator=gen))
    tcls = torch.randint(0, n_cls, (nt,), generator=gen).float()
    txy = torch.rand(nt, 2, generator=gen) * size
    twh = 20 + torch.rand(nt, 2, generator=gen) * 100
    target = torch.cat([tcls.view(-1, 1), txy, txy + twh], dim=1)
    boxes, classes = [], []
    for rep in range(2):
        keep = torch.rand(nt, generator=gen) > (0.2 if rep == 0 else 0.6)
        n = int(keep.sum())
        boxes.append(target[keep, 1:] + torch.randn(n, 4, generator=gen) * (5 if rep == 0 else 9))
        c = target[keep, 0].clone()
        flip = torch.rand(n, generator=gen) < 0.1
        c[flip] = (c[flip] + 1) % n_cls
        classes.append(c)
    nf = int(torch.randint(0, 4, (1,), generator=gen))
    fxy = torch.rand(nf, 2, generator=gen) * size
    boxes.append(torch.cat([fxy, fxy + 30 + torch.rand(nf, 2, generator=gen) * 60], dim=1))
    classes.append(torch.randint(0, n_cls, (nf,), generator=gen).float())
    box, cls = torch.cat(boxes), torch.cat(classes)
    perm = torch.randperm(box.size(0), generator=gen)
    box, cls = box[perm], cls[perm]
    conf = torch.rand(box.size(0), generator=gen)
    return torch.cat([cls.view(-1, 1), conf.view(-1, 1), box], dim=1), target


def tie_image():
    """Exact ties: target 0 twice (rows 0 and 1), target 2 apart; prediction 0 and its exact copy 1 on the duplicated target, prediction 2
    on the last.  Both predictions pick target row 0 (equal IoU, lowest index), the lower-indexed one keeps it, the copy gets nothing --
    target row 1 stays free -- and the last box matches: correct at 0.5 = 1, 0, 1."""
    target = torch.tensor([[1., 10., 10., 110., 110.], [1., 10., 10., 110., 110.], [1., 200., 200., 260., 280.]])
    pred = torch.tensor([[1., 0.9, 12., 11., 108., 112.], [1., 0.8, 12., 11., 108., 112.], [1., 0.7, 201., 199., 262., 281.]])
    return pred, target


def pack_batch(images, max_det, pad=float('nan'), shuffle=None, extra_rows=False):
    """images: list of (pred [M,6] = class, confidence, xyxy; target [N,5]) -> dets [B,max_det,6] = xyxy, score, category (rows beyond
    an image's M filled with ``pad``), kept [B] int32, targets [T,6] = image, class, xyxy.  shuffle: a torch.Generator that permutes the
    target rows across images; extra_rows: rows of image index -1 and B are mixed in."""
    B = len(images)
    dets = torch.full((B, max_det, 6), pad, dtype=torch.float32)
    kept = torch.zeros(B, dtype=torch.int32)
    rows = []
    for b, (pred, target) in enumerate(images):
        m = pred.size(0)
        assert m <= max_det
        dets[b, :m, 0:4], dets[b, :m, 4], dets[b, :m, 5] = pred[:, 2:6], pred[:, 1], pred[:, 0]
        kept[b] = m
        rows.append(torch.cat([torch.full((target.size(0), 1), float(b)), target], dim=1))
        if extra_rows and target.size(0):                  # the same boxes under image indices that do not exist
            for other in (-1.0, float(B)):
                rows.append(torch.cat([torch.full((target.size(0), 1), other), target], dim=1))
    targets = torch.cat(rows) if rows else torch.zeros(0, 6)
    if shuffle is not None:
        targets = targets[torch.randperm(targets.size(0), generator=shuffle)]
    return dets, kept, targets.float()


def at_threshold(thr, target_box=(0.0, 0.0, 128.0, 128.0)):
    """Five predictions inside the 128 x 128 target at the origin whose fp32 IoU (= the area ratio) sits on ``thr``: widths one fp32
    step apart around 128 * thr (x1 = 0, so the width is the stored coordinate itself).  Returns boxes [5,4]."""
    x1, y1, x2, y2 = target_box
    w = np.float32(128.0 * thr)
    steps = [np.float32(w + k * np.spacing(w)) for k in (-2, -1, 0, 1, 2)]
    return torch.tensor([[x1, y1, float(x1 + s), y2] for s in steps], dtype=torch.float32)
