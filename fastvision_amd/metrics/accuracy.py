"""Top-1 accuracy -- API mirror of the reference's metrics/accuracy.py -- and, beyond it, top-k.

Device logits run fva_top1_accuracy (argmax per row, compared with the label, counted in a fixed order) or, for ``topk`` > 1,
fva_topk_accuracy (a hit when fewer than k entries of the row beat the label's): the result stays on the device, with no host sync.
CPU tensors run the reference's torch expression (top-k: the same rule in torch ops).
"""
import torch

__all__ = ['Accuracy']


class Accuracy:
    """``Accuracy()(y_pred [N, num_classes], y_true [N]) -> [1]`` float tensor on y_pred's device: the fraction of rows whose argmax
    (torch.argmax: first index among equal maxima, a NaN counts as the maximum) equals the label.

    Shape quirk kept from the reference: the labels are broadcast with ``expand_as`` onto the [N] argmax, so ``y_true`` must be [N]
    (or broadcastable to it); a [N, 1] label tensor raises RuntimeError, as it does there."""

    def __init__(self, topk=1):
        if int(topk) != topk or topk < 1:
            raise ValueError(f'Accuracy: topk = {topk} must be an integer >= 1')
        self.topk = int(topk)

    @torch.no_grad()
    def __call__(self, y_pred, y_true):
        if self.topk > 1:
            return _device_accuracy(y_pred, y_true, self.topk) if y_pred.is_cuda else _host_topk(y_pred, y_true, self.topk)
        if not y_pred.is_cuda:
            pred = torch.argmax(y_pred, dim=1)
            batch_size = pred.size(0)
            correct = pred.eq(y_true.expand_as(pred)).float().sum(0, keepdim=True)
            return correct / batch_size
        return _device_accuracy(y_pred, y_true)


def _host_topk(y_pred, y_true, k):
    """The rule of fva_topk_accuracy in torch ops: entry j beats the label's entry when it is larger (a NaN is largest) or equal with a
    smaller index; a hit when fewer than k do.  A label outside [0, C) or not an integer never hits."""
    z = y_pred.float()
    R, Cc = z.shape
    lab = y_true.expand(R)
    valid = (lab >= 0) & (lab < Cc) & (lab == lab.long())
    y = torch.where(valid, lab.long(), torch.zeros_like(lab.long())).view(-1, 1)
    zy = z.gather(1, y)
    idx = torch.arange(Cc, device=z.device).view(1, -1)
    zn, yn = torch.isnan(z), torch.isnan(zy)
    same = (zn & yn) | (z == zy)
    beats = (zn & ~yn) | (~zn & ~yn & (z > zy)) | (same & (idx < y))
    hit = (beats.sum(1) < k) & valid
    return hit.float().sum(0, keepdim=True) / R


def _device_accuracy(y_pred, y_true, topk=1):
    from .. import _lib
    from ..ops import _p, _stream
    R, Cc = y_pred.shape
    lab = y_true.expand(R)                        # the reference's expand_as onto [N]: [N, 1] raises here as well
    if lab.device != y_pred.device:
        raise RuntimeError('Accuracy: y_pred and y_true must be on the same device')
    z = y_pred if (y_pred.dtype in (torch.float32, torch.bfloat16) and y_pred.is_contiguous()) else y_pred.float().contiguous()
    if lab.is_floating_point():
        lab, code = (lab if lab.dtype == torch.float32 else lab.float()).contiguous(), _lib.LABEL_F32
    else:
        lab, code = (lab if lab.dtype == torch.int64 else lab.long()).contiguous(), _lib.LABEL_I64
    out = torch.empty(1, dtype=torch.float32, device=z.device)
    ws = torch.empty(R, dtype=torch.int32, device=z.device)
    zcode = _lib.BF16 if z.dtype == torch.bfloat16 else _lib.F32
    if topk == 1:
        _lib.call('fva_top1_accuracy', _p(z), zcode, _p(lab), code, R, Cc, _p(out), _p(ws), _stream())
    else:
        _lib.call('fva_topk_accuracy', _p(z), zcode, _p(lab), code, R, Cc, topk, _p(out), _p(ws), _stream())
    return out
