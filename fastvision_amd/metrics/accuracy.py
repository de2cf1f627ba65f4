"""Top-1 accuracy -- API mirror of the reference's metrics/accuracy.py.

Device logits run fva_top1_accuracy (argmax per row, compared with the label, counted in a fixed order): the result stays on the
device, with no host sync.  CPU tensors run the reference's torch expression.
"""
import torch

__all__ = ['Accuracy']


class Accuracy:
    """``Accuracy()(y_pred [N, num_classes], y_true [N]) -> [1]`` float tensor on y_pred's device: the fraction of rows whose argmax
    (torch.argmax: first index among equal maxima, a NaN counts as the maximum) equals the label.

    Shape quirk kept from the reference: the labels are broadcast with ``expand_as`` onto the [N] argmax, so ``y_true`` must be [N]
    (or broadcastable to it); a [N, 1] label tensor raises RuntimeError, as it does there."""

    def __init__(self):
        ...

    @torch.no_grad()
    def __call__(self, y_pred, y_true):
        if not y_pred.is_cuda:
            pred = torch.argmax(y_pred, dim=1)
            batch_size = pred.size(0)
            correct = pred.eq(y_true.expand_as(pred)).float().sum(0, keepdim=True)
            return correct / batch_size
        return _device_accuracy(y_pred, y_true)


def _device_accuracy(y_pred, y_true):
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
    _lib.call('fva_top1_accuracy', _p(z), _lib.BF16 if z.dtype == torch.bfloat16 else _lib.F32, _p(lab), code, R, Cc, _p(out), _p(ws),
              _stream())
    return out
