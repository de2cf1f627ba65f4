"""ComputeLoss on the MI355X kernels -- API mirror of the reference's demos/yolov3_u/utils/lossv3.py.

``forward(predict_layers, target_all, model)``: best-anchor assignment on every level, BCE(xy) / MSE(wh) / BCE(cls),
IoU>0.5 ignore mask, masked objectness BCE, total = 2*xy + wh + cls + conf -- value and analytic gradients from the
fused HIP kernels (``fva_demo_loss``).  The reference prints its four partial losses every call (4 host syncs,
lossv3.py:108); here they stay on the device in ``self.last_parts`` and ``verbose=True`` restores the print.
"""
import torch

from ....loss.demo_loss import DemoComputeLoss, demo_loss_forward
from ....ops import scale_loss_grads

__all__ = ['ComputeLoss']


class _DemoLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, targets, anchors, *layers):
        out = demo_loss_forward(ctx, 'fva_demo_loss', 5, targets, anchors, layers)
        parts = out[1:5].clone()
        ctx.mark_non_differentiable(parts)
        return out[0:1].clone(), parts

    @staticmethod
    def backward(ctx, gout, _gparts):
        return (None, None, *scale_loss_grads(ctx, gout))


class ComputeLoss(DemoComputeLoss):
    empty_targets = 'ComputeLoss needs at least one target (the reference fails on an empty image too, lossv3.py:94)'

    def __init__(self, verbose=False):
        super().__init__()
        self.verbose = verbose

    def forward(self, predict_layers, target_all, model):
        tg, anchors = self._inputs(predict_layers, target_all, model)
        loss, parts = _DemoLossFn.apply(tg, anchors, *predict_layers)
        self.last_parts = parts                  # (xy, wh, cls, conf) as the reference prints them
        if self.verbose:
            print(*parts.tolist())
        return loss
