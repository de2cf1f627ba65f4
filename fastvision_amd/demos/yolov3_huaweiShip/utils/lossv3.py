"""ComputeLoss on the MI355X kernels -- API mirror of the reference's demos/yolov3_huaweiShip/utils/lossv3.py.

``forward(predict_layers, target_all, model)`` returns ``(loss_box, loss_cls, loss_conf)``, each of shape [1]: best-anchor assignment
on every level, box term mean(1 - CIoU(pred, target)) with pred = (sigmoid(xy) + cell, exp(wh) * anchor), BCE(cls), IoU>0.5 ignore mask,
masked objectness BCE -- values and analytic gradients from the fused HIP kernels (``fva_demo_ciou_loss``).  The three losses are one
autograd node with three outputs: the forward pass stores d (box + cls + conf) / d head once per level, and since the three parts write
disjoint channel groups of it (k < 4 box, k == 4 objectness, k >= 5 class) the backward pass only scales each group by its upstream
scalar (``fva_scale_head_groups``; no traffic for ``(box + cls + conf).backward()``).
"""
import torch

from ....loss.demo_loss import DemoComputeLoss, demo_loss_forward
from ....ops import scale_head_group_grads

__all__ = ['ComputeLoss']


class _ShipLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, targets, anchors, *layers):
        out = demo_loss_forward(ctx, 'fva_demo_ciou_loss', 4, targets, anchors, layers)
        parts = out[1:4].clone()
        ctx.mark_non_differentiable(parts)
        return out[1:2].clone(), out[2:3].clone(), out[3:4].clone(), parts

    @staticmethod
    def backward(ctx, g_box, g_cls, g_conf, _gparts):
        return (None, None, *scale_head_group_grads(ctx, g_box, g_cls, g_conf))


class ComputeLoss(DemoComputeLoss):
    empty_targets = 'ComputeLoss needs at least one target (the reference fails on an empty batch too, lossv3.py:88)'

    def forward(self, predict_layers, target_all, model):
        tg, anchors = self._inputs(predict_layers, target_all, model)
        loss_box, loss_cls, loss_conf, self.last_parts = _ShipLossFn.apply(tg, anchors, *predict_layers)      # last_parts = (box, cls, conf)
        return loss_box, loss_cls, loss_conf
