"""ComputeLoss on the MI355X kernels -- API mirror of the reference's demos/yolov3_huaweiShip/utils/lossv3.py.

``forward(predict_layers, target_all, model)`` returns ``(loss_box, loss_cls, loss_conf)``, each of shape [1]: best-anchor assignment
on every level, box term mean(1 - CIoU(pred, target)) with pred = (sigmoid(xy) + cell, exp(wh) * anchor), BCE(cls), IoU>0.5 ignore mask,
masked objectness BCE -- values and analytic gradients from the fused HIP kernels (``fva_demo_ciou_loss``).  The three losses are one
autograd node with three outputs: the forward pass stores d (box + cls + conf) / d head once per level, and since the three parts write
disjoint channel groups of it (k < 4 box, k == 4 objectness, k >= 5 class) the backward pass only scales each group by its upstream
scalar (``fva_scale_head_groups``; no traffic for ``(box + cls + conf).backward()``).
"""
import torch
import torch.nn as nn

from .... import _lib
from ....ops import _p, _stream, require_gpu, scale_head_group_grads

__all__ = ['ComputeLoss']


class _ShipLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, targets, anchors, *layers):
        need = any(ctx.needs_input_grad[2:])
        hs, grads = [], []
        levels = (_lib.HeadLevel * len(layers))()
        for i, raw in enumerate(layers):
            h = raw.detach()
            if h.dtype != torch.float32:
                h = h.float()
            B, ch, gh, gw = h.shape
            A = len(anchors[i])
            K = ch // A
            g = None
            if need:
                g = torch.zeros_like(h)
                if g.stride() != h.stride():
                    h = h.contiguous()
                    g = torch.zeros_like(h)
            sb, sc, sy, sx = h.stride()
            lv = levels[i]
            lv.data, lv.grad = h.data_ptr(), (g.data_ptr() if g is not None else None)
            lv.sb, lv.sa, lv.sy, lv.sx, lv.sk = sb, K * sc, sy, sx, sc      # channel c = a*K + k  (lossv3.py:43)
            lv.B, lv.A, lv.H, lv.W, lv.K = B, A, gh, gw, K
            for j, (w, hh) in enumerate(anchors[i]):
                lv.anchor_w[j], lv.anchor_h[j] = w, hh
            lv.stride = 1.0
            hs.append(h)
            grads.append(g)
        T = targets.shape[0]
        lib = _lib.load()
        wsb = lib.fva_demo_ciou_loss_workspace(T, levels, len(hs))
        ws = torch.empty(wsb, dtype=torch.uint8, device=hs[0].device)
        out = torch.empty(4, dtype=torch.float32, device=hs[0].device)
        _lib.call('fva_demo_ciou_loss', _p(targets), T, levels, len(hs), _p(out), _p(ws), wsb, _stream())
        ctx.grads, ctx.dtypes, ctx.anchors_per_level = grads, [l.dtype for l in layers], [len(a) for a in anchors]
        parts = out[1:4].clone()
        ctx.mark_non_differentiable(parts)
        return out[1:2].clone(), out[2:3].clone(), out[3:4].clone(), parts

    @staticmethod
    def backward(ctx, g_box, g_cls, g_conf, _gparts):
        return (None, None, *scale_head_group_grads(ctx, g_box, g_cls, g_conf))


class ComputeLoss(nn.Module):
    def __init__(self):
        super().__init__()
        self.last_parts = None
        self._anchors = None                     # (key, host copy): reading model.anchors is a device sync, and not allowed inside a graph capture

    def get_model(self, model):
        return model.module if hasattr(model, 'module') else model

    def forward(self, predict_layers, target_all, model):
        model = self.get_model(model)
        require_gpu(predict_layers[0], 'ComputeLoss')
        key = tuple((a.data_ptr(), a._version) for a in model.anchors)
        if self._anchors is None or self._anchors[0] != key:
            self._anchors = (key, [[(float(w), float(h)) for w, h in a.reshape(-1, 2).tolist()] for a in model.anchors])   # feature scale
        anchors = self._anchors[1]
        if target_all.shape[0] == 0:
            raise RuntimeError('ComputeLoss needs at least one target (the reference fails on an empty batch too, lossv3.py:88)')
        tg = target_all.detach().to(device=predict_layers[0].device, dtype=torch.float32).contiguous()
        loss_box, loss_cls, loss_conf, self.last_parts = _ShipLossFn.apply(tg, anchors, *predict_layers)      # last_parts = (box, cls, conf)
        return loss_box, loss_cls, loss_conf
