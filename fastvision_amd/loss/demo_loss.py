"""What the two demo losses share (demos/yolov3_u and demos/yolov3_huaweiShip ``utils/lossv3.py``): one pipeline of HIP kernels with two
box terms behind ``fva_demo_loss`` / ``fva_demo_ciou_loss``.  Each demo keeps its own autograd node (outputs and backward rule differ)
and its ``ComputeLoss`` subclass; the forward body and the module base are here.
"""
import torch
import torch.nn as nn

from .. import _lib
from ..ops import _p, _stream, head_grad_buffer, require_gpu


def demo_loss_forward(ctx, symbol, n_out, targets, anchors, layers):
    """The forward pass of a demo loss node whose inputs are (targets, anchors, *layers): heads [B, A * K, H, W] to fp32, gradient buffers
    with the heads' strides when a head needs one, the level structs, the workspace and the call of ``symbol``.  Returns the C function's
    ``loss_out`` [n_out]; ctx.grads / ctx.dtypes / ctx.anchors_per_level are what scale_loss_grads / scale_head_group_grads read."""
    need = any(ctx.needs_input_grad[2:])
    hs, grads = [], []                           # hs keeps the fp32 / contiguous copies alive until the call is enqueued
    levels = (_lib.HeadLevel * len(layers))()
    for i, raw in enumerate(layers):
        h = raw.detach()
        if h.dtype != torch.float32:
            h = h.float()
        h, g = head_grad_buffer(h, need)
        levels[i] = _lib.head_level_nchw(h, g, len(anchors[i]), anchors[i])      # feature-scale anchors; the kernels ignore the stride
        hs.append(h)
        grads.append(g)
    T, dev = targets.shape[0], hs[0].device
    wsb = getattr(_lib.load(), symbol + '_workspace')(T, levels, len(layers))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    out = torch.empty(n_out, dtype=torch.float32, device=dev)
    _lib.call(symbol, _p(targets), T, levels, len(layers), _p(out), _p(ws), wsb, _stream())
    ctx.grads, ctx.dtypes, ctx.anchors_per_level = grads, [l.dtype for l in layers], [len(a) for a in anchors]
    return out


class DemoComputeLoss(nn.Module):
    """Base of the demos' ``ComputeLoss``: the host copy of the model's anchors and the target conversion."""
    empty_targets = None                         # the subclass's message for an empty target tensor

    def __init__(self):
        super().__init__()
        self.last_parts = None
        self._anchors = None                     # (key, host copy): reading model.anchors is a device sync, and not allowed inside a graph capture

    def get_model(self, model):
        return model.module if hasattr(model, 'module') else model

    def _inputs(self, predict_layers, target_all, model):
        """(targets fp32 on the heads' device, per level [(w, h), ...] at feature scale)"""
        model = self.get_model(model)
        require_gpu(predict_layers[0], 'ComputeLoss')
        key = tuple((a.data_ptr(), a._version) for a in model.anchors)
        if self._anchors is None or self._anchors[0] != key:
            self._anchors = (key, [[(float(w), float(h)) for w, h in a.reshape(-1, 2).tolist()] for a in model.anchors])   # feature scale
        if target_all.shape[0] == 0:
            raise RuntimeError(self.empty_targets)
        return target_all.detach().to(device=predict_layers[0].device, dtype=torch.float32).contiguous(), self._anchors[1]
