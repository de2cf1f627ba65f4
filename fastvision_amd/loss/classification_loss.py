"""Classification losses -- API mirror of the reference's loss/classification_loss.py.

These two classes are the thin, standalone API surface (``CrossEntropyLoss`` is the CPU plumbing loss of
BASELINE config 1).  On the accelerated path ``Yolov3Loss`` does NOT call them: its class / objectness BCE
terms and their gradients are computed inside the fused HIP loss kernels (csrc/loss.hip), which restate
``BiCrossEntropyLoss`` exactly (1e-8 inside both logs, sum / numel).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

__all__ = ['one_hot', 'CrossEntropyLoss', 'BiCrossEntropyLoss']


def one_hot(y, num_classes):
    """datasets/common/id_2_onehot.py:10-15 (torch branch)."""
    col = y.view(-1, 1).long()
    return torch.zeros((col.size(0), num_classes)).to(y).scatter_(1, col, 1)


class _SoftmaxCEFn(torch.autograd.Function):
    """fva_softmax_ce (hard labels) or fva_softmax_ce_soft (label smoothing, a mixed pair of labels, dense probability rows): value and
    d loss / d logits in one pass over the rows (+ a one-block finish); backward scales the stored gradient by the upstream scalar on
    the device (fva_scale_by_device_scalar, an empty launch when it is exactly 1)."""

    @staticmethod
    def forward(ctx, y_pre, y_true, weights, mean, need_grad, smoothing, plan, dense):
        from .. import _lib
        from ..ops import _p, _stream, require_gpu
        require_gpu(y_pre, 'CrossEntropyLoss')
        R, Cc = y_pre.shape
        for name, t in (('y_true', y_true), ('weights', weights), ('the mix plan', plan)):
            # the kernel reads these through raw pointers: a tensor on another device (labels straight from a CPU loader) is refused
            # here, as torch's own ops refuse mixed devices, instead of being dereferenced on the GPU
            if t is not None and t.device != y_pre.device:
                raise RuntimeError(f'CrossEntropyLoss: {name} is on {t.device} but y_pre is on {y_pre.device}: move it to {y_pre.device} first')
        z = y_pre.detach()
        z = z if (z.dtype == torch.float32 and z.is_contiguous()) else z.float().contiguous()
        lab = y_true.detach()
        if dense:
            lab, code = (lab if lab.dtype == torch.float32 else lab.float()).contiguous(), _lib.LABEL_I64      # [R, C] probabilities
        else:
            if lab.numel() != R:
                raise RuntimeError(f'CrossEntropyLoss: {lab.numel()} labels for {R} rows')
            if lab.is_floating_point():
                lab, code = (lab if lab.dtype == torch.float32 else lab.float()).contiguous(), _lib.LABEL_F32
            else:
                lab, code = (lab if lab.dtype == torch.int64 else lab.long()).contiguous(), _lib.LABEL_I64
        w = None
        if weights is not None:
            w = weights.detach()
            w = (w if w.dtype == torch.float32 else w.float()).contiguous()
            if w.numel() != R:
                raise RuntimeError(f'CrossEntropyLoss: {w.numel()} weights for {R} rows')
        grad = torch.empty_like(z) if need_grad else None          # no [R, C] gradient under torch.no_grad() or for constant logits
        out = torch.empty(1, dtype=torch.float32, device=z.device)
        ws = torch.empty(max(_lib.load().fva_softmax_ce_workspace(R), 4), dtype=torch.uint8, device=z.device)
        reduction = _lib.REDUCE_MEAN if mean else _lib.REDUCE_SUM
        if smoothing == 0.0 and plan is None and not dense:
            _lib.call('fva_softmax_ce', _p(z), _p(lab), code, _p(w), R, Cc, reduction, _p(out), _p(grad), _p(ws), _stream())
        else:
            _lib.call('fva_softmax_ce_soft', _p(z), None if dense else _p(lab), code, _p(lab) if dense else None, _p(w), R, Cc, reduction,
                      smoothing, _p(plan), _p(out), _p(grad), _p(ws), _stream())
        ctx.grads, ctx.dtypes = [grad], [y_pre.dtype]
        return out.view(())

    @staticmethod
    def backward(ctx, gout):
        from ..ops import scale_loss_grads
        return scale_loss_grads(ctx, gout)[0], None, None, None, None, None, None, None


def _is_dense_target(y_pre, y_true):
    """torch's rule, a floating target of the input's shape holds probabilities -- except at C == 1, where [N, 1] float LABELS (which
    this class has always taken) have that shape too and stay labels."""
    return y_true.is_floating_point() and y_true.dim() == 2 and y_true.shape == y_pre.shape and y_pre.size(-1) > 1


class CrossEntropyLoss(nn.Module):
    """loss/classification_loss.py:8-33: ``forward(y_pre [N, C], y_true [N] or [N, 1] (integer or integral float), weights [N] or
    None)``, mean over N (not over the weights) or sum.  Device tensors run fva_softmax_ce (value and gradient in one launch, no host
    sync); a label outside [0, C) cannot raise there as the reference's ``scatter_`` does -- the loss comes back NaN instead.  Labels
    and weights must be on y_pre's device (RuntimeError otherwise, as torch raises for mixed devices).  On the device the gradient
    flows to y_pre only: weights that require grad are refused (RuntimeError) -- the reference would differentiate them -- and under
    ``torch.no_grad()`` (or for logits that need no gradient) only the value is computed.  CPU tensors run the reference's torch
    expression, weight gradients included.

    Beyond the reference: ``label_smoothing`` = eps turns the target t into (1 - eps) * t + eps / C (``F.cross_entropy``'s rule), and
    ``y_true`` may also be a float [N, C] tensor of probabilities (torch's soft-target form, C > 1) or the ``MixedLabels`` that
    ``fastvision_amd.BatchMix`` returns -- lambda is then read from its plan on the device.  These run fva_softmax_ce_soft; with
    ``label_smoothing == 0`` and plain labels the launch is fva_softmax_ce exactly as before."""

    def __init__(self, reduction='mean', label_smoothing=0.0):
        super().__init__()
        if not 0.0 <= float(label_smoothing) <= 1.0:
            raise ValueError(f'CrossEntropyLoss: label_smoothing = {label_smoothing} must lie in [0, 1]')
        self.reduction = reduction
        self.label_smoothing = float(label_smoothing)

    def forward(self, y_pre, y_true, weights=None):
        from ..mix import MixedLabels
        plan = None
        if isinstance(y_true, MixedLabels):
            y_true, plan = y_true.labels, y_true.plan
        dense = plan is None and _is_dense_target(y_pre, y_true)
        eps = self.label_smoothing
        if y_pre.is_cuda:
            grad_on = torch.is_grad_enabled()
            if grad_on and weights is not None and weights.requires_grad:
                raise RuntimeError('CrossEntropyLoss: on the device the gradient flows to y_pre only; pass weights.detach() '
                                   '(or compute the weighted loss on CPU tensors)')
            return _SoftmaxCEFn.apply(y_pre, y_true, weights, self.reduction == 'mean', grad_on and y_pre.requires_grad, eps, plan, dense)
        Cc = y_pre.size(-1)
        if dense:
            target = y_true.float()
        else:
            target = one_hot(y_true, Cc).float()
            if plan is not None:                            # row r pairs with row r - 1, as BatchMix paired the images
                lam = plan[2:3].view(torch.float32).to(target)
                target = lam * target + (1 - lam) * torch.roll(target, 1, 0)
        if eps != 0.0:
            target = target * (1 - eps) + eps / Cc
        loss = -torch.sum(target * F.log_softmax(y_pre, dim=-1), dim=1)
        if weights is not None:
            loss = loss * weights
        return torch.mean(loss) if self.reduction == 'mean' else torch.sum(loss)


class _BceFn(torch.autograd.Function):
    """fva_bce_loss: value and dl/dy in one launch (+ a one-block finish); backward scales the stored gradient."""

    @staticmethod
    def forward(ctx, y, label, dense, weights, C, already_sigmoid, mean):
        import ctypes as Ct
        from .. import _lib
        from ..ops import _p, _stream, require_gpu
        require_gpu(y, 'BiCrossEntropyLoss')
        yf = y.detach().float().contiguous().view(-1)
        numel = yf.numel()
        need = ctx.needs_input_grad[0]
        grad = torch.empty_like(yf) if need else None
        out = torch.empty(1, dtype=torch.float32, device=y.device)
        ws = torch.empty(1024, dtype=torch.float32, device=y.device)
        w = weights.detach().float().contiguous().view(-1) if weights is not None else None
        if w is not None and w.numel() not in (1, numel):
            w = w.expand(numel // w.numel(), w.numel()).contiguous().view(-1) if numel % w.numel() == 0 else w
        lab = label.detach().long().contiguous().view(-1) if label is not None else None
        den = dense.detach().float().contiguous().view(-1) if dense is not None else None
        _lib.call('fva_bce_loss', _p(yf), _p(lab), _p(den), _p(w), w.numel() if w is not None else 0, numel, C, 1 if already_sigmoid else 0,
                  1 if mean else 0, _p(out), _p(grad), _p(ws), _stream())
        ctx.grad, ctx.shape, ctx.dtype, ctx.scale = grad, y.shape, y.dtype, (1.0 / numel if mean else 1.0)
        return out.view(())

    @staticmethod
    def backward(ctx, gout):
        g = (ctx.grad * (gout * ctx.scale)).view(ctx.shape)
        return (g if g.dtype == ctx.dtype else g.to(ctx.dtype)), None, None, None, None, None, None


class BiCrossEntropyLoss(nn.Module):
    """loss/classification_loss.py:36-65 on the device: ``forward(y_pre, y_true, already_sigmoid=False, weights=None)``.  A last
    dimension > 1 means class scores with integer labels (one-hot targets); a last dimension of 1 a dense float target.  1e-8 sits
    inside both logarithms; ``mean`` divides the summed element losses by the element count.  Device tensors only (the reference's
    CPU use of this class, config 1's plumbing, goes through CrossEntropyLoss above)."""

    def __init__(self, reduction='mean'):
        super().__init__()
        self.reduction = reduction

    def forward(self, y_pre, y_true, already_sigmoid=False, weights=None):
        C = y_pre.size(-1)
        if C > 1:
            return _BceFn.apply(y_pre, y_true, None, weights, C, already_sigmoid, self.reduction == 'mean')
        return _BceFn.apply(y_pre, None, y_true, weights, 1, already_sigmoid, self.reduction == 'mean')
