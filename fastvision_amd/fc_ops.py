"""Fully connected layers and the small losses of the two-stage head on the library's kernels.

The reference's Fast head runs RoI features through the VGG classifier ``Linear(25088, 4096) -> ReLU -> Dropout -> Linear(4096, 4096)
-> ReLU -> Dropout`` and two output layers (demos/faster_rcnn/models/vgg.py:41-47, fast.py:47-52), then ``F.cross_entropy`` /
``F.smooth_l1_loss`` (fast.py:192,197); the RPN uses its FocalLoss and ``F.smooth_l1_loss`` (rpn.py:8-64,303-312).

    linear_relu(x, lin)        relu(x @ W^T + b): a 1x1 convolution over R "pixels" on the implicit-GEMM kernel with the bias + ReLU
                               epilogue (fva_conv_fwd_bias_act); backward: ReLU mask + bias gradient in one pass
                               (fva_rows_relu_bwd + fva_colsum), then fva_conv_dgrad / fva_conv_wgrad
    dropout(x, drop, state)    nn.Dropout behind a ReLU: counter-based mask drawn on the device (fva_dropout_fwd), no stored mask
    linear(x, lin)             x @ W^T + b without activation, fp32 output: the detection head's biased 1x1 convolution (ops.HeadFn)
    cross_entropy_mean / focal_mean / smooth_l1_mean      value and gradient in one launch (fva_row_loss / fva_smooth_l1)

Rows are the RoIs (a few hundred), so these GEMMs stream their weights once: HBM-bound on the 205 MB bf16 copy of the first layer.
Activations in the compute dtype (bf16 or fp32), parameters and their gradients fp32.  No CPU path.
"""
import ctypes as C

import torch

from . import _lib
from .ops import HeadFn, _code, _p, _stream, get_compute_dtype, packed_weights, require_gpu

__all__ = ['linear_relu', 'dropout', 'new_dropout_state', 'linear', 'cross_entropy_mean', 'focal_mean', 'smooth_l1_mean']


def _packed_linear(weight, d, dtype):
    """(w_fwd, w_dgrad) of an nn.Linear weight [N, K] seen as a 1x1 filter; cached on the parameter until it changes and re-packed
    with every other layer in the one launch of the registry (the 103 M weights of the first VGG classifier layer took 1.1 ms per
    step in the single-layer pack kernel)."""
    if not weight.is_contiguous():
        raise RuntimeError('linear: the weight must be contiguous')
    return packed_weights(weight.detach().view(weight.shape[0], weight.shape[1], 1, 1), d, dtype, owner=weight)


class LinearReLUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, dtype):
        require_gpu(x, 'linear_relu')
        R, K = x.shape
        N = weight.shape[0]
        xs = x.detach()
        xs = xs if (xs.dtype == dtype and xs.is_contiguous()) else xs.to(dtype).contiguous()
        d = _lib.ConvDesc(_code(dtype), 1, R, 1, K, N, 1, 1, 0, 1)            # x: [1][R][1][K] NHWC without halo; dY gets a border of 1
        wf, wd = _packed_linear(weight, d, dtype)
        z = torch.empty((R, N), dtype=dtype, device=x.device)
        _lib.call('fva_conv_fwd_bias_act', C.byref(d), _p(xs), _p(wf), _p(bias.detach().float().contiguous()), 1, _p(z), 0, _stream())
        ctx.saved = (xs, z, d, wd, dtype, tuple(weight.shape))
        ctx.x_dtype, ctx.weight = x.dtype, weight
        return z

    @staticmethod
    def backward(ctx, dz):
        xs, z, d, wd, dtype, wshape = ctx.saved
        lib = _lib.load()
        R, N, dev, code = d.H, d.Cout, z.device, _code(dtype)
        g = dz if (dz.dtype == dtype and dz.is_contiguous()) else dz.to(dtype).contiguous()
        dy = torch.zeros((1, R + 2, 3, N), dtype=dtype, device=dev)           # halo buffer (W = 1): the kernels want a zero border
        rows = lib.fva_rows_relu_bwd_rows(R)
        part = torch.empty((rows, N), dtype=torch.float32, device=dev)
        _lib.call('fva_rows_relu_bwd', code, _p(g), _p(z), C.c_void_p(dy[0, 1, 1].data_ptr()), 3 * N, _p(part), R, N, 1, _stream())
        dbias = torch.empty(N, dtype=torch.float32, device=dev)
        srows = lib.fva_colsum_scratch_rows(rows)
        scratch = torch.empty((srows, N), dtype=torch.float32, device=dev) if srows else None
        _lib.call('fva_colsum', _p(part), rows, N, _p(dbias), _p(scratch) if srows else None, _stream())
        dw = torch.empty((wshape[0], wshape[1], 1, 1), dtype=torch.float32, device=dev)
        wsb = lib.fva_conv_wgrad_workspace(C.byref(d))
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        # on the launch stream, not the side stream: a fully connected layer may be applied several times in one forward pass (the
        # reference runs positives and negatives through the head separately), and autograd then SUMS the weight gradients of the
        # calls on the launch stream -- it must find them finished
        _lib.call('fva_conv_wgrad', C.byref(d), _p(xs), _p(dy), _p(dw), 0, _p(ws), wsb, _stream())
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty((R, d.Cin), dtype=dtype, device=dev)
            _lib.call('fva_conv_dgrad', C.byref(d), _p(dy), _p(wd), _p(dx), C.c_void_p(0), _stream())
            dx = dx if dx.dtype == ctx.x_dtype else dx.to(ctx.x_dtype)
        return dx, dw.view(wshape), dbias, None


def linear_relu(x, lin, dtype=None):
    """``relu(lin(x))`` for an ``nn.Linear`` with bias; x [R, in_features]."""
    dtype = dtype or get_compute_dtype()
    bk = 64 if dtype == torch.bfloat16 else 32
    if lin.bias is None or lin.in_features % bk or lin.out_features % 8:
        raise RuntimeError(f'linear_relu: in_features must be a multiple of {bk}, out_features of 8, with a bias')
    return LinearReLUFn.apply(x, lin.weight, lin.bias, dtype)


def rows_as(x, dtype):
    """x [R, N] (fp32 or bf16, any strides) as a contiguous tensor of ``dtype``: itself when it already is one, else converted by the
    library's strided pack kernel (fva_pack_nchw with R images of N channels and one pixel) -- no ATen cast or copy kernel."""
    if x.dtype == dtype and x.is_contiguous():
        return x
    if x.dim() != 2 or x.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError(f'fastvision_amd: expected a [rows, features] fp32 / bf16 tensor, got {tuple(x.shape)} {x.dtype}')
    out = torch.empty(x.shape, dtype=dtype, device=x.device)
    _lib.call('fva_pack_nchw', _code(dtype), _p(x), 1 if x.dtype == torch.bfloat16 else 0, x.stride(0), x.stride(1), 0, 0, _p(out), 0,
              x.shape[0], x.shape[1], 1, 1, _stream())
    return out


class DropoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p, state, dtype):
        require_gpu(x, 'dropout')
        xs = rows_as(x.detach(), dtype)
        out = torch.empty_like(xs)
        _lib.call('fva_dropout_fwd', _code(dtype), _p(xs), _p(out), xs.numel(), p, _p(state), _stream())
        ctx.save_for_backward(out)
        ctx.p, ctx.dtype, ctx.x_dtype = p, dtype, x.dtype
        return out

    @staticmethod
    def backward(ctx, g):
        dtype = ctx.dtype
        g = rows_as(g, dtype)
        dx = torch.empty_like(g)
        _lib.call('fva_dropout_bwd', _code(dtype), _p(g), _p(ctx.saved_tensors[0]), _p(dx), g.numel(), ctx.p, _stream())
        return rows_as(dx, ctx.x_dtype), None, None, None


def new_dropout_state(seed=None):
    """int64[4] = {seed, call counter, 0, 0}: the generator state of ``dropout`` (a CPU tensor; move it with the model).  ``seed`` defaults
    to ``torch.initial_seed()``, the value of the last ``torch.manual_seed`` -- read, not drawn, so building a model consumes nothing of
    torch's random stream and the parameter initialisation stays the reference's."""
    seed = torch.initial_seed() if seed is None else int(seed)
    return torch.tensor([seed & 0x7FFFFFFFFFFFFFFF, 0, 0, 0], dtype=torch.int64)


def dropout(x, drop, state, dtype=None):
    """``drop(x)`` for an ``nn.Dropout`` that FOLLOWS A RELU (x >= 0); ``drop.p`` and ``drop.training`` are read at call time.  Eval mode
    and p = 0 return ``x`` itself and launch nothing.  ``state``: a device tensor from ``new_dropout_state`` that every call advances on
    the device (Philox-4x32-10 keyed by seed, call counter and element index); the mask is not stored -- backward reads it off
    ``out != 0``, which behind a ReLU loses only gradients that the ReLU's own mask discards."""
    p = float(drop.p)
    if not drop.training or p == 0.0:
        return x
    require_gpu(x, 'dropout')
    if p >= 1.0:
        raise RuntimeError('dropout: p = 1 is not on this path')
    if state.dtype != torch.int64 or state.numel() != 4 or not state.is_cuda:
        raise RuntimeError('dropout: state must be the int64[4] device tensor of new_dropout_state()')
    return DropoutFn.apply(x, p, state, dtype or get_compute_dtype())


def linear(x, lin, dtype=None):
    """``lin(x)`` (no activation), fp32 result [R, out_features] -- the biased 1x1 head convolution over R rows."""
    dtype = dtype or get_compute_dtype()
    R, K = x.shape
    xs = x if (x.dtype == dtype and x.is_contiguous()) else x.to(dtype).contiguous()
    x4 = xs.view(1, R, 1, K).permute(0, 3, 1, 2)                              # logical [1, K, R, 1] view of the NHWC rows: zero-copy
    out = HeadFn.apply(x4, lin.weight.view(lin.out_features, K, 1, 1), lin.bias, dtype)
    return out.view(R, lin.out_features)


class _RowLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, mode, gamma):
        require_gpu(logits, 'row loss')
        z = logits.detach().float().contiguous()
        R, Cc = z.shape
        grad = torch.empty_like(z) if ctx.needs_input_grad[0] else None
        out = torch.empty(1, dtype=torch.float32, device=z.device)
        ws = torch.empty(R, dtype=torch.float32, device=z.device)
        _lib.call('fva_row_loss', _p(z), _p(labels.detach().long().contiguous()), R, Cc, mode, float(gamma), _p(out), _p(grad), _p(ws), _stream())
        ctx.grad, ctx.dtype = grad, logits.dtype
        return out.view(())

    @staticmethod
    def backward(ctx, gout):
        g = ctx.grad * gout
        return (g if g.dtype == ctx.dtype else g.to(ctx.dtype)), None, None, None


class _SmoothL1Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target):
        require_gpu(pred, 'smooth_l1')
        a, b = pred.detach().float().contiguous(), target.detach().float().contiguous()
        grad = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        out = torch.empty(1, dtype=torch.float32, device=a.device)
        ws = torch.empty(1024, dtype=torch.float32, device=a.device)
        _lib.call('fva_smooth_l1', _p(a), _p(b), a.numel(), _p(out), _p(grad), _p(ws), _stream())
        ctx.grad, ctx.dtype, ctx.shape = grad, pred.dtype, pred.shape
        return out.view(())

    @staticmethod
    def backward(ctx, gout):
        g = (ctx.grad * gout).view(ctx.shape)
        return (g if g.dtype == ctx.dtype else g.to(ctx.dtype)), None


def cross_entropy_mean(logits, labels):
    """F.cross_entropy(logits [R, C], labels [R], reduction='mean')"""
    return _RowLossFn.apply(logits, labels, 0, 0.0)


def focal_mean(logits, labels, gamma=2.0):
    """mean over rows of -(1 - p_t)^gamma * log p_t, p = softmax(logits) (the RPN's FocalLoss with alpha = 1, rpn.py:8-64)"""
    return _RowLossFn.apply(logits, labels, 1, gamma)


def smooth_l1_mean(pred, target):
    """F.smooth_l1_loss(pred, target, reduction='mean') (beta = 1)"""
    if pred.numel() == 0:
        return pred.sum() * 0.0
    return _SmoothL1Fn.apply(pred, target)
