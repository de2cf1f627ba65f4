"""What the classifier blocks of vgg_ops (VGG-bn) and resnet_ops (ResNet, ResNeXt) share: the ONE autograd node of a
Conv2d -> BatchNorm2d -> ReLU layer, its pieces, and the one max-pool node.

    ConvBNReLUFn                 relu(bn(conv(x) [+ b])): the convolution with (training) or without batch statistics, fva_bn_finalize /
                                 fva_bn_eval_coeffs, the BatchNorm + ReLU apply pass; backward = the two BatchNorm + ReLU passes (training) or the
                                 one-pass frozen-statistics backward (ops.frozen_bn_bwd), then the convolution's weight and data gradients.
                                 The convolution is a back end: PlainConv (implicit GEMM on the packed weights, 1x1 / 3x3, stride 1 / 2) or
                                 GroupedConv (fva_gconv_* on the fp32 master weight, or fva_gconv_mfma_* on its packed tables).  A convolution
                                 bias (VGG) changes three launches and the dbias rule, see the node's docstring
    MaxPoolFn                    max_pool2 / max_pool3s2: two entry-point names and an output-size rule
    _conv_bn, _bn_relu_apply, _bn_relu_bwd, _bn_add_relu_bwd_identity, _block_bn_relu_bwd
                                 the pieces, also used by resnet_ops' stem and BatchNorm + add + ReLU tail

The public functions, their argument checks and the ``_Link`` between a residual block's first node and its tail stay with vgg_ops / resnet_ops.
No CPU path.
"""
import ctypes as C

import torch

from . import _lib
from .ops import (_code, _grad_like, _p, _released, _stream, _wgrad_dgrad, flush_pending_apply, frozen_bn_bwd, halo_alloc, packed_weights,
                  require_gpu, to_dense, to_halo, wgrad_stream)


def _check_bn(bn, who):
    if not bn.affine:
        raise RuntimeError(f'{who}: the BatchNorm2d must be affine')
    if bn.training and bn.momentum is None and bn.track_running_stats:
        raise RuntimeError(f'{who}: momentum=None (cumulative average) is not on this path')
    return bn.training or not bn.track_running_stats


def _conv_bn(d, x_ptr, wf, gamma, beta, bn, training, M, dev, dtype, who, fwd='fva_conv_fwd', blocks='fva_conv_stat_blocks', bias=None):
    """The convolution with (training) or without batch statistics and the BatchNorm coefficients: (y, scale, shift, mean, rstd).
    ``fwd`` / ``blocks``: the forward launch and its statistics-block count (the grouped 3x3: fva_gconv_fwd / fva_gconv_stat_blocks on a
    GConvDesc and the fp32 master weight).  ``bias``: the fp32 convolution bias in front of the BatchNorm; the convolution runs without it
    (ConvBNReLUFn's docstring), running_mean and the eval-mode shift account for it."""
    lib = _lib.load()
    Cout = d.C if isinstance(d, _lib.GConvDesc) else d.Cout
    y = torch.empty((M, Cout), dtype=dtype, device=dev)
    scale = torch.empty(Cout, dtype=torch.float32, device=dev)
    shift = torch.empty_like(scale)
    mean = rstd = None
    if training:
        nblk = getattr(lib, blocks)(C.byref(d))
        stats = torch.empty((lib.fva_bn_partial_rows(nblk), 2, Cout), dtype=torch.float32, device=dev)
        mean, rstd = torch.empty_like(scale), torch.empty_like(scale)
        _lib.call(fwd, C.byref(d), C.c_void_p(x_ptr), _p(wf), _p(y), _p(stats), _stream())
        _lib.call('fva_bn_finalize', _p(stats), nblk, stats.shape[0], M, Cout, _p(gamma), _p(beta), _p(bn.rm), _p(bn.rv), _p(bn.nbt),
                  bn.momentum, bn.eps, _p(mean), _p(rstd), _p(scale), _p(shift), _stream())
        if bias is not None and bn.rm is not None:
            _lib.call('fva_bn_bias_running_mean', Cout, _p(bn.rm), _p(bias), bn.momentum, _stream())
    else:
        if bn.rm is None:
            raise RuntimeError(f'{who}: eval mode needs running statistics (track_running_stats=True)')
        _lib.call(fwd, C.byref(d), C.c_void_p(x_ptr), _p(wf), _p(y), C.c_void_p(0), _stream())
        if bias is not None:
            _lib.call('fva_bn_eval_coeffs_bias', Cout, _p(gamma), _p(beta), _p(bn.rm), _p(bn.rv), _p(bias), bn.eps, _p(scale), _p(shift), _stream())
        else:
            _lib.call('fva_bn_eval_coeffs', Cout, _p(gamma), _p(beta), _p(bn.rm), _p(bn.rv), bn.eps, _p(scale), _p(shift), _stream())
    return y, scale, shift, mean, rstd


def _wide(code, Cout):
    """fva_bn_relu_* serve at most 256 16-byte chunks per pixel: 2048 channels in bf16, 1024 in fp32.  Wider fp32 tensors (the 2048
    channels of resnext101_32x8d's res5, in the fp32 parity runs) take the BatchNorm + add + ReLU passes with a zero addend instead."""
    return Cout // (8 if code == _lib.BF16 else 4) > 256


WIDE_FROZEN = ('conv_bn_relu: backward with frozen statistics (the BatchNorm in eval mode) through an fp32 tensor wider than 1024 channels is not '
               'on this path -- the one-pass frozen backward serves at most 256 16-byte chunks per pixel; run it in bf16, or keep the BatchNorm in '
               'training mode')


def _bn_relu_apply(code, y, scale, shift, zbuf, B, H, W, Cout):
    """z = relu(y * scale + shift) into the halo buffer zbuf (border 1)."""
    if not _wide(code, Cout):
        _lib.call('fva_bn_relu_apply', code, _p(y), _p(scale), _p(shift), _p(zbuf), 1, B, H, W, Cout, _stream())
        return
    none = C.c_void_p(0)
    r = torch.zeros((B, H, W, Cout), dtype=y.dtype, device=y.device)
    _lib.call('fva_bn_add_relu_apply', code, _p(y), _p(scale), _p(shift), _p(r), 0, none, none, none, _p(zbuf), 1, B, H, W, Cout, _stream())


def _bn_add_relu_bwd_identity(code, dz_ptr, y, scale, shift, mean, rstd, gamma, r_ptr, r_pad, B, H, W, Cout, dtype):
    """The BatchNorm + add + ReLU backward in the identity form (training mode), z = relu(bn(y) + r) with r a halo buffer of border
    ``r_pad``: reduce, fva_bn_bwd_finalize, apply.  Returns (dy halo, dr dense = dU, dgamma, dbeta)."""
    lib, dev, M = _lib.load(), y.device, B * H * W
    f32 = dict(dtype=torch.float32, device=dev)
    nb = lib.fva_bn_add_relu_bwd_blocks(code, M, Cout)
    rows = lib.fva_bn_partial_rows(nb)
    part = torch.empty((rows, 2, Cout), **f32)
    dgamma, dbeta, coef = torch.empty(Cout, **f32), torch.empty(Cout, **f32), torch.empty((3, Cout), **f32)
    dy = torch.empty((B, H + 2, W + 2, Cout), dtype=dtype, device=dev)
    dr = torch.empty((B, H, W, Cout), dtype=dtype, device=dev)
    main = (code, C.c_void_p(dz_ptr), _p(y), _p(scale), _p(shift), _p(mean), _p(rstd))
    _lib.call('fva_bn_add_relu_bwd_reduce', *main, C.c_void_p(r_ptr), r_pad, None, None, None, None, None, _p(part), None, nb, B, H, W, Cout,
              _stream())
    _lib.call('fva_bn_bwd_finalize', _p(part), nb, rows, M, Cout, _p(gamma), _p(rstd), _p(dgamma), _p(dbeta), 0, _p(coef), _stream())
    _lib.call('fva_bn_add_relu_bwd_apply', *main, _p(coef), C.c_void_p(r_ptr), r_pad, None, None, None, None, None, None, _p(dy), None, 1, _p(dr),
              B, H, W, Cout, _stream())
    return dy, dr, dgamma, dbeta


def _bn_relu_bwd(code, dz_ptr, y, scale, shift, mean, rstd, gamma, B, H, W, Cout, dtype):
    """The two BatchNorm + ReLU backward passes (training mode): (dy halo, dgamma, dbeta)."""
    if _wide(code, Cout):
        # through the add + ReLU passes with a zero addend; the addend's gradient is dropped
        r = torch.zeros((B, H, W, Cout), dtype=dtype, device=y.device)
        dy, _, dgamma, dbeta = _bn_add_relu_bwd_identity(code, dz_ptr, y, scale, shift, mean, rstd, gamma, r.data_ptr(), 0, B, H, W, Cout, dtype)
        return dy, dgamma, dbeta
    lib, dev, M = _lib.load(), y.device, B * H * W
    nb = lib.fva_bn_bwd_blocks(code, M, Cout)
    part = torch.empty((lib.fva_bn_partial_rows(nb), 2, Cout), dtype=torch.float32, device=dev)
    _lib.call('fva_bn_relu_bwd_reduce', code, C.c_void_p(dz_ptr), _p(y), _p(scale), _p(shift), _p(mean), _p(rstd), _p(part), nb, M, Cout, _stream())
    dgamma = torch.empty(Cout, dtype=torch.float32, device=dev)
    dbeta = torch.empty_like(dgamma)
    coef = torch.empty((3, Cout), dtype=torch.float32, device=dev)
    _lib.call('fva_bn_bwd_finalize', _p(part), nb, part.shape[0], M, Cout, _p(gamma), _p(rstd), _p(dgamma), _p(dbeta), 0, _p(coef), _stream())
    dy = torch.empty((B, H + 2, W + 2, Cout), dtype=dtype, device=dev)
    _lib.call('fva_bn_relu_bwd_apply', code, C.c_void_p(dz_ptr), _p(y), _p(scale), _p(shift), _p(mean), _p(rstd), _p(coef), _p(dy), 1,
              B, H, W, Cout, _stream())
    return dy, dgamma, dbeta


def _block_bn_relu_bwd(training, code, dz_ptr, y, scale, shift, mean, rstd, gamma, bn, bias, B, H, W, Cout, dtype, need_gamma, need_beta,
                       need_bias=False):
    """The BatchNorm + ReLU backward of a block: (dy halo, dgamma, dbeta, dbias).  Training mode: _bn_relu_bwd (dbias is None: the
    caller's rule).  Frozen statistics: one pass, and only what autograd asks for; ``bias``: the fp32 convolution bias in front of the
    BatchNorm, or None."""
    if training:
        return _bn_relu_bwd(code, dz_ptr, y, scale, shift, mean, rstd, gamma, B, H, W, Cout, dtype) + (None,)
    if _wide(code, Cout):
        raise RuntimeError(WIDE_FROZEN)
    dy = torch.empty((B, H + 2, W + 2, Cout), dtype=dtype, device=y.device)
    return (dy,) + frozen_bn_bwd('relu', code, dz_ptr, y, scale, shift, bn, bias, dy, 1, B, H, W, Cout, need_gamma, need_beta, need_bias)


# ------------------------------------------------------------------------------------------------ the two convolutions
class PlainConv:
    """``groups == 1``: the implicit-GEMM kernels on the packed weights (cached on a leaf weight, ops.packed_weights)."""
    fwd, blocks = 'fva_conv_fwd', 'fva_conv_stat_blocks'

    def __init__(self, k, stride):
        self.k, self.stride = k, stride

    def operands(self, code, B, Cin, H, W, x_pad, weight, dtype):
        """(descriptor, forward weight operand, backward weight operand)"""
        d = _lib.ConvDesc(code, B, H, W, Cin, weight.shape[0], self.k, self.stride, x_pad, 1)
        return (d,) + tuple(packed_weights(weight, d, dtype, cache=weight.is_leaf))

    def backward(self, d, x_ptr, dy, wd, wshape, keep, weight, need_x, need_w, addend):
        """(dx dense or None, dw or None); ``addend``: a tensor that the data gradient adds in its epilogue (the _Link of a residual block)."""
        return _wgrad_dgrad(d, x_ptr, dy, wd, wshape, (keep,), weight, need_x, addend_ptr=None if addend is None else addend.data_ptr(),
                            need_dw=need_w)


class GroupedConv:
    """``groups > 1``, 3x3.  ``path`` (resnet_ops.set_grouped_path) routes per layer:
    'plain': fva_gconv_fwd / _dgrad / _wgrad on the fp32 master weight (no packed copy, nothing registered with ops._PackRegistry).
    'mfma':  where fva_gconv_mfma_serves(d) == 1 (bf16, stride 1, border 1, a map that fits the staging) the matrix-unit kernels:
             operands() launches fva_gconv_mfma_pack in front of every forward (not cached: a captured step replays it on the weights the
             optimizer has just written) and the forward / backward take the two packed tables; every other layer takes the plain launches.
    Its data gradient takes no addend: a tail's summand comes back through autograd."""
    k, fwd, blocks = 3, 'fva_gconv_fwd', 'fva_gconv_stat_blocks'
    wgrad, wgrad_ws, dgrad = 'fva_gconv_wgrad', 'fva_gconv_wgrad_workspace', 'fva_gconv_dgrad'

    def __init__(self, groups, stride, path='plain'):
        self.groups, self.stride, self.path = groups, stride, path

    def operands(self, code, B, Cin, H, W, x_pad, weight, dtype):
        w = weight.detach()
        if w.dtype != torch.float32 or not w.is_contiguous():
            w = w.float().contiguous()
        d = _lib.GConvDesc(code, B, H, W, Cin, self.groups, self.stride, x_pad, 1)
        lib = _lib.load()
        if self.path != 'mfma' or lib.fva_gconv_mfma_serves(C.byref(d)) != 1:
            return d, w, w
        self.fwd, self.blocks = 'fva_gconv_mfma_fwd', 'fva_gconv_mfma_stat_blocks'
        self.wgrad, self.wgrad_ws, self.dgrad = 'fva_gconv_mfma_wgrad', 'fva_gconv_mfma_wgrad_workspace', 'fva_gconv_mfma_dgrad'
        nb = lib.fva_gconv_mfma_pack_bytes(C.byref(d))
        wf = torch.empty(nb, dtype=torch.uint8, device=w.device)
        wb = torch.empty_like(wf)
        _lib.call('fva_gconv_mfma_pack', C.byref(d), _p(w), _p(wf), _p(wb), _stream())
        return d, wf, wb

    def backward(self, d, x_ptr, dy, w, wshape, keep, weight, need_x, need_w, addend):
        assert addend is None
        dw = dxb = None
        if need_w:
            dw = torch.empty(wshape, dtype=torch.float32, device=dy.device)
            wsb = getattr(_lib.load(), self.wgrad_ws)(C.byref(d))
            ws = torch.empty(wsb, dtype=torch.uint8, device=dy.device)
            _lib.call(self.wgrad, C.byref(d), C.c_void_p(x_ptr), _p(dy), _p(dw), _p(ws), wsb, wgrad_stream((keep, dy, ws), weight))
        if need_x:
            dxb = torch.empty((d.B, d.H, d.W, d.C), dtype=dy.dtype, device=dy.device)
            _lib.call(self.dgrad, C.byref(d), _p(dy), _p(w), _p(dxb), _stream())
        return dxb, dw


# ------------------------------------------------------------------------------------------------ conv -> BN -> ReLU
class ConvBNReLUFn(torch.autograd.Function):
    """``relu(bn(conv(x) [+ b]))``; autograd inputs x, weight, bias (may be None), gamma, beta.  ``conv``: PlainConv or GroupedConv.
    ``link``: resnet_ops._Link or None.  Saved state is kept iff ``grad_on`` (torch.is_grad_enabled() at call time) and some input asks
    for a gradient; the backward pass that uses it releases it.

    The bias cancels in the training-mode output (the batch mean takes it away again), so the convolution runs without it and the bias is
    accounted for where it stays visible (_conv_bn's two bias launches): running_mean tracks mean(y) + b and the eval-mode shift is
    beta + (b - running_mean) * scale.  Its gradient is the channel sum of dy, which the BatchNorm backward
    makes zero up to rounding: returned as exact zeros (a real fp32 tensor, for optimizers with weight decay).  With frozen statistics
    (the BatchNorm in eval mode, gradients on) nothing cancels: u = (y + b - running_mean) * scale_bn + beta, the one-pass backward
    (ops.frozen_bn_bwd, ReLU form) takes m = running_mean - b, and dbias = scale * sum dU is a real gradient."""

    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, bn, training, dtype, conv, link, grad_on):
        require_gpu(x, 'conv_bn_relu')
        flush_pending_apply()
        B, Cin, H, W = x.shape
        Cout, dev, code = weight.shape[0], x.device, _code(dtype)
        keep, x_ptr, x_pad = to_halo(x.detach(), dtype, conv.k // 2)
        d, wf, wb = conv.operands(code, B, Cin, H, W, x_pad, weight, dtype)
        b32 = None if bias is None else bias.detach().float().contiguous()
        OH, OW = (H - 1) // conv.stride + 1, (W - 1) // conv.stride + 1
        y, scale, shift, mean, rstd = _conv_bn(d, x_ptr, wf, gamma, beta, bn, training, B * OH * OW, dev, dtype, 'conv_bn_relu', conv.fwd,
                                               conv.blocks, b32)
        zbuf, z = halo_alloc(B, Cout, OH, OW, dtype, dev, 1)
        _bn_relu_apply(code, y, scale, shift, zbuf, B, OH, OW, Cout)
        need = grad_on and any(ctx.needs_input_grad)
        ctx.saved = (keep, x_ptr, y, scale, shift, mean, rstd, d, wb, dtype, tuple(weight.shape), gamma, OH, OW) if need else None
        ctx.training, ctx.bn, ctx.bias = training, (None if training else bn), b32
        ctx.x_like, ctx.weight, ctx.conv, ctx.link = x, weight, conv, link
        if need and link is not None:
            link.shape, link.dtype, link.x_ptr, link.open = tuple(x.shape), dtype, x_ptr, True
        return z

    @staticmethod
    def backward(ctx, dz):
        if ctx.saved is None:
            raise _released('conv_bn_relu')
        keep, x_ptr, y, scale, shift, mean, rstd, d, wb, dtype, wshape, gamma, OH, OW = ctx.saved
        B, Cout, code = d.B, y.shape[1], _code(dtype)
        link, addend = ctx.link, None
        if link is not None:
            link.open = False                                   # a tail that runs its backward later keeps its summand for autograd
            addend, link.addend = link.addend, None
        keep_dz, dz_ptr = to_dense(dz, dtype)
        need_x, need_w, need_bias, need_g, need_b = ctx.needs_input_grad[:5]
        dy, dgamma, dbeta, dbias = _block_bn_relu_bwd(ctx.training, code, dz_ptr, y, scale, shift, mean, rstd, gamma, ctx.bn, ctx.bias,
                                                      B, OH, OW, Cout, dtype, need_g, need_b, need_bias)
        dxb, dw = ctx.conv.backward(d, x_ptr, dy, wb, wshape, keep, ctx.weight, need_x, need_w or ctx.training, addend)
        dx = _grad_like(dxb, ctx.x_like) if dxb is not None else None
        if ctx.training and ctx.bias is not None:
            dbias = torch.zeros(Cout, dtype=torch.float32, device=y.device)
        ctx.saved = ctx.x_like = ctx.weight = ctx.bn = ctx.bias = ctx.conv = ctx.link = None      # released by the backward pass that used them
        return dx, dw, dbias, dgamma, dbeta, None, None, None, None, None, None


# ------------------------------------------------------------------------------------------------ max pool
class MaxPoolFn(torch.autograd.Function):
    """``who``: the public name; ``fwd`` / ``bwd``: the two entry points; ``out_size``: output height / width from the input's.  Backward
    recomputes the first maximum from x."""

    @staticmethod
    def forward(ctx, x, dtype, who, fwd, bwd, out_size):
        require_gpu(x, who)
        flush_pending_apply()
        B, Cc, H, W = x.shape
        keep, x_ptr, x_pad = to_halo(x.detach(), dtype, 0)
        obuf, out = halo_alloc(B, Cc, out_size(H), out_size(W), dtype, x.device, 1)
        _lib.call(fwd, _code(dtype), C.c_void_p(x_ptr), x_pad, _p(obuf), 1, B, H, W, Cc, _stream())
        ctx.saved = (keep, x_ptr, x_pad, (B, Cc, H, W), dtype, bwd)
        ctx.x_like = x
        return out

    @staticmethod
    def backward(ctx, dz):
        keep, x_ptr, x_pad, (B, Cc, H, W), dtype, bwd = ctx.saved
        keep_dz, dz_ptr = to_dense(dz, dtype)
        dxb = torch.empty((B, H, W, Cc), dtype=dtype, device=dz.device)
        _lib.call(bwd, _code(dtype), C.c_void_p(dz_ptr), C.c_void_p(x_ptr), x_pad, _p(dxb), B, H, W, Cc, _stream())
        return _grad_like(dxb, ctx.x_like), None, None, None, None, None
