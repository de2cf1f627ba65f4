"""ResNet blocks on the HIP kernels (reference classfication/models/resnet.py).

    stem_bn_relu(x, conv, bn)        the 7x7 / stride 2 / pad 3 stem + BatchNorm + ReLU: fva_stem7_patches, then the 1x1 implicit GEMM over the
                                     patch matrix, fva_bn_finalize, fva_bn_relu_apply; backward = the BatchNorm + ReLU passes, then fva_conv_wgrad
                                     over the same patch matrix (the images get no gradient)
    max_pool3s2(x)                   MaxPool2d(3, 2, 1); backward recomputes the first maximum from x
    conv_bn_relu(x, conv, bn)        bias-free Conv2d (1x1 s1, 3x3 s1, 3x3 s2) -> BatchNorm2d -> ReLU: conv_bn_ops.ConvBNReLUFn, the node that
                                     vgg_ops.conv_bn_relu runs too, without a bias; frozen statistics take the one-pass backward.  A grouped
                                     3x3 (ResNeXt's conv2; GROUPED_CONTRACT) is the same node on conv_bn_ops.GroupedConv (fva_gconv_*, or
                                     fva_gconv_mfma_* under set_grouped_path('mfma'))
    conv_bn_add_relu(x, conv, bn, identity)
    conv_bn_add_relu(x, conv, bn, shortcut_in, shortcut_conv, shortcut_bn)
                                     the tail of a residual block, relu(bn(conv(x)) + R) with the add INSIDE the ReLU, one autograd node:
                                     R = the identity, or bn_d(conv_d(shortcut_in)) with conv_d a 1x1 convolution of stride 1 or 2 (stride 2:
                                     fva_subsample2_fwd, then the 1x1 stride-1 convolution).  Its backward returns both branch gradients.

The gradient of a block's input has two summands: what the main branch's first convolution hands back and what the tail hands to the
identity / the shortcut.  When the tail's second operand is the very tensor the block's first conv_bn_relu consumed, the tail leaves its
summand with that node (``_Link``) and returns None for it; the node's fva_conv_dgrad takes it as its ``addend`` -- no separate add.
Any other wiring gets the summand back through autograd as usual.

Activations stay in the halo NHWC layout between blocks, in the compute dtype; parameters and their gradients are fp32; running
statistics and num_batches_tracked are updated on the device; nothing synchronises the host.  No CPU path.

The conv -> BatchNorm -> ReLU node, the max-pool node and the BatchNorm + ReLU pieces that the stem and the tail use are conv_bn_ops';
this module keeps the public functions, their argument checks, the stem, the tail and the ``_Link``.
"""
import ctypes as C

import torch

from . import _lib
from .conv_bn_ops import (WIDE_FROZEN, ConvBNReLUFn, GroupedConv, MaxPoolFn, PlainConv, _block_bn_relu_bwd, _bn_add_relu_bwd_identity, _check_bn,  # noqa: F401
                          _conv_bn, _wide)
from .ops import (_BNState, _code, _grad_like, _p, _released, _stream, _wgrad_dgrad, flush_pending_apply, get_compute_dtype, halo_alloc,
                  packed_weights, require_gpu, to_dense, to_halo)

__all__ = ['stem_bn_relu', 'max_pool3s2', 'conv_bn_relu', 'conv_bn_add_relu', 'set_grouped_path', 'get_grouped_path']

FROZEN_TAIL = ('conv_bn_add_relu: backward through a BatchNorm + add + ReLU tail with frozen statistics (the BatchNorm in eval mode) is out of '
               'scope -- run eval-mode forwards under torch.no_grad(), or keep the BatchNorm layers of a ResNet in training mode')


class _Link:
    """What the first conv_bn_relu of a block and the block's tail share: the tail's summand of the block input's gradient."""
    __slots__ = ('shape', 'dtype', 'x_ptr', 'open', 'taken', 'addend')

    def __init__(self):
        self.shape = self.dtype = self.x_ptr = self.addend = None
        self.open = self.taken = False


# ------------------------------------------------------------------------------------------------ the stem
class StemBNReLUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, images, weight, gamma, beta, bn, training, dtype, grad_on):
        require_gpu(images, 'stem_bn_relu')
        flush_pending_apply()
        lib = _lib.load()
        img = images.detach()
        if img.dtype != torch.float32 or not img.is_contiguous():
            img = img.float().contiguous()
        B, Cin, H, W = img.shape
        Cout, dev, code = weight.shape[0], img.device, _code(dtype)
        OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        K, Kp, M = Cin * 49, lib.fva_stem7_kp(code, Cin), B * OH * OW
        P = torch.empty((M, Kp), dtype=dtype, device=dev)
        _lib.call('fva_stem7_patches', code, _p(img), _p(P), B, Cin, H, W, _stream())
        # the filter as a 1x1 one over the patch columns, zero behind column Cin * 49
        wpad = torch.zeros((Cout, Kp, 1, 1), dtype=torch.float32, device=dev)
        wpad.view(Cout, Kp)[:, :K].copy_(weight.detach().reshape(Cout, K))
        d = _lib.ConvDesc(code, B, OH, OW, Kp, Cout, 1, 1, 0, 1)
        wf, _ = packed_weights(wpad, d, dtype, cache=False)
        y, scale, shift, mean, rstd = _conv_bn(d, P.data_ptr(), wf, gamma, beta, bn, training, M, dev, dtype, 'stem_bn_relu')
        zbuf, z = halo_alloc(B, Cout, OH, OW, dtype, dev, 1)
        _lib.call('fva_bn_relu_apply', code, _p(y), _p(scale), _p(shift), _p(zbuf), 1, B, OH, OW, Cout, _stream())
        need = grad_on and any(ctx.needs_input_grad)
        ctx.saved = (P, y, scale, shift, mean, rstd, d, dtype, tuple(weight.shape), gamma) if need else None
        ctx.training, ctx.bn = training, (None if training else bn)
        return z

    @staticmethod
    def backward(ctx, dz):
        if ctx.saved is None:
            raise _released('stem_bn_relu')
        P, y, scale, shift, mean, rstd, d, dtype, wshape, gamma = ctx.saved
        ctx.saved = None
        lib = _lib.load()
        B, OH, OW, Cout, Kp, dev, code = d.B, d.H, d.W, d.Cout, d.Cin, y.device, _code(dtype)
        keep_dz, dz_ptr = to_dense(dz, dtype)
        need_w, need_g, need_b = ctx.needs_input_grad[1:4]
        dy, dgamma, dbeta, _ = _block_bn_relu_bwd(ctx.training, code, dz_ptr, y, scale, shift, mean, rstd, gamma, ctx.bn, None, B, OH, OW, Cout,
                                                  dtype, need_g, need_b)
        ctx.bn = None
        dw = None
        if need_w or ctx.training:
            # on the launch stream: the slice below reads dW right away
            dwp = torch.empty((Cout, Kp), dtype=torch.float32, device=dev)
            wsb = lib.fva_conv_wgrad_workspace(C.byref(d))
            ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
            _lib.call('fva_conv_wgrad', C.byref(d), _p(P), _p(dy), _p(dwp), 0, _p(ws), wsb, _stream())
            dw = dwp[:, :wshape[1] * 49].reshape(wshape)          # columns ci * 49 + kh * 7 + kw: OIHW as they stand
        return None, dw, dgamma, dbeta, None, None, None, None


def stem_bn_relu(x, conv, bn, dtype=None):
    """``relu(bn(conv(x)))`` for the stem ``nn.Conv2d(Cin, Cout, 7, stride 2, padding 3, bias=False)`` on fp32 NCHW images."""
    if (conv.kernel_size != (7, 7) or conv.stride != (2, 2) or conv.padding != (3, 3) or conv.bias is not None or conv.groups != 1
            or conv.dilation != (1, 1)):
        raise RuntimeError('stem_bn_relu: only the ResNet stem (7x7, stride 2, padding 3, no bias) is on this path')
    if x.requires_grad:
        raise RuntimeError('stem_bn_relu: the stem does not produce a gradient for the input images (x.requires_grad is set)')
    training = _check_bn(bn, 'stem_bn_relu')
    return StemBNReLUFn.apply(x, conv.weight, bn.weight, bn.bias, _BNState(bn), training, dtype or get_compute_dtype(), torch.is_grad_enabled())


# ------------------------------------------------------------------------------------------------ MaxPool2d(3, 2, 1)
def max_pool3s2(x, dtype=None):
    """``nn.MaxPool2d(kernel_size=3, stride=2, padding=1)``"""
    return MaxPoolFn.apply(x, dtype or get_compute_dtype(), 'max_pool3s2', 'fva_maxpool3s2_fwd', 'fva_maxpool3s2_bwd', lambda n: (n - 1) // 2 + 1)


# ------------------------------------------------------------------------------------------------ conv -> BN -> ReLU
def _conv_geometry(conv, who, allowed, grouped=False):
    k, s, p = conv.kernel_size, conv.stride, conv.padding
    if (k[0] != k[1] or s[0] != s[1] or (k[0], s[0]) not in allowed or p != (k[0] // 2, k[0] // 2) or conv.bias is not None
            or (conv.groups != 1 and not (grouped and k[0] == 3)) or conv.dilation != (1, 1)):
        raise RuntimeError(f'{who}: a bias-free Conv2d with (kernel, stride) in {sorted(allowed)} and padding kernel // 2 is on this path; got {conv}')
    return k[0], s[0]


def _even_map(x, stride, who):
    if stride == 2 and ((x.shape[2] | x.shape[3]) & 1):
        raise RuntimeError(f'{who}: a stride-2 block needs an even map, got {x.shape[2]} x {x.shape[3]} (odd map in front of a stride-2 block)')


GROUPED_CONTRACT = ('conv_bn_relu: a grouped convolution is on this path as a 3x3 of stride 1 or 2 with in_channels == out_channels == C, '
                    'C = groups * Cg, Cg in {4, 8, 16, 32, 64}, C % 64 == 0 and C <= 2048')


# Which kernels a grouped 3x3 takes.  'plain' (the default): the FMA kernels of grouped.hip at every layer, the launches every recorded
# sequence and every earlier measurement were made with.  'mfma': the matrix-unit kernels of grouped_mfma.hip at the layers they serve (bf16,
# stride 1); stride 2 and fp32 stay plain.  The default moves only once the measured table of DESIGN 3.12 says it should.
_GROUPED = {'path': 'plain'}


def set_grouped_path(mode):
    """'plain' | 'mfma' (see above).  Returns the previous mode."""
    if mode not in ('plain', 'mfma'):
        raise ValueError("grouped path must be 'plain' or 'mfma'")
    prev, _GROUPED['path'] = _GROUPED['path'], mode
    return prev


def get_grouped_path():
    """The path in force for grouped 3x3 layers: 'plain' or 'mfma'."""
    return _GROUPED['path']


def _check_grouped(x, conv):
    Cc, groups = conv.in_channels, conv.groups
    if conv.out_channels != Cc or Cc % groups or Cc // groups not in (4, 8, 16, 32, 64) or Cc % 64 or Cc > 2048 or x.shape[1] != Cc:
        raise RuntimeError(f'{GROUPED_CONTRACT}; got {conv} on an input of {x.shape[1]} channels')


def conv_bn_relu(x, conv, bn, dtype=None):
    """``relu(bn(conv(x)))`` for a bias-free ``nn.Conv2d`` of 1x1 stride 1, 3x3 stride 1 or 3x3 stride 2 (padding kernel // 2) followed by
    ``nn.BatchNorm2d``; the module's ``training`` flag, momentum and eps are read at call time.  The 3x3 may be grouped (GROUPED_CONTRACT)."""
    k, stride = _conv_geometry(conv, 'conv_bn_relu', {(1, 1), (3, 1), (3, 2)}, grouped=True)
    _even_map(x, stride, 'conv_bn_relu')
    grouped, grad_on = conv.groups != 1, torch.is_grad_enabled()
    if grouped:
        _check_grouped(x, conv)
    training = _check_bn(bn, 'conv_bn_relu')
    back_end = GroupedConv(conv.groups, stride, _GROUPED['path']) if grouped else PlainConv(k, stride)
    link = _Link() if grad_on and not grouped else None         # the grouped data gradient takes no addend: no link to the block's tail
    z = ConvBNReLUFn.apply(x, conv.weight, None, bn.weight, bn.bias, _BNState(bn), training, dtype or get_compute_dtype(), back_end, link, grad_on)
    if link is not None and link.open:
        x._fva_block_in = link                                  # a tail whose second operand is this very tensor finds the node here
    return z


# ------------------------------------------------------------------------------------------------ conv -> BN -> (+ R) -> ReLU
class ConvBNAddReLUFn(torch.autograd.Function):
    """Arguments 0..3: the main branch (x, weight, gamma, beta); 4: the second operand (the identity, or the shortcut's input); 5..7: the
    shortcut's weight, gamma, beta (None in the identity form)."""

    @staticmethod
    def forward(ctx, x, weight, gamma, beta, other, w_d, gamma_d, beta_d, bn, bn_d, training, dtype, k, stride_d, link, grad_on):
        require_gpu(x, 'conv_bn_add_relu')
        flush_pending_apply()
        B, Cin, H, W = x.shape
        Cout, dev, code = weight.shape[0], x.device, _code(dtype)
        M = B * H * W
        keep, x_ptr, x_pad = to_halo(x.detach(), dtype, k // 2)
        d = _lib.ConvDesc(code, B, H, W, Cin, Cout, k, 1, x_pad, 1)
        wf, wd = packed_weights(weight, d, dtype, cache=weight.is_leaf)
        y, scale, shift, mean, rstd = _conv_bn(d, x_ptr, wf, gamma, beta, bn, training, M, dev, dtype, 'conv_bn_add_relu')
        keep_o, o_ptr, o_pad = to_halo(other.detach(), dtype, 0)
        short = None
        if w_d is None:
            if tuple(other.shape) != (B, Cout, H, W):
                raise RuntimeError(f'conv_bn_add_relu: the identity {tuple(other.shape)} does not match the block output {(B, Cout, H, W)}')
            r_args = (C.c_void_p(o_ptr), o_pad, C.c_void_p(0), C.c_void_p(0), C.c_void_p(0))
        else:
            Bo, Cd, Hs, Ws = other.shape
            if (Bo, Hs, Ws) != (B, H * stride_d, W * stride_d):
                raise RuntimeError(f'conv_bn_add_relu: the shortcut input {tuple(other.shape)} at stride {stride_d} does not match the block output '
                                   f'{(B, Cout, H, W)}')
            xs = None
            if stride_d == 2:                                   # the even pixels, dense: the shortcut is then a 1x1 stride-1 convolution
                xs = torch.empty((B, H, W, Cd), dtype=dtype, device=dev)
                _lib.call('fva_subsample2_fwd', code, C.c_void_p(o_ptr), o_pad, _p(xs), B, Hs, Ws, Cd, _stream())
                keep_o, o_ptr, o_pad = xs, xs.data_ptr(), 0
            dd = _lib.ConvDesc(code, B, H, W, Cd, Cout, 1, 1, o_pad, 1)
            wf_d, wd_d = packed_weights(w_d, dd, dtype, cache=w_d.is_leaf)
            y_d, scale_d, shift_d, mean_d, rstd_d = _conv_bn(dd, o_ptr, wf_d, gamma_d, beta_d, bn_d, training, M, dev, dtype, 'conv_bn_add_relu')
            short = (dd, wd_d, y_d, scale_d, shift_d, mean_d, rstd_d, tuple(w_d.shape), gamma_d, (Hs, Ws, Cd))
            r_args = (C.c_void_p(0), 0, _p(y_d), _p(scale_d), _p(shift_d))
        zbuf, z = halo_alloc(B, Cout, H, W, dtype, dev, 1)
        _lib.call('fva_bn_add_relu_apply', code, _p(y), _p(scale), _p(shift), *r_args, _p(zbuf), 1, B, H, W, Cout, _stream())
        need = grad_on and any(ctx.needs_input_grad)
        ctx.saved = (keep, x_ptr, y, scale, shift, mean, rstd, d, wd, dtype, tuple(weight.shape), gamma, keep_o, o_ptr, o_pad, short) if need else None
        ctx.training, ctx.stride_d = training, stride_d
        ctx.x_like, ctx.other_like, ctx.weight, ctx.w_d = x, other, weight, w_d
        ctx.link = link if need else None
        return z

    @staticmethod
    def backward(ctx, dz):
        if ctx.saved is None:
            raise _released('conv_bn_add_relu')
        if not ctx.training:
            raise RuntimeError(FROZEN_TAIL)
        keep, x_ptr, y, scale, shift, mean, rstd, d, wd, dtype, wshape, gamma, keep_o, o_ptr, o_pad, short = ctx.saved
        lib = _lib.load()
        B, H, W, Cout, dev, code = d.B, d.H, d.W, d.Cout, y.device, _code(dtype)
        M = B * H * W
        keep_dz, dz_ptr = to_dense(dz, dtype)
        if short is None:
            # dr = dU: the identity's gradient
            dy, other_grad, dgamma, dbeta = _bn_add_relu_bwd_identity(code, dz_ptr, y, scale, shift, mean, rstd, gamma, o_ptr, o_pad, B, H, W, Cout,
                                                                      dtype)
            dw_d = dgamma_d = dbeta_d = None
        else:
            dd, wd_d, y_d, scale_d, shift_d, mean_d, rstd_d, wshape_d, gamma_d, (Hs, Ws, Cd) = short
            f32 = dict(dtype=torch.float32, device=dev)
            nb = lib.fva_bn_add_relu_bwd_blocks(code, M, Cout)
            rows = lib.fva_bn_partial_rows(nb)
            part, part_d = torch.empty((rows, 2, Cout), **f32), torch.empty((rows, 2, Cout), **f32)
            dgamma, dbeta, coef = torch.empty(Cout, **f32), torch.empty(Cout, **f32), torch.empty((3, Cout), **f32)
            dy = torch.empty((B, H + 2, W + 2, Cout), dtype=dtype, device=dev)
            main = (code, C.c_void_p(dz_ptr), _p(y), _p(scale), _p(shift), _p(mean), _p(rstd))
            sc = (_p(y_d), _p(scale_d), _p(shift_d), _p(mean_d), _p(rstd_d))
            _lib.call('fva_bn_add_relu_bwd_reduce', *main, None, 0, *sc, _p(part), _p(part_d), nb, B, H, W, Cout, _stream())
            dgamma_d, dbeta_d, coef_d = torch.empty(Cout, **f32), torch.empty(Cout, **f32), torch.empty((3, Cout), **f32)
            _lib.call('fva_bn_bwd_finalize', _p(part), nb, rows, M, Cout, _p(gamma), _p(rstd), _p(dgamma), _p(dbeta), 0, _p(coef), _stream())
            _lib.call('fva_bn_bwd_finalize', _p(part_d), nb, rows, M, Cout, _p(gamma_d), _p(rstd_d), _p(dgamma_d), _p(dbeta_d), 0, _p(coef_d), _stream())
            dy_d = torch.empty_like(dy)
            _lib.call('fva_bn_add_relu_bwd_apply', *main, _p(coef), None, 0, *sc, _p(coef_d), _p(dy), _p(dy_d), 1, None, B, H, W, Cout, _stream())
            other_grad, dw_d = _wgrad_dgrad(dd, o_ptr, dy_d, wd_d, wshape_d, (keep_o,), ctx.w_d, ctx.needs_input_grad[4])
            if other_grad is not None and ctx.stride_d == 2:
                full = torch.empty((B, Hs, Ws, Cd), dtype=dtype, device=dev)
                _lib.call('fva_subsample2_bwd', code, _p(other_grad), _p(full), B, Hs, Ws, Cd, _stream())
                other_grad = full
        dxb, dw = _wgrad_dgrad(d, x_ptr, dy, wd, wshape, (keep,), ctx.weight, ctx.needs_input_grad[0])
        dx = _grad_like(dxb, ctx.x_like) if dxb is not None else None
        link, g_other = ctx.link, None
        if other_grad is not None and ctx.needs_input_grad[4]:
            if link is not None and link.open and not link.taken:
                link.addend, link.taken = other_grad, True       # the block's first dgrad adds it in its epilogue
            else:
                g_other = _grad_like(other_grad, ctx.other_like)
        ctx.saved = ctx.x_like = ctx.other_like = ctx.weight = ctx.w_d = ctx.link = None
        return dx, dw, dgamma, dbeta, g_other, dw_d, dgamma_d, dbeta_d, None, None, None, None, None, None, None, None


def conv_bn_add_relu(x, conv, bn, other, shortcut_conv=None, shortcut_bn=None, dtype=None):
    """The tail of a residual block.  ``conv_bn_add_relu(x, conv, bn, identity)`` = ``relu(bn(conv(x)) + identity)``;
    ``conv_bn_add_relu(x, conv, bn, shortcut_in, shortcut_conv, shortcut_bn)`` = ``relu(bn(conv(x)) + shortcut_bn(shortcut_conv(shortcut_in)))``.
    ``conv``: bias-free 1x1 or 3x3 of stride 1; ``shortcut_conv``: bias-free 1x1 of stride 1 or 2."""
    dtype = dtype or get_compute_dtype()
    k, _ = _conv_geometry(conv, 'conv_bn_add_relu', {(1, 1), (3, 1)})
    training = _check_bn(bn, 'conv_bn_add_relu')
    if (shortcut_conv is None) != (shortcut_bn is None):
        raise RuntimeError('conv_bn_add_relu: shortcut_conv and shortcut_bn come together')
    stride_d, w_d, g_d, b_d, bn_d = 1, None, None, None, None
    if shortcut_conv is not None:
        _, stride_d = _conv_geometry(shortcut_conv, 'conv_bn_add_relu (shortcut)', {(1, 1), (1, 2)})
        _even_map(other, stride_d, 'conv_bn_add_relu (shortcut)')
        if _check_bn(shortcut_bn, 'conv_bn_add_relu (shortcut)') != training:
            raise RuntimeError('conv_bn_add_relu: the two BatchNorm layers of a tail must be in the same mode')
        w_d, g_d, b_d, bn_d = shortcut_conv.weight, shortcut_bn.weight, shortcut_bn.bias, _BNState(shortcut_bn)
    grad_on = torch.is_grad_enabled()
    link = getattr(other, '_fva_block_in', None) if grad_on else None
    if link is not None and not (link.open and not link.taken and link.shape == tuple(other.shape) and link.dtype == dtype):
        link = None
    return ConvBNAddReLUFn.apply(x, conv.weight, bn.weight, bn.bias, other, w_d, g_d, b_d, _BNState(bn), bn_d, training, dtype, k, stride_d, link,
                                 grad_on)
