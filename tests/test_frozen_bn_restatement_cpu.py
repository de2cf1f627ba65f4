"""Pins tests/frozen_bn_restatement.py (the reference of the frozen-BatchNorm GPU tests) against float64 torch autograd of
F.batch_norm(training=False) + F.silu / F.relu, with and without a convolution bias, with gamma = 0 and gamma < 0 channels; and, still without a
GPU: the new entry points are declared, bound and exported, refuse bad arguments before any launch, and utils.freeze_batchnorm keeps
the BatchNorm modules in eval mode without changing what the module IS (state_dict keys and tensors, pickling, deep copies)."""
import copy
import ctypes as C
import os
import pickle
import re

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import frozen_bn_restatement as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('fva_bn_frozen_bwd_blocks', 'fva_bn_silu_frozen_bwd', 'fva_bn_relu_frozen_bwd', 'fva_bn_frozen_bwd_finalize', 'fva_bn_frozen_stats')


@pytest.fixture(scope='module')
def built():
    import __graft_entry__ as ge
    ge.build()
    from fastvision_amd import _lib
    return _lib


@pytest.mark.parametrize('act', ['silu', 'relu'])
@pytest.mark.parametrize('with_bias', [False, True])
def test_restatement_equals_float64_autograd(act, with_bias):
    g = torch.Generator().manual_seed(11 + with_bias)
    B, H, W, Cc = 3, 5, 4, 8
    dd = torch.float64
    y = (torch.randn(B, Cc, H, W, generator=g, dtype=dd) * 1.5).requires_grad_()
    gamma = torch.tensor([1.2, -0.7, 0.0, 0.9, -1.4, 0.6, 1.1, 0.8], dtype=dd).requires_grad_()     # a zero and two negative channels
    beta = (0.5 * torch.randn(Cc, generator=g, dtype=dd)).requires_grad_()
    bias = (torch.randn(Cc, generator=g, dtype=dd)).requires_grad_() if with_bias else None
    rm, rv, eps = 0.3 * torch.randn(Cc, generator=g, dtype=dd), 0.5 + 1.5 * torch.rand(Cc, generator=g, dtype=dd), 1e-5
    dz = torch.randn(B, Cc, H, W, generator=g, dtype=dd)
    rm0, rv0 = rm.clone(), rv.clone()
    pre = y + bias[None, :, None, None] if with_bias else y
    z = (F.silu if act == 'silu' else F.relu)(F.batch_norm(pre, rm, rv, gamma, beta, training=False, eps=eps))
    z.backward(dz)
    assert torch.equal(rm, rm0) and torch.equal(rv, rv0)

    with torch.no_grad():
        scale, shift, m, r = fr.eval_coeffs(gamma, beta, rm, rv, eps, bias)
        nhwc = lambda t: t.permute(0, 2, 3, 1)
        u, du, t2, dY = fr.terms(nhwc(dz), nhwc(y), scale, shift, m, r, act, dd)
        dgamma, dbeta, dbias = fr.param_grads(du, t2, scale)
    close = lambda a, b: torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-14)
    close(dY, nhwc(y.grad))
    close(dgamma, gamma.grad)
    close(dbeta, beta.grad)
    if with_bias:
        close(dbias, bias.grad)
        assert bias.grad.abs().max() > 1e-3          # a real gradient, not the zeros of training mode
    assert dY[..., 2].abs().max() == 0               # gamma = 0: nothing flows back, dbeta still does
    assert dbeta[2].abs() > 0


def test_kink_mask_and_chain_length():
    y = torch.tensor([1.0, 1.0, 2.0])
    scale, shift = torch.tensor([1.0, 1.0, 0.0]), torch.tensor([-1.0, -1.0 + 2.0 ** -20, 0.5])
    assert fr.kink_mask(y, scale, shift).tolist() == [True, False, False]
    # 2 x (5 + 2) padded rows in one block, (7 + 2) * 4 = 36 chunks per row: 14 rows x 1 step + 64 lanes per channel chunk
    assert fr.chain_length(1, 2, 5, 7, 32, 1, 8) == 14 + 64
    # cpp = 128: 7 * 128 = 896 chunks -> 4 steps per row, 2 lanes per channel chunk
    assert fr.chain_length(1, 2, 3, 5, 1024, 1, 8) == 10 * 4 + 2
    assert fr.finalize_chain(1) == 2 and fr.finalize_chain(2048) == 17


def test_new_symbols_are_declared_bound_and_exported(built):
    hdr = open(os.path.join(ROOT, 'include', 'fastvision_amd.h')).read()
    declared = set(re.findall(r'\b(fva_[a-z0-9_]+)\s*\(', hdr))
    lib = built.load()
    for name in NEW:
        assert name in declared and name in built.PROTOTYPES and hasattr(lib, name), name
    assert lib.fva_version() >= 7


def test_argument_errors_are_reported_before_any_launch(built):
    lib = built.load()
    p = C.c_void_p(16)
    for name in ('fva_bn_silu_frozen_bwd', 'fva_bn_relu_frozen_bwd'):
        fn = getattr(lib, name)
        # C not a multiple of the 16-byte chunk (bf16: 8 channels, fp32: 4)
        assert fn(built.BF16, p, p, p, p, p, p, p, p, 1, 2, 4, 4, 36, None) == -1 and b'multiple of 8' in lib.fva_last_error()
        assert fn(built.F32, p, p, p, p, p, p, p, p, 1, 2, 4, 4, 6, None) == -1 and b'multiple of 4' in lib.fva_last_error()
        # a chunk count that does not divide the block of 256
        assert fn(built.BF16, p, p, p, p, p, p, p, p, 1, 2, 4, 4, 24, None) == -1 and b'power of two' in lib.fva_last_error()
        assert fn(built.F32, p, p, p, p, p, p, p, p, 1, 2, 4, 4, 2048, None) == -1 and b'power of two' in lib.fva_last_error()
        for pad in (-1, 2):
            assert fn(built.BF16, p, p, p, p, p, p, p, p, pad, 2, 4, 4, 64, None) == -1 and b'pad' in lib.fva_last_error()
        for hole in (1, 2, 3, 4, 8):                 # dz, y, scale, shift, dy
            args = [built.BF16, p, p, p, p, p, p, p, p, 1, 2, 4, 4, 64, None]
            args[hole] = None
            assert fn(*args) == -1 and b'null pointer' in lib.fva_last_error(), hole
        for hole in (5, 6):                          # a partial table needs m and r
            args = [built.BF16, p, p, p, p, p, p, p, p, 1, 2, 4, 4, 64, None]
            args[hole] = None
            assert fn(*args) == -1 and b'null pointer' in lib.fva_last_error(), hole
        assert fn(7, p, p, p, p, p, p, p, p, 1, 2, 4, 4, 64, None) == -1 and b'dtype' in lib.fva_last_error()
    assert lib.fva_bn_frozen_bwd_blocks(built.BF16, 2, 4, 4, 24, 1) == 0
    assert lib.fva_bn_frozen_bwd_blocks(built.BF16, 2, 4, 4, 64, 2) == 0
    assert lib.fva_bn_frozen_bwd_finalize(None, 1, 1, 8, p, p, p, p, None) == -1
    assert lib.fva_bn_frozen_bwd_finalize(p, 4, 3, 8, p, p, p, None, None) == -3 and b'rows' in lib.fva_last_error()     # FVA_ERR_WORKSPACE, as fva_bn_bwd_finalize
    assert lib.fva_bn_frozen_bwd_finalize(p, 4, 4, 8, None, None, None, p, None) == -1          # dbias needs scale
    assert lib.fva_bn_frozen_stats(8, None, p, None, 1e-5, p, p, None) == -1


def test_grid_is_capped_by_rows_blocks_and_pixels(built):
    """One block per padded row, at most 1024, and at most one per 64 pixels: the partial table (16 C bytes per block, written and read)
    stays under 5 % of the pass's own 6 M C bytes at every shape."""
    lib = built.load()
    assert lib.fva_bn_frozen_bwd_blocks(built.BF16, 2, 5, 7, 32, 1) == 1            # 70 pixels
    assert lib.fva_bn_frozen_bwd_blocks(built.BF16, 2, 24, 40, 64, 1) == 30         # 1920 pixels / 64 < 52 rows
    assert lib.fva_bn_frozen_bwd_blocks(built.F32, 2, 24, 40, 64, 0) == 30
    assert lib.fva_bn_frozen_bwd_blocks(built.BF16, 2, 30, 100, 64, 1) == 64        # 64 rows < 6000 / 64
    assert lib.fva_bn_frozen_bwd_blocks(built.BF16, 32, 320, 320, 64, 1) == 1024
    assert lib.fva_bn_frozen_bwd_blocks(built.BF16, 2, 520, 64, 8, 1) == 1024 and lib.fva_bn_frozen_bwd_blocks(built.F32, 2, 520, 64, 8, 0) == 1024
    for B, H, W, Cc in ((32, 20, 20, 1024), (32, 40, 40, 512), (32, 80, 80, 256), (32, 640, 640, 32), (64, 14, 14, 512), (64, 224, 224, 64)):
        nb = lib.fva_bn_frozen_bwd_blocks(built.BF16, B, H, W, Cc, 1)
        assert 0 < 2 * nb * 2 * Cc * 4 <= 0.05 * B * H * W * Cc * 6, (B, H, W, Cc, nb)


class _Net(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(3, 4, 3)
        self.bn = nn.BatchNorm2d(4)
        self.body = nn.Sequential(nn.Conv2d(4, 4, 1), nn.BatchNorm2d(4), nn.BatchNorm1d(4))


def test_freeze_batchnorm_helper():
    import fastvision
    from fastvision_amd import utils
    assert fastvision.utils.freeze_batchnorm is utils.freeze_batchnorm and fastvision.utils.unfreeze_batchnorm is utils.unfreeze_batchnorm
    net = _Net().train()
    keys, tensors = list(net.state_dict().keys()), [id(t) for t in net.state_dict(keep_vars=True).values()]
    params = [id(p) for p in net.parameters()]
    assert utils.freeze_batchnorm(net.body) is net.body
    net.train()
    assert net.training and net.bn.training and net.body.training and net.body[0].training
    assert not net.body[1].training                                   # survives .train()
    assert net.body[2].training                                       # a BatchNorm1d is none of its business
    assert isinstance(net.body[1], nn.BatchNorm2d)
    utils.freeze_batchnorm(net)
    net.eval(); net.train()
    assert not net.bn.training and not net.body[1].training and net.conv.training
    assert list(net.state_dict().keys()) == keys
    assert [id(t) for t in net.state_dict(keep_vars=True).values()] == tensors and [id(p) for p in net.parameters()] == params
    # frozen statistics in a forward pass: running statistics and the batch counter do not move
    rm, nbt = net.bn.running_mean.clone(), net.bn.num_batches_tracked.clone()
    net.bn(torch.randn(2, 4, 3, 3))
    assert torch.equal(net.bn.running_mean, rm) and torch.equal(net.bn.num_batches_tracked, nbt)
    for twin in (copy.deepcopy(net), pickle.loads(pickle.dumps(net))):
        twin.train()
        assert not twin.bn.training and not twin.body[1].training and type(twin.bn) is type(net.bn)
        assert list(twin.state_dict().keys()) == keys
    utils.unfreeze_batchnorm(net)
    assert type(net.bn) is nn.BatchNorm2d and type(net.body[1]) is nn.BatchNorm2d
    assert net.bn.training and net.body[1].training                   # the mode of the modules that hold them
    net.eval()
    assert not net.bn.training
    utils.freeze_batchnorm(net)
    utils.unfreeze_batchnorm(net)
    assert not net.bn.training and not net.body[1].training           # ... which is eval now
    net.train()
    assert net.bn.training and net.body[1].training
