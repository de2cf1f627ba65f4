"""tests/ship_restatement.py pinned without a GPU.  With dt = float32 it reproduces the reference's own ship-demo ComputeLoss
(tests/golden/ship_loss.npz, written by tools/make_ship_golden.py) at the tolerances tests/test_gpu_model.py uses for CIOULoss against the
reference's vectors: values rtol 1e-5, gradients rtol 1e-3, atol 1e-6.  The cases tests/test_gpu_ship_loss.py uses hold no undecidable
decision, the measure accepts the honest fp32 evaluation and rejects three wrong box terms, and the decode restatement's fp32 instance
leaves at most MAX_EXCUSED of a case's rows on the min_wh drop."""
import os

import numpy as np
import pytest
import torch

import detect_restatement as dr
import loss_restatement as lr
import ship_restatement as sr

F64, F32 = torch.float64, torch.float32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ship_loss.npz')


@pytest.fixture(scope='module')
def gold():
    return np.load(GOLD)


def _fp32(layers, tg, anchors, wrong=''):
    leaves = [l.clone().requires_grad_(True) for l in layers]
    parts, und = sr.ship_terms(leaves, tg, anchors, F32, wrong=wrong)
    (parts[0] + parts[1] + parts[2]).backward()
    return torch.stack([p.detach() for p in parts]), [l.grad for l in leaves], und


@pytest.mark.parametrize('name', ['c65', 'c1', 'c80'])
def test_ship_restatement_fp32_is_the_reference(gold, name):
    layers, tg, anchors = lr.demo_case(name)
    vals, grads, und = _fp32(layers, tg, anchors)
    assert und == 0
    np.testing.assert_allclose(vals.numpy(), gold[f'{name}_values'], rtol=1e-5, atol=0)
    stored = [k for k in gold.files if k.startswith(f'{name}_grad')]
    assert len(stored) == (1 if name == 'c80' else len(layers))
    for l in range(len(stored)):
        want = gold[f'{name}_grad{l}']
        assert np.abs(want).max() > 0
        np.testing.assert_allclose(grads[l].numpy(), want, rtol=1e-3, atol=1e-6)
    print(f'{name}: values bit-identical to the reference: {np.array_equal(vals.numpy(), gold[f"{name}_values"])}')


def _worst(ref, vals, grads):
    return max(lr.worst(vals.double(), ref['vals64'], ref['val_limits']),
               max(lr.worst(g, r, l) for g, r, l in zip(grads, ref['grads64'], ref['grad_limits'])))


@pytest.mark.parametrize('name', list(lr.DEMO_CASES))
def test_honest_fp32_evaluation_is_accepted(name):
    layers, tg, anchors = lr.demo_case(name)
    ref = sr.ship_reference(layers, tg, anchors)
    assert ref['undecidable'] == 0
    assert (ref['val_limits'] > 0).all() and all((l >= 0).all() for l in ref['grad_limits'])
    w = _worst(ref, *_fp32(layers, tg, anchors)[:2])
    print(f'{name}: fp32 restatement against float64: worst err / limit {w:.3f}')
    assert w <= 1.0 / sr.sm.FACTOR + 1e-12             # e32 itself is a quarter of the limit at the most


@pytest.mark.parametrize('wrong', sr.WRONG)
def test_wrong_box_terms_are_rejected(wrong):
    layers, tg, anchors = lr.demo_case('c80')
    ref = sr.ship_reference(layers, tg, anchors)
    vals, grads, _ = _fp32(layers, tg, anchors, wrong)
    wv = lr.worst(vals.double(), ref['vals64'], ref['val_limits'])
    wg = max(lr.worst(g, r, l) for g, r, l in zip(grads, ref['grads64'], ref['grad_limits']))
    print(f'{wrong}: worst err / limit values {wv:.1f}, gradients {wg:.1f}')
    assert wg > 1.0
    if wrong != 'alpha_grad':                           # differentiating alpha changes the gradient only
        assert wv > 1.0


@pytest.mark.parametrize('name', list(dr.DECODE_CASES))
def test_decode2_restatement_and_its_excused_share(name):
    heads, anchors, strides, letterbox = dr.decode_case(name)
    # without a letterbox the centre is the library variant's and the rows are in the demo variant's order
    o2, m2, _ = sr.decode_rows2(heads, anchors, strides, None, F64)
    B, K = o2.shape[0], o2.shape[2]
    row0 = 0
    for h, anc, stride in zip(heads, anchors, strides):
        _, A, H, W, _ = h.shape
        lib, _, _ = dr.decode_rows([h], [anc], [stride], 0, None, F64)                      # (a, y, x) rows
        lib = lib.view(B, A, H, W, K).permute(0, 2, 3, 1, 4).reshape(B, -1, K)
        mine = o2[:, row0:row0 + A * H * W]
        # (torch's sigmoid is not the same function on every memory path: float64 roundings apart)
        assert torch.allclose(mine[..., 0:2], lib[..., 0:2], rtol=1e-14, atol=0) and torch.allclose(mine[..., 4:], lib[..., 4:], rtol=1e-14, atol=0)
        assert torch.allclose(mine[..., 2:4], lib[..., 2:4] * stride, rtol=1e-14, atol=0)
        row0 += A * H * W
    r64, _, e64 = sr.decode_rows2(heads, anchors, strides, letterbox, F64)
    r32, _, e32 = sr.decode_rows2(heads, anchors, strides, letterbox, F32)
    excused = dr.decode_excused(e64, e32, letterbox[5])
    dropped = r64[..., 4] == -1
    assert excused.double().mean() <= dr.MAX_EXCUSED
    assert dr.MIN_SHARE <= dropped.double().mean() <= 1 - dr.MIN_SHARE
    assert torch.equal((r32[..., 4] == -1)[~excused], dropped[~excused])
