"""RandAugment and RandomErasing on the GPU (fva_randaug_plan / _plan_fixed / _stats / _apply, fva_random_erase) against the integer /
float64 statements of tests/randaug_restatement.py, by the rule stated there: bit-exact, except a difference of 1 where the float64 value
before truncation lies within 2^-10 of an integer, and pixels left out where a source coordinate lies within 2^-10 of a half-integer; the
share of both is capped at 1 % per case.  Canvases: 3 x 37 x 53 (tile seams and byte tails inside the image; noise, a constant and a
two-level channel, a narrow ramp), 9 x 9 (smaller than a tile), 70 x 300 (full tiles: with the fourth value of the geometric ops the source
window of a tile exceeds the LDS window and is gathered) and 34 x 96 (W % 16 == 0: the 16-byte path)."""
import numpy as np
import pytest
import torch

import randaug_restatement as rr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FILL = (7, 8, 9)
SHAPES = [(3, 37, 53), (1, 9, 9), (1, 70, 300), (2, 34, 96)]
# negative, positive, bin 0 (where the op has a value); the geometric ops: a fourth beyond the standard space, for the gather path.
# 0.29 not 0.3, 29 not 30 degrees: with the canvases' integer centres those put whole rows on half-integer source coordinates.
BLEND = [-0.6317, 0.8731, 0.0]
CASES = {'Identity': [0.0], 'ShearX': [-0.21, 0.29, 0.0, 3.73], 'ShearY': [-0.21, 0.29, 0.0, -2.21], 'TranslateX': [-7, 11, 0],
         'TranslateY': [-5, 16, 0], 'Rotate': [-17.0, 29.0, 0.0, 43.0], 'Brightness': BLEND, 'Color': BLEND, 'Contrast': BLEND, 'Sharpness': BLEND,
         'Posterize': [4, 6, 8], 'Solarize': [76.5, 178.5, 255.0], 'AutoContrast': [0.0], 'Equalize': [0.0]}


@pytest.fixture(scope='module')
def images():
    return [rr.canvases(B, H, W, 100 + i) for i, (B, H, W) in enumerate(SHAPES)]


def _run(aug, batch, ops, values):
    out = aug.apply_plan(torch.from_numpy(batch).to(DEV), ops, values)
    return out.cpu().numpy()


@pytest.mark.parametrize('op,v', [(op, v) for op, vals in CASES.items() for v in vals])
def test_each_op_against_the_restatement(images, op, v):
    from fastvision_amd import RandAugment
    aug = RandAugment(num_ops=1, fill=FILL)
    v = float(np.float32(v))
    marked = total = 0
    for batch in images:
        B = batch.shape[0]
        got = _run(aug, batch, [[op]] * B, [[v]] * B)
        want, excused, skipped = rr.apply_plan(batch, [[op]] * B, [[v]] * B, FILL)
        ok, _ = rr.compare(got, want, excused, skipped)
        assert ok, (op, v, batch.shape)
        marked, total = marked + int((excused | skipped).sum()), total + want.size
        if op in ('Posterize', 'Solarize', 'Equalize', 'TranslateX', 'TranslateY', 'Identity', 'AutoContrast') or v == 0:
            assert not (excused | skipped).any()                     # the bit-exact ops take no excuse at all
    assert marked <= 0.01 * total


def test_rounds_compose_and_a_second_call_starts_from_clean_histograms(images):
    """Rotate -> Equalize -> Sharpness: Equalize must see the histogram of the ROTATED image, and the second call (an odd number of rounds,
    so the two histogram sets swap roles) must not see what the first left"""
    from fastvision_amd import RandAugment
    batch = images[0]
    ops, vals = [['Rotate', 'Equalize', 'Sharpness']] * 3, [[23.0, 0.0, 0.8731]] * 3
    want, excused, skipped = rr.apply_plan(batch, ops, vals, FILL)
    aug = RandAugment(num_ops=3, fill=FILL)
    for call in range(3):
        ok, share = rr.compare(_run(aug, batch, ops, vals), want, excused, skipped)
        assert ok and share <= 0.01, (call, share)
    ops2, vals2 = [['Contrast', 'AutoContrast', 'Equalize']] * 3, [[0.0, 0.0, 0.0]] * 3          # statistics in every round
    want2, e2, s2 = rr.apply_plan(batch, ops2, vals2, FILL)
    assert rr.compare(_run(aug, batch, ops2, vals2), want2, e2, s2)[0]


def test_random_plan_distribution_and_reproducibility():
    from fastvision_amd import RandAugment
    B, N = 4096, 2
    x = torch.zeros(B, 4, 4, 3, dtype=torch.uint8, device=DEV)

    def draw(calls=1, **kw):
        aug = RandAugment(num_ops=N, seed=11, **kw).to(DEV)
        plans = []
        for _ in range(calls):
            aug(x)
            plans.append(aug.plan_arrays())
        assert aug._state.cpu().tolist() == [11, calls, 0, 0]
        return plans
    (ops, vals), (ops_b, vals_b) = draw(2)
    assert ops.min() >= 0 and ops.max() < 14
    n, q = B * N, 1 / 14
    counts = np.bincount(ops.ravel(), minlength=14)
    assert (np.abs(counts - n * q) <= 5 * np.sqrt(n * q * (1 - q))).all(), counts
    signed = np.isin(ops, [rr.OPS.index(o) for o in rr.SIGNED]) & (vals != 0)
    assert 0.45 <= (vals[signed] < 0).mean() <= 0.55
    shear = np.abs(vals[ops == rr.OPS.index('ShearX')])
    assert np.allclose(shear, np.float32(0.3 * 9 / 30), rtol=1e-6, atol=0) and (vals[ops == rr.OPS.index('Posterize')] == 7).all()   # bin 9 of 31
    (ops_c, vals_c), = draw(1)
    assert (ops_c == ops).all() and (vals_c == vals).all()                          # the same seed: the same plan
    assert (ops_b != ops).any()                                                      # the second call: another
    (ops_d, _), = draw(1, ops=['Rotate', 'Equalize', 'Identity'])
    assert set(np.unique(ops_d)) == {rr.OPS.index(o) for o in ('Rotate', 'Equalize', 'Identity')}


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('inplace,W', [(False, 56), (False, 52), (True, 52)], ids=['out-chunks', 'out-elements', 'inplace'])
def test_random_erasing_boxes_fill_and_the_rest_untouched(dtype, inplace, W):
    """W = 52 is no multiple of the bf16 chunk: out of place, bf16 takes the one-element path there and 16-byte chunks at 56"""
    from fastvision_amd import RandomErasing
    B, C, H = 64, 3, 40
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(B, C, H, W, generator=gen).to(dtype).to(DEV)
    keep = x.clone()
    view = lambda t: t.view(torch.int32 if dtype == torch.float32 else torch.int16).cpu()
    era = RandomErasing(p=1.0, value=-2.5, inplace=inplace, seed=3).to(DEV)
    out = era(x)
    assert (out is x) == inplace and (inplace or torch.equal(view(x), view(keep)))
    boxes = era.boxes.cpu().numpy()
    inside = np.zeros((B, 1, H, W), bool)
    for b, (top, left, h, w) in enumerate(boxes):
        inside[b, 0, top:top + h, left:left + w] = True
        assert 0 <= top and top + h <= H and 0 <= left and left + w <= W and h < H and w < W
        if h * w == 0:                                               # ten attempts and none fitted: nothing erased
            continue
        # sides are rounded to integers: half a pixel of slack on each
        assert (h + 0.5) * (w + 0.5) >= 0.02 * H * W and (max(h - 0.5, 0)) * max(w - 0.5, 0) <= 0.33 * H * W, (h, w)
        assert max(h - 0.5, 0) / (w + 0.5) <= 3.3 and (h + 0.5) / max(w - 0.5, 1e-9) >= 0.3, (h, w)
    assert (boxes[:, 2] * boxes[:, 3] > 0).mean() > 0.9                               # ten attempts: nearly every image finds a box
    inside = torch.from_numpy(np.broadcast_to(inside, (B, C, H, W)).copy())
    got = out.cpu()
    assert (got[inside].float() == -2.5).all() and torch.equal(view(out)[~inside], view(keep)[~inside])
    # p = 0: the bits stay
    before = view(out)
    same = RandomErasing(p=0.0, inplace=inplace, seed=3).to(DEV)(out)
    assert torch.equal(view(same), before) and era._state.cpu().tolist() == [3, 1, 0, 0]
    # noise: N(0, 1) over the erased elements, 5 sigma on mean and variance (variance of the sample variance of a normal: 2 / n)
    noisy = RandomErasing(p=1.0, value='random', inplace=False, seed=4).to(DEV)
    big = torch.zeros(256, C, H, W, dtype=dtype, device=DEV)
    z = noisy(big).float().cpu()
    nb = noisy.boxes.cpu().numpy()
    n = int((nb[:, 2] * nb[:, 3]).sum()) * C
    vals = z[z != 0]
    assert n >= 10 ** 5 and abs(vals.numel() - n) <= 0.01 * n                         # bf16 may round a tiny draw to 0: far below 1 %
    assert abs(vals.mean().item()) <= 5 / np.sqrt(n) and abs(vals.var().item() - 1) <= 5 * np.sqrt(2 / n)
    assert not torch.equal(noisy(big).float().cpu(), z)                               # the next call: other boxes, other noise


def test_chain_is_capturable_draws_per_replay_and_launches_only_the_library(monkeypatch):
    from fastvision_amd import BatchMix, RandAugment, RandomErasing, _lib, normalise
    B, H, W = 8, 32, 48
    canv = torch.from_numpy(rr.canvases(B, H, W, 7)).to(DEV)
    labels = torch.arange(B, device=DEV)
    aug, era, mix = RandAugment(seed=1).to(DEV), RandomErasing(p=1.0, seed=2).to(DEV), BatchMix(seed=3).to(DEV)
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)

    def chain():
        return mix(era(normalise(aug(canv), mean, std)), labels)[0]
    eager = chain()                                                                  # warm-up: tables, buffers
    seen = []
    monkeypatch.setattr(_lib, 'tracer', lambda name, args: seen.append(name))
    torch.cuda.set_sync_debug_mode('error')
    try:
        chain()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    monkeypatch.undo()
    assert seen == ['fva_randaug_plan'] + ['fva_randaug_stats', 'fva_randaug_apply'] * 2 + ['fva_colour_blur_shuffle_normalize', 'fva_random_erase',
                                                                                          'fva_mix_plan', 'fva_mix_apply']
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        augmented = aug(canv)
        captured = mix(era(normalise(augmented, mean, std)), labels)[0]
    plans, canvs, outs = [], [], []
    for _ in range(3):
        graph.replay()
        plans.append(aug.plan.clone()), canvs.append(augmented.clone()), outs.append(captured.clone())
    torch.cuda.synchronize()
    assert aug._state.cpu().tolist() == [1, 5, 0, 0]                                 # two eager calls, then one tick per replay (the capture runs nothing)
    assert not torch.equal(plans[0], plans[1]) and not torch.equal(plans[1], plans[2]) and not torch.equal(outs[0], outs[1])
    assert torch.isfinite(outs[2]).all() and eager.shape == (B, 3, H, W)
    for plan, got in zip(plans, canvs):                                              # every replay computed what the eager launches compute for its plan
        assert torch.equal(aug.apply_plan(canv, plan[..., 0], plan[..., 1].contiguous().view(torch.float32)), got)
