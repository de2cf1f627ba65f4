"""resnext50_32x4d on the device under resnet_ops.set_grouped_path('mfma_s2'), with the machinery and the bars of tests/test_gpu_resnext.py
and tests/test_gpu_resnext_mfma.py (imported; both unchanged): the bf16 train step against the float64 restatement and three captured steps
bit-identical with three eager ones.  At 2 x 3 x 64 x 64 the stride-2 grouped layers run at 16^2, 8^2 and 4^2 with Cg = 8, 16, 32; both
tests assert that all 16 grouped layers were launched on their matrix-unit entries and none on the plain ones."""
import collections
import contextlib

import pytest
import torch

import test_gpu_resnet as T
import test_gpu_resnext as X
from test_gpu_resnext_mfma import NAME

pytestmark = pytest.mark.gpu

DEV = T.DEV


@contextlib.contextmanager
def s2_path():
    """'mfma_s2' for the body, the previous path afterwards; yields a counter of the entry points launched meanwhile."""
    import __graft_entry__ as ge
    ge.build()
    from fastvision_amd import _lib, resnet_ops as ro
    counts = collections.Counter()
    real = _lib.call

    def counting(name, *args):
        counts[name] += 1
        return real(name, *args)
    prev = ro.set_grouped_path('mfma_s2')
    _lib.call = counting
    try:
        yield counts
    finally:
        _lib.call = real
        ro.set_grouped_path(prev)


def _assert_routed(counts, steps=1):
    """13 stride-1 and 3 stride-2 grouped layers, each on its own matrix-unit entries"""
    for pre, layers in (('fva_gconv_mfma_', 13), ('fva_gconv_mfma_s2_', 3)):
        assert {counts[pre + k] for k in ('pack', 'fwd', 'wgrad', 'dgrad')} == {layers * steps}, counts
    assert counts['fva_gconv_fwd'] == counts['fva_gconv_wgrad'] == counts['fva_gconv_dgrad'] == 0, counts


def test_train_step_bf16_resnext50():
    """X.test_train_step_bf16_resnext50 under 'mfma_s2': the same seed and the bars of its 'mfma' twin (logits within 1.3e-1 of their scale,
    gradient norms within 1.2e-1, sampled cosines above X.BF16_COSINE's bar)."""
    with s2_path() as counts:
        ref, r64, net, rl, rloss, gl, gloss, images, labels, _ = X._both_steps(NAME, X.BF, X.SEED_BF16, adopt=False)
    _assert_routed(counts)
    rp, gp = dict(r64.named_parameters()), dict(net.named_parameters())
    herr = T.rel_err(gl, rl)
    rel = {}
    for k, p in rp.items():
        a, b = gp[k].grad.double().cpu(), p.grad.double()
        assert torch.isfinite(a).all(), k
        rel[k] = abs(a.norm().item() - b.norm().item()) / max(b.norm().item(), 1e-300)
    cos = {k: T._cosine(gp[k].grad, rp[k].grad) for k in X._grad_names()}
    wk = max(rel, key=rel.get)
    print(f'\n  {NAME} bf16 64 mfma_s2: logits {herr:.2e} of scale, loss {gloss:.5f} vs {rloss:.5f}, gradient norms max {rel[wk]:.2e} ({wk}); '
          f'lowest cosine {min(cos.values()):.4f}')
    assert herr < 1.3e-1
    assert rel[wk] < 1.2e-1, wk
    for k in cos:
        assert cos[k] > X.BF16_COSINE[k][1], (k, cos[k])


def test_graphed_step_is_bit_identical_with_eager():
    """Three captured steps against three eager ones; both pack launches are part of the captured forward."""
    from fastvision_amd import ops
    from fastvision_amd.graphs import GraphedTrainStep
    gen = torch.Generator().manual_seed(5)
    batches = [(torch.randn(4, 3, 64, 64, generator=gen), torch.randint(0, 10, (4, 1), generator=gen).float()) for _ in range(3)]
    with s2_path() as counts:
        prev = ops.set_wgrad_side_stream(False)
        try:
            net, crit, opt = T._train_parts(NAME)
            want = [T._step(net, crit, opt, im.to(DEV), lab.to(DEV)) for im, lab in batches]
            torch.cuda.synchronize()
        finally:
            ops.set_wgrad_side_stream(prev)
        _assert_routed(counts, steps=3)
        net2, crit2, opt2 = T._train_parts(NAME)
        step = GraphedTrainStep(net2, lambda p, t: crit2(p, t), opt2, batches[0][0].to(DEV), batches[0][1].to(DEV))
        got = [step(im.to(DEV), lab.to(DEV)).clone() for im, lab in batches]
        torch.cuda.synchronize()
    assert counts['fva_gconv_mfma_s2_pack'] > 3 * 3                 # the capture launched them too
    assert len({w.item() for w in want}) == 3
    for a, b in zip(got, want):
        assert torch.equal(a, b), (a, b)
    for (k, p), q in zip(net.state_dict().items(), net2.state_dict().values()):
        assert torch.equal(p, q), k
