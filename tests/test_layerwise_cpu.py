"""FusedLARS / FusedLAMB without a GPU: constructor checks, the two groups of layerwise_groups, and the C entry points reporting bad
arguments instead of crashing."""
import ctypes as C

import pytest
import torch


@pytest.fixture(scope='module')
def built():
    import __graft_entry__ as ge
    ge.build()
    from fastvision_amd import _lib
    return _lib


def _params():
    return [torch.nn.Parameter(torch.zeros(3))]


@pytest.mark.parametrize('kw', [dict(lr=-1.0), dict(momentum=-0.5), dict(weight_decay=-1e-4), dict(nesterov=True), dict(trust_coefficient=-1e-3),
                                dict(eps=-1e-8), dict(clip_norm=0.0), dict(clip_norm=float('nan')), dict(foreach=True)])
def test_lars_refuses_bad_arguments(kw):
    from fastvision_amd import FusedLARS
    with pytest.raises(ValueError):
        FusedLARS(_params(), **kw)


@pytest.mark.parametrize('kw', [dict(lr=-1.0), dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)), dict(eps=-1e-8), dict(weight_decay=-1e-2),
                                dict(clip_norm=float('inf')), dict(clip_norm=-1.0)])
def test_lamb_refuses_bad_arguments(kw):
    from fastvision_amd import FusedLAMB
    with pytest.raises(ValueError):
        FusedLAMB(_params(), **kw)


def test_defaults_state_layout_and_cpu_parameters():
    from fastvision_amd import FusedAdam, FusedLAMB, FusedLARS
    lars, lamb = FusedLARS(_params(), lr=0.1, momentum=0.9), FusedLAMB(_params())
    assert lars.param_groups[0]['trust_coefficient'] == 0.001 and lars.param_groups[0]['eps'] == 1e-8
    assert lamb.param_groups[0]['trust'] is True
    assert lamb.state_dict()['state'] == FusedAdam(_params()).state_dict()['state'] == {}
    for opt in (lars, lamb):
        opt.param_groups[0]['params'][0].grad = torch.ones(3)
        with pytest.raises(RuntimeError, match='GPU'):
            opt.step()


def test_layerwise_groups_split_by_ndim():
    from fastvision_amd import FusedLAMB, FusedLARS, layerwise_groups
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.BatchNorm2d(4), torch.nn.Flatten(), torch.nn.Linear(4, 2, bias=False))
    net[3].weight.requires_grad_(False)
    groups = layerwise_groups(net, 5e-4)
    assert [[tuple(p.shape) for p in g['params']] for g in groups] == [[(4, 3, 3, 3)], [(4,), (4,), (4,)]]
    assert groups[0]['weight_decay'] == 5e-4 and 'trust' not in groups[0] and 'trust_coefficient' not in groups[0]
    assert groups[1]['weight_decay'] == 0.0 and groups[1]['trust'] is False and groups[1]['trust_coefficient'] == 0.0
    lars, lamb = FusedLARS(groups, lr=0.1), FusedLAMB(layerwise_groups(net, 5e-4))
    assert [g['trust_coefficient'] for g in lars.param_groups] == [0.001, 0.0]
    assert [g['trust'] for g in lamb.param_groups] == [True, False]


def test_entry_points_report_bad_arguments(built):
    lib = built.load()
    p = C.c_void_p(16)
    lars = [p, 1, p, 1, p, p, p, 0, 0.0, p, p, None, None]       # tab n chunks nchunks first hyper fresh clear clip partial ratio clip_out stream
    lamb = [p, 1, p, 1, p, p, 1, p, 0.0, p, p, None, None]       # tab n chunks nchunks first hyper groups state clip partial ratio clip_out stream
    for name, good, bad in (('fva_lars_step', lars, [(0, None), (1, 0), (2, None), (3, 0), (4, None), (5, None), (6, None), (9, None), (10, None),
                                                     (8, 10.0), (8, -1.0), (8, float('inf')), (8, float('nan'))]),
                            ('fva_lamb_step', lamb, [(0, None), (1, 0), (2, None), (3, 0), (4, None), (5, None), (6, 0), (7, None), (9, None),
                                                     (10, None), (8, 10.0), (8, -1.0), (8, float('inf')), (8, float('nan'))])):
        for i, v in bad:                                         # clip 10.0 is refused because clip_out is null
            args = list(good)
            args[i] = v
            assert getattr(lib, name)(*args) == -1 and name.encode() in lib.fva_last_error(), (name, i, v)
        with pytest.raises(RuntimeError, match=name):
            built.call(name, None, *good[1:])
