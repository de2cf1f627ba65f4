"""resnet_ops.set_grouped_path / get_grouped_path and the routing of conv_bn_ops.GroupedConv, on CPU tensors with the recorder of
tests/test_conv_bn_node_cpu.py (its helpers are imported, the file is not touched): under 'mfma' the bf16 stride-1 layer records the pack
launch and the fva_gconv_mfma_* entries with the descriptor's fields, every layer the matrix-unit kernels do not serve (stride 2, fp32,
frozen fp32, the wide fp32 one) records exactly its golden sequence, and the default is 'plain'."""
import ctypes as C
import copy
import json

import pytest

import test_conv_bn_node_cpu as node
from test_conv_bn_node_cpu import built, golden            # noqa: F401  (fixtures)


@pytest.fixture
def ro(built):                                             # noqa: F811
    from fastvision_amd import resnet_ops
    assert resnet_ops.get_grouped_path() == 'plain'         # the default, and what every other test of the suite runs under
    yield resnet_ops
    resnet_ops.set_grouped_path('plain')


def _record(monkeypatch, case):
    return json.loads(json.dumps(node._record(monkeypatch, node._grouped, case)))


def test_the_switch(ro):
    assert ro.get_grouped_path() == 'plain'
    assert ro.set_grouped_path('mfma') == 'plain' and ro.get_grouped_path() == 'mfma'
    assert ro.set_grouped_path('mfma') == 'mfma'
    assert ro.set_grouped_path('plain') == 'mfma' and ro.get_grouped_path() == 'plain'
    for bad in ('MFMA', 'auto', '', None, 1):
        with pytest.raises(ValueError, match="grouped path must be 'plain' or 'mfma'"):
            ro.set_grouped_path(bad)
        assert ro.get_grouped_path() == 'plain'
    assert {'set_grouped_path', 'get_grouped_path'} <= set(ro.__all__)


def test_the_default_records_the_golden_sequences(ro, golden, monkeypatch):             # noqa: F811
    assert ro.get_grouped_path() == 'plain'
    for case in ('s1_bf16_train', 's2_train', 'frozen', 'wide_train'):
        assert _record(monkeypatch, case) == golden[f'grouped/{case}'], case


def test_mfma_routes_the_bf16_stride_1_layer(ro, built, golden, monkeypatch):           # noqa: F811
    ro.set_grouped_path('mfma')
    got = _record(monkeypatch, 's1_bf16_train')['calls']
    lib = built.load()
    d = built.GConvDesc(1, 2, 8, 8, 128, 32, 1, 1, 1)
    assert lib.fva_gconv_mfma_serves(C.byref(d)) == 1
    desc = {'type': 'GConvDesc', 'dtype': 1, 'B': 2, 'H': 8, 'W': 8, 'C': 128, 'groups': 32, 'stride': 1, 'in_pad': 1, 'dy_pad': 1}
    # what the plain path records, entry for entry: the pack in front of the forward, the new names, the new workspace size
    want = []
    rename = {'fva_gconv_fwd': 'fva_gconv_mfma_fwd', 'fva_gconv_wgrad': 'fva_gconv_mfma_wgrad', 'fva_gconv_dgrad': 'fva_gconv_mfma_dgrad'}
    for call in copy.deepcopy(golden['grouped/s1_bf16_train']['calls']):
        if call[0] == 'fva_gconv_fwd':
            want.append(['fva_gconv_mfma_pack', desc, 'ptr', 'ptr', 'ptr', 'null'])
        if call[0] == 'fva_gconv_wgrad':
            call[6] = lib.fva_gconv_mfma_wgrad_workspace(C.byref(d))
        if call[0] == 'fva_bn_finalize':
            nblk = lib.fva_gconv_mfma_stat_blocks(C.byref(d))
            call[2], call[3] = nblk, lib.fva_bn_partial_rows(nblk)
        call[0] = rename.get(call[0], call[0])
        want.append(call)
    names = [c[0] for c in got]
    assert names == [c[0] for c in want]
    assert got == want
    assert names.index('fva_gconv_mfma_pack') + 1 == names.index('fva_gconv_mfma_fwd')
    assert names.index('fva_gconv_mfma_wgrad') < names.index('fva_gconv_mfma_dgrad')
    assert all(c[1] == desc for c in got if c[0].startswith('fva_gconv_mfma'))
    assert not any(c[0] in rename for c in got)


@pytest.mark.parametrize('case', ['s2_train', 'frozen', 'wide_train'])
def test_mfma_leaves_the_layers_it_does_not_serve(ro, golden, monkeypatch, case):       # noqa: F811
    ro.set_grouped_path('mfma')
    assert _record(monkeypatch, case) == golden[f'grouped/{case}']


def test_mfma_packs_in_front_of_every_forward(ro, built, monkeypatch):                  # noqa: F811
    """Nothing is cached or keyed on the parameter: two forwards of one layer, two pack launches."""
    import torch
    import torch.nn as nn
    ro.set_grouped_path('mfma')
    trace = []
    node._patch(monkeypatch, trace)
    conv, bn = node._conv(128, 128, 3, 1, groups=32), nn.BatchNorm2d(128)
    for _ in range(2):
        node._bwd(ro.conv_bn_relu(node._x(2, 128, 8, 8), conv, bn, torch.bfloat16))
    names = [c[0] for c in trace]
    assert names.count('fva_gconv_mfma_pack') == names.count('fva_gconv_mfma_fwd') == 2
