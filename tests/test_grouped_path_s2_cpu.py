"""resnet_ops.set_grouped_path('mfma_s2') and the third route of conv_bn_ops.GroupedConv, on CPU tensors with the recorder of
tests/test_conv_bn_node_cpu.py as tests/test_grouped_path_cpu.py uses it.  The golden ``s2_train`` case runs in fp32, which no matrix-unit
kernel serves, so under 'mfma_s2' it records its golden sequence like ``frozen`` and ``wide_train``; the route itself is checked on the same
layer in bf16 against what 'plain' records for it, entry for entry."""
import ctypes as C
import copy

import pytest
import torch
import torch.nn as nn

import test_conv_bn_node_cpu as node
from test_conv_bn_node_cpu import built, golden            # noqa: F401  (fixtures)
from test_grouped_path_cpu import _record, ro              # noqa: F401  (ro: fixture)


def _s2_bf16(case):
    from fastvision_amd import resnet_ops
    node._bwd(resnet_ops.conv_bn_relu(node._x(2, 128, 8, 8), node._conv(128, 128, 3, 2, groups=32), nn.BatchNorm2d(128), torch.bfloat16))


def test_the_switch_has_three_values(ro):
    assert ro.set_grouped_path('mfma_s2') == 'plain' and ro.get_grouped_path() == 'mfma_s2'
    assert ro.set_grouped_path('mfma') == 'mfma_s2' and ro.set_grouped_path('plain') == 'mfma'
    with pytest.raises(ValueError, match="grouped path must be 'plain' or 'mfma'"):
        ro.set_grouped_path('mfma_s1')
    assert ro.get_grouped_path() == 'plain'


def test_mfma_s2_routes_the_bf16_stride_2_layer(ro, built, monkeypatch):                 # noqa: F811
    plain = node._record(monkeypatch, _s2_bf16, None)['calls']
    ro.set_grouped_path('mfma')
    assert node._record(monkeypatch, _s2_bf16, None)['calls'] == plain
    ro.set_grouped_path('mfma_s2')
    got = node._record(monkeypatch, _s2_bf16, None)['calls']
    lib = built.load()
    d = built.GConvDesc(1, 2, 8, 8, 128, 32, 2, 1, 1)
    assert lib.fva_gconv_mfma_s2_serves(C.byref(d)) == 1
    rename = {'fva_gconv_fwd': 'fva_gconv_mfma_s2_fwd', 'fva_gconv_wgrad': 'fva_gconv_mfma_s2_wgrad', 'fva_gconv_dgrad': 'fva_gconv_mfma_s2_dgrad'}
    want = []
    for call in copy.deepcopy(plain):
        if call[0] == 'fva_gconv_fwd':
            want.append(['fva_gconv_mfma_s2_pack', call[1], 'ptr', 'ptr', 'ptr', call[-1]])
        if call[0] == 'fva_gconv_wgrad':
            call[6] = lib.fva_gconv_mfma_s2_wgrad_workspace(C.byref(d))
        if call[0] == 'fva_bn_finalize':
            nblk = lib.fva_gconv_mfma_s2_stat_blocks(C.byref(d))
            call[2], call[3] = nblk, lib.fva_bn_partial_rows(nblk)
        call[0] = rename.get(call[0], call[0])
        want.append(call)
    names = [c[0] for c in got]
    assert names == [c[0] for c in want]
    assert got == want
    assert names.index('fva_gconv_mfma_s2_pack') + 1 == names.index('fva_gconv_mfma_s2_fwd')
    assert sum(n.startswith('fva_gconv_mfma_s2') for n in names) == 4 and not any(n in rename for n in names)


def test_mfma_s2_routes_stride_1_as_mfma_does(ro, monkeypatch):
    ro.set_grouped_path('mfma')
    want = _record(monkeypatch, 's1_bf16_train')
    ro.set_grouped_path('mfma_s2')
    got = _record(monkeypatch, 's1_bf16_train')
    assert got == want and any(c[0] == 'fva_gconv_mfma_fwd' for c in got['calls'])


@pytest.mark.parametrize('case', ['s2_train', 'frozen', 'wide_train'])
def test_mfma_s2_leaves_the_layers_it_does_not_serve(ro, golden, monkeypatch, case):     # noqa: F811
    ro.set_grouped_path('mfma_s2')
    assert _record(monkeypatch, case) == golden[f'grouped/{case}']
