"""The launches of the classifier blocks (vgg_ops, resnet_ops; their shared part is conv_bn_ops), recorded on CPU tensors without launching
anything and compared with tests/golden/conv_bn_node_launches.json: entry names, order, scalar arguments, the pattern of null pointers and
the descriptor fields.  ``_lib.call`` is replaced by a recorder that returns without calling, ``_stream`` by a null stream and ``require_gpu``
by a no-op, in the test only; the count and size helpers reached through ``_lib.load()`` are pure host functions of the built library.
Pointer values and identities are not recorded (they depend on the allocator); the dataflow is what the GPU suites check.

The golden was written by this file's ``__main__`` on a checkout of the commit BEFORE the three conv -> BatchNorm -> ReLU nodes became one
(where conv_bn_ops does not exist yet and is skipped), never by the code under test:

    python tests/test_conv_bn_node_cpu.py            # writes tests/golden/conv_bn_node_launches.json
"""
import ctypes as C
import importlib
import json
import os
import sys

import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'conv_bn_node_launches.json')
_BYREF = type(C.byref(C.c_int()))


@pytest.fixture(scope='module')
def built():
    import __graft_entry__ as ge
    ge.build()
    from fastvision_amd import _lib
    return _lib


def _ptr(v):
    return 'null' if not v else 'ptr'


def _arg(a):
    if a is None:
        return 'null'
    if isinstance(a, (bool, int, float)):
        return a
    if isinstance(a, C.c_void_p):
        return _ptr(a.value)
    if isinstance(a, _BYREF):
        obj = a._obj
        out = {'type': type(obj).__name__}
        for name, ft in getattr(obj, '_fields_', ()):
            if not (ft is C.c_void_p or hasattr(ft, 'contents')):          # pointer fields stay out of the record
                v = getattr(obj, name)
                out[name] = v if isinstance(v, (int, float)) else list(v)
        return out
    raise TypeError(f'unexpected argument {a!r}')


def _host_modules():
    mods = []
    for name in ('ops', 'resnet_ops', 'vgg_ops', 'conv_bn_ops'):
        try:
            mods.append(importlib.import_module('fastvision_amd.' + name))
        except ImportError:
            if name != 'conv_bn_ops':                   # absent only where the golden is written
                raise
    return mods


def _patch(mp, trace):
    from fastvision_amd import _lib, ops
    mp.setattr(_lib, 'call', lambda name, *args: trace.append([name] + [_arg(a) for a in args]) or 0)
    for mod in _host_modules():
        for name, fn in (('_stream', lambda: C.c_void_p(0)), ('require_gpu', lambda t, who: None)):
            if hasattr(mod, name):
                mp.setattr(mod, name, fn)
    # process-wide host state that earlier tests or the environment may have touched: every case starts from the defaults
    mp.delenv('FVA_PACK_TILED', raising=False)
    mp.setattr(ops, '_registry', ops._PackRegistry())
    mp.setitem(ops._PLAN, 'mode', 'auto')
    mp.setitem(ops._PLAN, 'applied', None)
    mp.setitem(ops._SIDE, 'on', True)
    mp.setitem(ops._SIDE, 'keep', [])
    mp.setitem(ops._SIDE, 'queued', False)
    mp.setitem(ops._DEFER, 'pending', None)


# ------------------------------------------------------------------------------------------------ the cases
def _x(*shape, grad=True, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype).requires_grad_(grad)


def _bwd(z):
    z.float().sum().backward()


def _conv(cin, cout, k=3, stride=1, bias=False, groups=1):
    return nn.Conv2d(cin, cout, k, stride, k // 2, bias=bias, groups=groups)


def _freeze(bn, only_x=False, mods=()):
    bn.eval()
    if only_x:
        for m in (bn,) + tuple(mods):
            for p in m.parameters():
                p.requires_grad_(False)
    return bn


def _vgg(case):
    from fastvision_amd import vgg_ops as vo
    f32 = torch.float32
    conv, bn = _conv(64, 64, bias=True), nn.BatchNorm2d(64)
    if case == 'train':
        _bwd(vo.conv_bn_relu(_x(2, 64, 8, 8), conv, bn, f32))
    elif case == 'train_rgb':
        _bwd(vo.conv_bn_relu(_x(2, 3, 8, 8, grad=False), _conv(3, 64, bias=True), bn, f32))
    elif case == 'frozen_all':
        _bwd(vo.conv_bn_relu(_x(2, 64, 8, 8), conv, _freeze(bn), f32))
    elif case == 'frozen_x_only':
        _bwd(vo.conv_bn_relu(_x(2, 64, 8, 8), conv, _freeze(bn, True, (conv,)), f32))
    elif case == 'eval_no_grad':
        with torch.no_grad():
            vo.conv_bn_relu(_x(2, 64, 8, 8), conv, _freeze(bn), f32)
    elif case == 'train_twice_weight_updated':
        _bwd(vo.conv_bn_relu(_x(2, 64, 8, 8), conv, bn, f32))
        with torch.no_grad():
            conv.weight.add_(1.0)
        _bwd(vo.conv_bn_relu(_x(2, 64, 8, 8), conv, bn, f32))
    else:
        raise KeyError(case)


def _resnet(case):
    from fastvision_amd import resnet_ops as ro
    f32, bf16 = torch.float32, torch.bfloat16
    if case == '3x3s1_train':
        _bwd(ro.conv_bn_relu(_x(2, 64, 8, 8), _conv(64, 64), nn.BatchNorm2d(64), f32))
    elif case == '3x3s2_train':
        _bwd(ro.conv_bn_relu(_x(2, 64, 8, 8), _conv(64, 128, 3, 2), nn.BatchNorm2d(128), f32))
    elif case == '1x1_bf16_train':
        _bwd(ro.conv_bn_relu(_x(2, 64, 8, 8), _conv(64, 128, 1), nn.BatchNorm2d(128), bf16))
    elif case == '3x3s1_frozen':
        _bwd(ro.conv_bn_relu(_x(2, 64, 8, 8), _conv(64, 64), _freeze(nn.BatchNorm2d(64)), f32))
    elif case == 'eval_no_grad':
        with torch.no_grad():
            ro.conv_bn_relu(_x(2, 64, 8, 8), _conv(64, 64), _freeze(nn.BatchNorm2d(64)), f32)
    elif case == 'wide_train':
        _bwd(ro.conv_bn_relu(_x(2, 64, 2, 2), _conv(64, 2048, 1), nn.BatchNorm2d(2048), f32))
    elif case == 'wide_frozen_raises':
        z = ro.conv_bn_relu(_x(2, 64, 2, 2), _conv(64, 2048, 1), _freeze(nn.BatchNorm2d(2048)), f32)
        with pytest.raises(RuntimeError) as e:
            _bwd(z)
        assert str(e.value) == ro.WIDE_FROZEN
        return {'raises': str(e.value)}
    elif case in ('linked_tail', 'unlinked_tail'):
        x = _x(2, 64, 8, 8)
        h = ro.conv_bn_relu(x, _conv(64, 64), nn.BatchNorm2d(64), f32)
        _bwd(ro.conv_bn_add_relu(h, _conv(64, 64), nn.BatchNorm2d(64), x if case == 'linked_tail' else x * 1.0, dtype=f32))
    else:
        raise KeyError(case)


def _grouped(case):
    from fastvision_amd import resnet_ops as ro
    f32, bf16 = torch.float32, torch.bfloat16
    conv = lambda c, s=1: _conv(c, c, 3, s, groups=32)
    if case == 's1_bf16_train':
        _bwd(ro.conv_bn_relu(_x(2, 128, 8, 8), conv(128), nn.BatchNorm2d(128), bf16))
    elif case == 's2_train':
        _bwd(ro.conv_bn_relu(_x(2, 128, 8, 8), conv(128, 2), nn.BatchNorm2d(128), f32))
    elif case == 'frozen':
        _bwd(ro.conv_bn_relu(_x(2, 128, 8, 8), conv(128), _freeze(nn.BatchNorm2d(128)), f32))
    elif case == 'wide_train':
        _bwd(ro.conv_bn_relu(_x(2, 2048, 2, 2), conv(2048), nn.BatchNorm2d(2048), f32))
    else:
        raise KeyError(case)


def _neighbour(case):
    from fastvision_amd import resnet_ops as ro, vgg_ops as vo
    f32 = torch.float32
    if case in ('stem_train', 'stem_frozen'):
        bn = nn.BatchNorm2d(64)
        _bwd(ro.stem_bn_relu(_x(2, 3, 16, 16, grad=False), nn.Conv2d(3, 64, 7, 2, 3, bias=False), bn if case == 'stem_train' else _freeze(bn), f32))
    elif case == 'add_relu_s2_shortcut':
        x = _x(2, 64, 8, 8)
        h = _x(2, 128, 4, 4)
        _bwd(ro.conv_bn_add_relu(h, _conv(128, 128), nn.BatchNorm2d(128), x, _conv(64, 128, 1, 2), nn.BatchNorm2d(128), dtype=f32))
    elif case == 'max_pool2':
        _bwd(vo.max_pool2(_x(2, 64, 6, 6), f32))
    elif case == 'max_pool3s2':
        _bwd(ro.max_pool3s2(_x(2, 64, 6, 6), f32))
    else:
        raise KeyError(case)


CASES = ([('vgg', c, _vgg) for c in ('train', 'train_rgb', 'frozen_all', 'frozen_x_only', 'eval_no_grad', 'train_twice_weight_updated')]
         + [('resnet', c, _resnet) for c in ('3x3s1_train', '3x3s2_train', '1x1_bf16_train', '3x3s1_frozen', 'eval_no_grad', 'wide_train',
                                             'wide_frozen_raises', 'linked_tail', 'unlinked_tail')]
         + [('grouped', c, _grouped) for c in ('s1_bf16_train', 's2_train', 'frozen', 'wide_train')]
         + [('neighbour', c, _neighbour) for c in ('stem_train', 'stem_frozen', 'add_relu_s2_shortcut', 'max_pool2', 'max_pool3s2')])


def _record(mp, run, case):
    trace = []
    _patch(mp, trace)
    torch.manual_seed(0)
    extra = run(case)
    return {'calls': trace, **(extra or {})}


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_golden_holds_exactly_these_cases(golden):
    assert sorted(golden) == sorted(f'{fam}/{case}' for fam, case, _ in CASES)


@pytest.mark.parametrize('fam,case,run', CASES, ids=[f'{f}/{c}' for f, c, _ in CASES])
def test_launches_equal_the_recorded_ones(built, golden, monkeypatch, fam, case, run):
    got = json.loads(json.dumps(_record(monkeypatch, run, case)))        # through JSON: tuples and lists compare alike
    want = golden[f'{fam}/{case}']
    assert [c[0] for c in got['calls']] == [c[0] for c in want['calls']]
    assert got == want


def test_the_golden_cases_take_the_routes_they_are_named_for(golden):
    names = lambda key: [c[0] for c in golden[key]['calls']]
    assert 'fva_bn_frozen_bwd_finalize' not in names('vgg/frozen_x_only') and 'fva_conv_wgrad' not in names('vgg/frozen_x_only')
    assert 'fva_conv_pack_weights_tiled' in names('vgg/train_twice_weight_updated')
    dgrad = lambda key: [c for c in golden[key]['calls'] if c[0] == 'fva_conv_dgrad']
    assert dgrad('resnet/linked_tail')[-1][5] == 'ptr' and dgrad('resnet/unlinked_tail')[-1][5] == 'null'
    assert 'fva_bn_add_relu_bwd_reduce' in names('resnet/wide_train') and 'fva_bn_add_relu_bwd_reduce' in names('grouped/wide_train')
    assert 'fva_bn_bias_running_mean' in names('vgg/train') and 'fva_bn_eval_coeffs_bias' in names('vgg/eval_no_grad')
    assert 'fva_side_stream_fork' not in names('vgg/train_rgb')                    # a derived weight: its gradient stays on the main stream
    assert golden['resnet/wide_frozen_raises']['raises'].startswith('conv_bn_relu: backward with frozen statistics')


@pytest.mark.parametrize('fam', ['vgg', 'resnet', 'grouped'])
def test_saved_state_serves_one_backward(built, monkeypatch, fam):
    from fastvision_amd import resnet_ops as ro, vgg_ops as vo
    _patch(monkeypatch, [])
    fn, conv = {'vgg': (vo.conv_bn_relu, _conv(64, 64, bias=True)), 'resnet': (ro.conv_bn_relu, _conv(64, 64)),
                'grouped': (ro.conv_bn_relu, _conv(128, 128, groups=32))}[fam]
    bn = nn.BatchNorm2d(conv.out_channels)
    z = fn(_x(2, conv.in_channels, 8, 8), conv, bn, torch.float32)
    z.float().sum().backward(retain_graph=True)
    with pytest.raises(RuntimeError, match='conv_bn_relu: the buffers saved for backward have already been released'):
        z.float().sum().backward()


if __name__ == '__main__':
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    out = {}
    for fam, case, run in CASES:
        with pytest.MonkeyPatch.context() as mp:
            out[f'{fam}/{case}'] = _record(mp, run, case)
        print(f'{fam}/{case}: {len(out[f"{fam}/{case}"]["calls"])} calls')
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    with open(GOLDEN, 'w') as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write('\n')
