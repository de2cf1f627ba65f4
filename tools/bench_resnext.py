#!/usr/bin/env python3
"""ResNeXt classification train step (resnext50_32x4d and resnext101_32x8d): B=128, 3 x 224 x 224, 1000 classes, bf16 compute; forward,
CrossEntropyLoss, backward, FusedSGD(momentum=0.9, nesterov=True, weight_decay=5e-4).  The method of tools/bench_resnet.py:

Per model, on identically seeded weights (wall time over --steps steps after --warmup, device synchronised at both ends):
    eager     the library step
    torch     the same network from stock torch.nn modules on the same GPU (bf16 autocast, channels_last, torch.optim.SGD)
eager and torch ALTERNATE in one process, --rounds times each after warm-up; the figure per mode is the median of its rounds.  The eager
step is taken once per grouped path of --grouped (resnet_ops.set_grouped_path: 'plain', the FMA kernels of csrc/grouped.hip, and 'mfma',
the matrix-unit kernels of csrc/grouped_mfma.hip at the stride-1 layers), all in the same alternation; every figure carries a ``grouped`` key.

Per grouped kernel (forward with statistics, data gradient, weight gradient; under 'mfma' also the pack launch that precedes every forward)
at the six stride-1 shapes of DESIGN 3.12 and per path: device-event time over --iters launches after warm-up, the paths and a
device-to-device copy of x read + y written once (the floor's bytes) ALTERNATING --rounds times in one process; per figure the median, the
best, and the spread between its rounds, the useful GFLOP, and under 'mfma' whether every round beat every round of 'plain'.

Writes one JSON object to --out (default profiles/bench_resnext.json) and prints it as one line.
usage: python tools/bench_resnext.py [--steps K] [--warmup W] [--batch B] [--size S] [--rounds R] [--iters N] [--models a,b] [--modes eager,torch]
[--grouped plain,mfma] [--no-kernels] [--out PATH]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_resnet import DEV, NUM_CLASSES, SGD_KW, event_us, timed          # noqa: E402  (puts the repository root on the path too)

import torch          # noqa: E402
import torch.nn as nn          # noqa: E402
import torch.nn.functional as F          # noqa: E402

import fastvision_amd          # noqa: E402
from fastvision_amd import FusedSGD, _lib, ops, resnet_ops          # noqa: E402
from fastvision_amd.classfication import models          # noqa: E402
from fastvision_amd.loss import CrossEntropyLoss          # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCKS = {'resnext50_32x4d': ([3, 4, 6, 3], 32, 4), 'resnext101_32x8d': ([3, 4, 23, 3], 32, 8)}
# (model, stage): C, Cg, map at 224 x 224 -- the stride-1 grouped layers of DESIGN 3.12's floor table
SHAPES = [('50_32x4d res2', 128, 4, 56), ('50_32x4d res3', 256, 8, 28), ('50_32x4d res4', 512, 16, 14), ('50_32x4d res5', 1024, 32, 7),
          ('101_32x8d res2', 256, 8, 56), ('101_32x8d res5', 2048, 64, 7)]


def _cb(cin, cout, k, s=1, groups=1):
    return nn.Sequential(nn.Conv2d(cin, cout, k, s, k // 2, groups=groups, bias=False), nn.BatchNorm2d(cout))


class _TorchBlock(nn.Module):
    def __init__(self, cin, mid, stride, groups, width):
        super().__init__()
        total, cout = groups * width, mid * 4
        self.body = nn.Sequential(_cb(cin, total, 1), nn.ReLU(True), _cb(total, total, 3, stride, groups), nn.ReLU(True), _cb(total, cout, 1))
        self.short = _cb(cin, cout, 1, stride) if (stride != 1 or cin != cout) else None

    def forward(self, x):
        return F.relu(self.body(x) + (x if self.short is None else self.short(x)))


class TorchResNeXt(nn.Module):
    """The reference's network (classfication/models/resnext.py) from stock modules: what the same GPU does without this library."""

    def __init__(self, name):
        super().__init__()
        blocks, groups, width = BLOCKS[name]
        layers = [_cb(3, 64, 7, 2), nn.ReLU(True), nn.MaxPool2d(3, 2, 1)]
        planes = 64
        for stage, (n, mid) in enumerate(zip(blocks, (64, 128, 256, 512))):
            for i in range(n):
                layers.append(_TorchBlock(planes, mid, 2 if (i == 0 and stage > 0) else 1, groups, width))
                planes = mid * 4
            width *= 2
        self.features = nn.Sequential(*layers)
        self.fc = nn.Linear(planes, NUM_CLASSES)

    def forward(self, x):
        return self.fc(torch.flatten(F.adaptive_avg_pool2d(self.features(x), 1), 1))


def make_step(name, mode, images, labels):
    """``mode``: 'torch', or 'eager/<grouped path>'"""
    torch.manual_seed(0)
    if mode == 'torch':
        net = TorchResNeXt(name).to(DEV).to(memory_format=torch.channels_last).train()
        opt = torch.optim.SGD(net.parameters(), **SGD_KW)
        x = images.to(memory_format=torch.channels_last)

        def step():
            with torch.autocast('cuda', dtype=torch.bfloat16):
                loss = F.cross_entropy(net(x), labels)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            return loss
        return step
    net = getattr(models, name)(num_classes=NUM_CLASSES).to(DEV).train()
    opt = FusedSGD(net.parameters(), capturable=True, **SGD_KW)
    crit = CrossEntropyLoss()

    grouped = mode.split('/')[1]

    def step():
        prev = resnet_ops.set_grouped_path(grouped)         # read at call time by every grouped layer of the forward
        try:
            pred = net(images)
        finally:
            resnet_ops.set_grouped_path(prev)
        opt.zero_grad(set_to_none=True)
        loss = crit(pred, labels)
        loss.backward()
        opt.step()
        return loss
    return step


def _modes(args):
    return [f'eager/{g}' for m in args.modes.split(',') if m == 'eager' for g in args.grouped.split(',')] + [m for m in args.modes.split(',') if m != 'eager']


def bench_models(args, images, labels):
    out = {}
    for name in args.models.split(','):
        steps = {m: make_step(name, m, images, labels) for m in _modes(args)}
        for st in steps.values():
            for _ in range(args.warmup):
                st()
        torch.cuda.synchronize()
        runs, last = {m: [] for m in steps}, {}
        for _ in range(args.rounds):
            for m, st in steps.items():
                ms, last[m] = timed(st, args.steps)
                runs[m].append(ms)
        out[name] = {m: {'ms_per_step': round(statistics.median(v), 3), 'img_per_s': round(args.batch / statistics.median(v) * 1e3, 1),
                         'spread': round((max(v) - min(v)) / statistics.median(v), 4), 'last_loss': round(last[m], 5),
                         'grouped': m.split('/')[1] if '/' in m else None} for m, v in runs.items()}
        del steps
        torch.cuda.empty_cache()
    return out


ENTRY = {'plain': ('fva_gconv_fwd', 'fva_gconv_dgrad', 'fva_gconv_wgrad', 'fva_gconv_stat_blocks', 'fva_gconv_wgrad_workspace'),
         'mfma': ('fva_gconv_mfma_fwd', 'fva_gconv_mfma_dgrad', 'fva_gconv_mfma_wgrad', 'fva_gconv_mfma_stat_blocks', 'fva_gconv_mfma_wgrad_workspace')}


def _halo_randn(B, H, Cc, dt):
    t = torch.zeros(B, H + 2, H + 2, Cc, dtype=dt, device=DEV)
    t[:, 1:-1, 1:-1] = torch.randn(B, H, H, Cc, device=DEV).to(dt)
    return t


def bench_kernels(args):
    dt, code, p, st = torch.bfloat16, _lib.BF16, ops._p, ops._stream
    lib = _lib.load()
    B, it, E = args.batch, args.iters, 2
    paths = args.grouped.split(',')
    rows = []
    for tag, Cc, Cg, H in SHAPES:
        H = H * args.size // 224
        d = _lib.GConvDesc(code, B, H, H, Cc, Cc // Cg, 1, 1, 1)
        M = B * H * H
        x, dy = _halo_randn(B, H, Cc, dt), _halo_randn(B, H, Cc, dt)
        w = torch.randn(Cc, Cg, 3, 3, device=DEV) * (9 * Cg) ** -0.5
        y = torch.empty((M, Cc), dtype=dt, device=DEV)
        dx = torch.empty((B, H, H, Cc), dtype=dt, device=DEV)
        dw = torch.empty((Cc, Cg, 3, 3), dtype=torch.float32, device=DEV)
        nbytes, gflop = 2 * M * Cc * E, 2.0 * M * Cc * Cg * 9 / 1e9
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device=DEV)
        dst = torch.empty_like(src)
        fns, keep = {}, []
        for g in paths:
            if g == 'mfma' and lib.fva_gconv_mfma_serves(C.byref(d)) != 1:
                continue
            fwd, dgrad, wgrad, blocks, wsf = ENTRY[g]
            nblk = getattr(lib, blocks)(C.byref(d))
            stats = torch.empty((lib.fva_bn_partial_rows(nblk), 2, Cc), dtype=torch.float32, device=DEV)
            wsb = getattr(lib, wsf)(C.byref(d))
            ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
            wf = wb = w
            if g == 'mfma':
                nb = lib.fva_gconv_mfma_pack_bytes(C.byref(d))
                wf, wb = torch.empty(nb, dtype=torch.uint8, device=DEV), torch.empty(nb, dtype=torch.uint8, device=DEV)
                fns[(g, 'fva_gconv_mfma_pack')] = lambda wf=wf, wb=wb: _lib.call('fva_gconv_mfma_pack', C.byref(d), p(w), p(wf), p(wb), st())
                fns[(g, 'fva_gconv_mfma_pack')]()
            keep.append((stats, ws, wf, wb))
            fns[(g, fwd)] = lambda fwd=fwd, wf=wf, stats=stats: _lib.call(fwd, C.byref(d), p(x), p(wf), p(y), p(stats), st())
            fns[(g, dgrad)] = lambda dgrad=dgrad, wb=wb: _lib.call(dgrad, C.byref(d), p(dy), p(wb), p(dx), st())
            fns[(g, wgrad)] = lambda wgrad=wgrad, ws=ws, wsb=wsb: _lib.call(wgrad, C.byref(d), p(x), p(dy), p(dw), p(ws), wsb, st())
        us = {k: [] for k in fns}
        copy_us = []
        for _ in range(args.rounds):                        # the paths and the copy alternate: one round = every figure once
            for k, fn in fns.items():
                us[k].append(event_us(fn, it))
            copy_us.append(event_us(lambda: dst.copy_(src), it))
        cu = min(copy_us)
        for (g, name), v in us.items():
            med = statistics.median(v)
            r = {'kernel': name, 'grouped': g, 'layer': tag, 'Cg': Cg, 'shape': [B, H, H, Cc], 'bytes': nbytes, 'us': round(med, 1),
                 'us_best': round(min(v), 1), 'us_rounds': [round(t, 1) for t in v], 'spread': round((max(v) - min(v)) / med, 4),
                 'gb_per_s': round(nbytes / med / 1e3, 1), 'copy_us': round(cu, 1), 'copy_gb_per_s': round(nbytes / cu / 1e3, 1),
                 'share_of_copy_rate': round(cu / med, 3), 'useful_gflop': round(gflop, 2), 'useful_tflop_per_s': round(gflop / med * 1e3, 2),
                 'hbm_floor_us_at_5p5_tb_per_s': round(nbytes / 5.5e6, 1)}
            twin = ENTRY['plain'][ENTRY['mfma'].index(name)] if g == 'mfma' and name in ENTRY['mfma'] else None
            if twin is not None and ('plain', twin) in us:
                r['plain_us'] = round(statistics.median(us[('plain', twin)]), 1)
                r['beats_plain_in_every_round'] = max(v) < min(us[('plain', twin)])      # by more than the spread between rounds of a mode
            rows.append(r)
        del x, dy, y, dx, keep, fns
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--size', type=int, default=224)
    ap.add_argument('--models', default='resnext50_32x4d,resnext101_32x8d')
    ap.add_argument('--modes', default='eager,torch')
    ap.add_argument('--grouped', default='plain,mfma')
    ap.add_argument('--no-kernels', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bench_resnext.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_resnext: no GPU -- nothing to measure here')
    gen = torch.Generator().manual_seed(0)
    images = torch.randn(args.batch, 3, args.size, args.size, generator=gen).to(DEV)
    labels = torch.randint(0, NUM_CLASSES, (args.batch,), generator=gen).to(DEV)
    out = {'workload': f'ResNeXt classification train step B={args.batch} 3x{args.size}x{args.size} {NUM_CLASSES} classes bf16, SGD nesterov',
           'steps': args.steps, 'warmup': args.warmup, 'rounds': args.rounds, 'device': torch.cuda.get_device_name(0),
           'reference': 'torch: the same network from stock torch.nn on the same device, bf16 autocast, channels_last, torch.optim.SGD',
           'grouped_paths': {'plain': 'the FMA kernels of csrc/grouped.hip at every grouped layer (the default of resnet_ops)',
                             'mfma': 'the matrix-unit kernels of csrc/grouped_mfma.hip at the bf16 stride-1 layers, plain elsewhere'}}
    for g in args.grouped.split(','):
        if g not in ENTRY:
            raise SystemExit(f'bench_resnext: --grouped takes plain and mfma, got {g}')
    with fastvision_amd.compute_dtype(torch.bfloat16):
        out.update(bench_models(args, images, labels))
        if not args.no_kernels:
            out['kernels'] = bench_kernels(args)
            out['kernels_measured_against'] = 'a device-to-device copy of x read + y written (the same number of bytes), same process, alternating with the kernels'
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
