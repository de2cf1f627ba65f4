#!/usr/bin/env python3
"""VGG classification train step (vgg16_bn and vgg16): B=64, 3 x 224 x 224, 1000 classes, bf16 compute; forward, CrossEntropyLoss,
backward, FusedSGD(momentum=0.9, nesterov=True, weight_decay=5e-4), dropout on (p = 0.5).

Per model, on identically seeded weights (wall time over --steps steps after --warmup, device synchronised at both ends):
    eager     the library step
    graphed   the same step captured once by graphs.GraphedTrainStep and replayed
    torch     the same network from stock torch.nn modules on the same GPU (bf16 autocast, channels_last, torch.optim.SGD): ATen / MIOpen
eager and torch ALTERNATE in one process, --rounds times each after warm-up (the same clocks and the same neighbours for both); the
figure per mode is the median of its rounds, the spread (max - min) / median is printed beside it.

--passes: the BatchNorm + ReLU streaming passes alone (apply, backward sums, backward apply) at the VGG layer shapes of this batch against
a device-to-device copy of the same number of bytes (bf16, then fp32), with the SiLU passes of the same shapes beside them (tools/bench_bn.py pattern):
microseconds per pass, its share of the copy rate, and the run-to-run spread of the same command.

Prints one JSON line.  usage: python tools/bench_vgg.py [--steps K] [--warmup W] [--batch B] [--size S] [--rounds R] [--models vgg16_bn,vgg16]
[--modes eager,graphed,torch] [--passes]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn as nn
import torch.nn.functional as F

import fastvision_amd
from fastvision_amd import FusedSGD, _lib, ops
from fastvision_amd.classfication import models
from fastvision_amd.loss import CrossEntropyLoss

DEV = 'cuda:0'
NUM_CLASSES = 1000
SGD_KW = dict(lr=0.01, momentum=0.9, nesterov=True, weight_decay=5e-4)
BLOCKS = {'vgg16': [2, 2, 3, 3, 3]}
WIDTHS = [64, 128, 256, 512, 512]


class TorchVGG(nn.Module):
    """The reference's network (classfication/models/vgg.py) from stock modules: what the same GPU does without this library."""

    def __init__(self, name):
        super().__init__()
        bn, width, layers = name.endswith('_bn'), 3, []
        for blocks, out in zip(BLOCKS[name.replace('_bn', '')], WIDTHS):
            for _ in range(blocks):
                layers += [nn.Conv2d(width, out, 3, 1, 1)] + ([nn.BatchNorm2d(out)] if bn else []) + [nn.ReLU(inplace=True)]
                width = out
            layers.append(nn.MaxPool2d(2, 2))
        self.features = nn.Sequential(*layers)
        self.gmp = nn.AdaptiveAvgPool2d((7, 7))
        self.classifier = nn.Sequential(nn.Linear(512 * 49, 4096), nn.ReLU(True), nn.Dropout(), nn.Linear(4096, 4096), nn.ReLU(True), nn.Dropout(),
                                        nn.Linear(4096, NUM_CLASSES))

    def forward(self, x):
        return self.classifier(torch.flatten(self.gmp(self.features(x)), 1))


def batch(B, S):
    g = torch.Generator().manual_seed(0)
    return torch.randn(B, 3, S, S, generator=g).to(DEV), torch.randint(0, NUM_CLASSES, (B,), generator=g).to(DEV)


def make_step(name, mode, images, labels):
    torch.manual_seed(0)
    if mode == 'torch':
        net = TorchVGG(name).to(DEV).to(memory_format=torch.channels_last).train()
        opt = torch.optim.SGD(net.parameters(), **SGD_KW)
        x = images.contiguous(memory_format=torch.channels_last)

        def step():
            with torch.autocast('cuda', dtype=torch.bfloat16):
                loss = F.cross_entropy(net(x).float(), labels)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            return loss.detach()
        return step
    net = getattr(models, name)(num_classes=NUM_CLASSES).to(DEV).train()
    crit = CrossEntropyLoss()
    opt = FusedSGD(net.parameters(), capturable=(mode == 'graphed'), **SGD_KW)
    if mode == 'graphed':
        from fastvision_amd.graphs import GraphedTrainStep
        g = GraphedTrainStep(net, lambda p, t: crit(p, t), opt, images, labels.float().view(-1, 1))
        return lambda: g()

    def step():
        pred = net(images)
        opt.zero_grad(set_to_none=True)
        loss = crit(pred, labels)
        loss.backward()
        opt.step()
        return loss.detach()
    return step


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps, float(loss)


def run_model(name, modes, images, labels, steps, warmup, rounds):
    fns = {m: make_step(name, m, images, labels) for m in modes}
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    ms = {m: [] for m in modes}
    last = {}
    for _ in range(rounds):                       # the modes alternate: round r of every mode before round r + 1 of any
        for m in modes:
            t, last[m] = timed(fns[m], steps)
            ms[m].append(t)
    out = {}
    for m in modes:
        med = statistics.median(ms[m])
        out[m] = {'ms_per_step': round(med, 3), 'img_per_s': round(images.shape[0] * 1e3 / med, 1), 'spread': round((max(ms[m]) - min(ms[m])) / med, 4),
                  'last_loss': round(last[m], 5)}
    return out


def _time_us(fn, reps=20):
    for _ in range(3):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) * 1e3 / reps


def bench_passes(B, S, dt=torch.bfloat16):
    """apply / backward sums / backward apply, ReLU and SiLU, at the five VGG stage shapes, each against a copy of the same bytes."""
    lib, code, p, st = _lib.load(), ops._code(dt), ops._p, ops._stream
    rows = []
    for stage, Cc in enumerate(WIDTHS):
        H = S >> stage
        M = B * H * H
        g = torch.Generator().manual_seed(stage)
        y = torch.randn(M, Cc, generator=g).to(dt).to(DEV)
        dz = torch.randn(M, Cc, generator=g).to(dt).to(DEV)
        scale, shift = (torch.rand(Cc, generator=g) + 0.5).to(DEV), torch.randn(Cc, generator=g).to(DEV)
        mean, rstd = torch.randn(Cc, generator=g).to(DEV), (torch.rand(Cc, generator=g) + 0.5).to(DEV)
        gamma = torch.ones(Cc, device=DEV)
        z = torch.empty((B, H + 2, H + 2, Cc), dtype=dt, device=DEV)
        nb = lib.fva_bn_bwd_blocks(code, M, Cc)
        part = torch.zeros((lib.fva_bn_partial_rows(nb), 2, Cc), dtype=torch.float32, device=DEV)
        coef = torch.empty((3, Cc), dtype=torch.float32, device=DEV)
        dg, db = torch.empty(Cc, device=DEV), torch.empty(Cc, device=DEV)
        _lib.call('fva_bn_relu_bwd_reduce', code, p(dz), p(y), p(scale), p(shift), p(mean), p(rstd), p(part), nb, M, Cc, st())
        _lib.call('fva_bn_bwd_finalize', p(part), nb, part.shape[0], M, Cc, p(gamma), p(rstd), p(dg), p(db), 0, p(coef), st())
        src2, dst2 = torch.empty(2 * M * Cc, dtype=dt, device=DEV), torch.empty(2 * M * Cc, dtype=dt, device=DEV)
        copies = {'apply': lambda: dst2[:M * Cc].copy_(src2[:M * Cc]),                       # 2 + 2 bytes per element
                  'bwd_reduce': lambda: dst2[:M * Cc].copy_(src2[:M * Cc]),                  # 4 read (a copy of half of it moves the same 4)
                  'bwd_apply': lambda: dst2[:3 * M * Cc // 2].copy_(src2[:3 * M * Cc // 2])}   # 4 + 2
        calls = {
            'relu': {'apply': lambda: _lib.call('fva_bn_relu_apply', code, p(y), p(scale), p(shift), p(z), 1, B, H, H, Cc, st()),
                     'bwd_reduce': lambda: _lib.call('fva_bn_relu_bwd_reduce', code, p(dz), p(y), p(scale), p(shift), p(mean), p(rstd), p(part), nb, M, Cc, st()),
                     'bwd_apply': lambda: _lib.call('fva_bn_relu_bwd_apply', code, p(dz), p(y), p(scale), p(shift), p(mean), p(rstd), p(coef), p(z), 1, B, H, H, Cc, st())},
            'silu': {'apply': lambda: _lib.call('fva_bn_silu_apply', code, p(y), p(scale), p(shift), None, 0, p(z), 1, B, H, H, Cc, st()),
                     'bwd_reduce': lambda: _lib.call('fva_bn_silu_bwd_reduce', code, p(dz), p(y), p(scale), p(shift), p(mean), p(rstd), p(part), nb, M, Cc, st()),
                     'bwd_apply': lambda: _lib.call('fva_bn_silu_bwd_apply', code, p(dz), p(y), p(scale), p(shift), p(mean), p(rstd), p(coef), p(z), 1, B, H, H, Cc, st())},
        }
        row = {'shape': [B, H, H, Cc]}
        for which in ('apply', 'bwd_reduce', 'bwd_apply'):
            copy_us = _time_us(copies[which])
            r = [_time_us(calls['relu'][which]) for _ in range(3)]
            s = [_time_us(calls['silu'][which]) for _ in range(3)]
            row[which] = {'copy_us': round(copy_us, 1), 'relu_us': round(statistics.median(r), 1), 'silu_us': round(statistics.median(s), 1),
                          'relu_share_of_copy_rate': round(copy_us / statistics.median(r), 3), 'relu_spread': round((max(r) - min(r)) / statistics.median(r), 3),
                          'silu_spread': round((max(s) - min(s)) / statistics.median(s), 3)}
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--size', type=int, default=224)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--models', default='vgg16_bn,vgg16')
    ap.add_argument('--modes', default='eager,graphed,torch')
    ap.add_argument('--passes', action='store_true')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_vgg needs a GPU'
    images, labels = batch(a.batch, a.size)
    res = {'workload': f'VGG classification train step B={a.batch} 3x{a.size}x{a.size} {NUM_CLASSES} classes bf16, dropout 0.5, SGD nesterov',
           'steps': a.steps, 'warmup': a.warmup, 'rounds': a.rounds, 'device': torch.cuda.get_device_name(0)}
    with fastvision_amd.compute_dtype(torch.bfloat16):
        for name in [m for m in a.models.split(',') if m]:
            res[name] = run_model(name, a.modes.split(','), images, labels, a.steps, a.warmup, a.rounds)
            torch.cuda.empty_cache()
        if a.passes:
            res['bn_relu_passes'] = bench_passes(a.batch, a.size)
            res['bn_relu_passes_fp32'] = bench_passes(a.batch, a.size, torch.float32)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
