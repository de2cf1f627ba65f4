#!/usr/bin/env python3
"""ResNet classification train step (resnet50 and resnet18): B=128, 3 x 224 x 224, 1000 classes, bf16 compute; forward, CrossEntropyLoss,
backward, FusedSGD(momentum=0.9, nesterov=True, weight_decay=5e-4).

Per model, on identically seeded weights (wall time over --steps steps after --warmup, device synchronised at both ends):
    eager     the library step
    torch     the same network from stock torch.nn modules on the same GPU (bf16 autocast, channels_last, torch.optim.SGD): ATen / MIOpen --
              the reference figure
eager and torch ALTERNATE in one process, --rounds times each after warm-up (the same clocks and the same neighbours for both); the
figure per mode is the median of its rounds, the spread (max - min) / median is printed beside it.

Per new kernel of csrc/resnet.hip, at the shapes this batch gives it: device-event time over --iters launches after warm-up, the bytes
the algorithm moves (computed here from the shape), the achieved GB/s, and the time and rate of a device-to-device copy of the same
number of bytes measured in the same process right beside it.

The stem's three launches (fva_stem7_patches, the 1x1 GEMM over the patch matrix forward, fva_conv_wgrad over it backward) are timed on
their own at this batch and reported as a share of each model's eager step.

Prints one JSON line.  usage: python tools/bench_resnet.py [--steps K] [--warmup W] [--batch B] [--size S] [--rounds R] [--iters N]
[--models resnet50,resnet18] [--modes eager,torch] [--no-kernels]"""
import argparse
import ctypes as C
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
BLOCKS = {'resnet18': (False, [2, 2, 2, 2]), 'resnet50': (True, [3, 4, 6, 3])}


def _cb(cin, cout, k, s=1):
    return nn.Sequential(nn.Conv2d(cin, cout, k, s, k // 2, bias=False), nn.BatchNorm2d(cout))


class _TorchBlock(nn.Module):
    def __init__(self, bottleneck, cin, mid, stride, down):
        super().__init__()
        if bottleneck:
            cout = mid * 4
            self.body = nn.Sequential(_cb(cin, mid, 1), nn.ReLU(True), _cb(mid, mid, 3, stride), nn.ReLU(True), _cb(mid, cout, 1))
            down = down or cin != cout
        else:
            cout = mid
            self.body = nn.Sequential(_cb(cin, mid, 3, stride), nn.ReLU(True), _cb(mid, cout, 3))
        self.short = _cb(cin, cout, 1, stride) if down else None

    def forward(self, x):
        return F.relu(self.body(x) + (x if self.short is None else self.short(x)))


class TorchResNet(nn.Module):
    """The reference's network (classfication/models/resnet.py) from stock modules: what the same GPU does without this library."""

    def __init__(self, name):
        super().__init__()
        bottleneck, blocks = BLOCKS[name]
        layers = [_cb(3, 64, 7, 2), nn.ReLU(True), nn.MaxPool2d(3, 2, 1)]
        planes = 64
        for stage, (n, mid) in enumerate(zip(blocks, (64, 128, 256, 512))):
            for i in range(n):
                layers.append(_TorchBlock(bottleneck, planes, mid, 2 if (i == 0 and stage > 0) else 1, i == 0 and stage > 0))
                planes = mid * (4 if bottleneck else 1)
        self.features = nn.Sequential(*layers)
        self.fc = nn.Linear(planes, NUM_CLASSES)

    def forward(self, x):
        return self.fc(torch.flatten(F.adaptive_avg_pool2d(self.features(x), 1), 1))


def make_step(name, mode, images, labels):
    torch.manual_seed(0)
    if mode == 'torch':
        net = TorchResNet(name).to(DEV).to(memory_format=torch.channels_last).train()
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

    def step():
        pred = net(images)
        opt.zero_grad(set_to_none=True)
        loss = crit(pred, labels)
        loss.backward()
        opt.step()
        return loss
    return step


def timed(step, steps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        loss = step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / steps * 1e3, float(loss.detach())


def bench_models(args, images, labels):
    out = {}
    for name in args.models.split(','):
        steps = {m: make_step(name, m, images, labels) for m in args.modes.split(',')}
        for st in steps.values():
            for _ in range(args.warmup):
                st()
        torch.cuda.synchronize()
        runs = {m: [] for m in steps}
        last = {}
        for _ in range(args.rounds):
            for m, st in steps.items():
                ms, last[m] = timed(st, args.steps)
                runs[m].append(ms)
        out[name] = {m: {'ms_per_step': round(statistics.median(v), 3), 'img_per_s': round(args.batch / statistics.median(v) * 1e3, 1),
                         'spread': round((max(v) - min(v)) / statistics.median(v), 4), 'last_loss': round(last[m], 5)} for m, v in runs.items()}
        del steps
        torch.cuda.empty_cache()
    return out


def event_us(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3


def with_copy(name, fn, nbytes, iters, shape):
    """the kernel and a device copy of the same bytes (half read, half written), alternating twice; the better of each"""
    src = torch.empty(max(nbytes // 2, 16), dtype=torch.uint8, device=DEV)
    dst = torch.empty_like(src)
    k, c = [], []
    for _ in range(2):
        k.append(event_us(fn, iters))
        c.append(event_us(lambda: dst.copy_(src), iters))
    ku, cu = min(k), min(c)
    return {'kernel': name, 'shape': list(shape), 'bytes': nbytes, 'us': round(ku, 1), 'gb_per_s': round(nbytes / ku / 1e3, 1), 'copy_us': round(cu, 1),
            'copy_gb_per_s': round(nbytes / cu / 1e3, 1), 'share_of_copy_rate': round(cu / ku, 3)}


def bench_kernels(args):
    dt, code, p, st = torch.bfloat16, _lib.BF16, ops._p, ops._stream
    lib = _lib.load()
    B, S, it, E = args.batch, args.size, args.iters, 2
    rows = []
    f32 = dict(dtype=torch.float32, device=DEV)
    # ---- the stem: patches, GEMM forward, weight gradient
    OH = (S - 1) // 2 + 1
    M, Kp = B * OH * OH, lib.fva_stem7_kp(code, 3)
    img = torch.randn(B, 3, S, S, device=DEV)
    P = torch.empty((M, Kp), dtype=dt, device=DEV)
    patches = lambda: _lib.call('fva_stem7_patches', code, p(img), p(P), B, 3, S, S, st())
    rows.append(with_copy('fva_stem7_patches', patches, img.numel() * 4 + P.numel() * E, it, (B, 3, S, S)))
    d = _lib.ConvDesc(code, B, OH, OH, Kp, 64, 1, 1, 0, 1)
    wf, _ = ops.packed_weights(torch.randn(64, Kp, 1, 1, device=DEV), d, dt, cache=False)
    y = torch.empty((M, 64), dtype=dt, device=DEV)
    nblk = lib.fva_conv_stat_blocks(C.byref(d))
    stats = torch.empty((lib.fva_bn_partial_rows(nblk), 2, 64), **f32)
    gemm = lambda: _lib.call('fva_conv_fwd', C.byref(d), p(P), p(wf), p(y), p(stats), st())
    dy = torch.zeros((B, OH + 2, OH + 2, 64), dtype=dt, device=DEV)
    dw = torch.empty((64, Kp), **f32)
    wsb = lib.fva_conv_wgrad_workspace(C.byref(d))
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=DEV)
    wgrad = lambda: _lib.call('fva_conv_wgrad', C.byref(d), p(P), p(dy), p(dw), 0, p(ws), wsb, st())
    stem = {'patches_us': rows[-1]['us'], 'gemm_fwd_us': round(event_us(gemm, it), 1), 'wgrad_us': round(event_us(wgrad, it), 1),
            'patch_matrix_mb': round(P.numel() * E / 1e6, 1)}
    stem['total_us'] = round(stem['patches_us'] + stem['gemm_fwd_us'] + stem['wgrad_us'], 1)
    del img, P, y, dy
    # ---- MaxPool2d(3, 2, 1) on the stem's output
    H, Cc = OH, 64
    PH = (H - 1) // 2 + 1
    x = torch.randn(B, H + 2, H + 2, Cc, device=DEV).to(dt)
    o = torch.empty((B, PH + 2, PH + 2, Cc), dtype=dt, device=DEV)
    rows.append(with_copy('fva_maxpool3s2_fwd', lambda: _lib.call('fva_maxpool3s2_fwd', code, p(x), 1, p(o), 1, B, H, H, Cc, st()),
                          (B * H * H + B * PH * PH) * Cc * E, it, (B, H, H, Cc)))
    dz = torch.randn(B, PH, PH, Cc, device=DEV).to(dt)
    dx = torch.empty((B, H, H, Cc), dtype=dt, device=DEV)
    rows.append(with_copy('fva_maxpool3s2_bwd', lambda: _lib.call('fva_maxpool3s2_bwd', code, p(dz), p(x), 1, p(dx), B, H, H, Cc, st()),
                          (2 * B * H * H + B * PH * PH) * Cc * E, it, (B, H, H, Cc)))
    del x, o, dz, dx
    # ---- the even-pixel subsample in front of res3's shortcut (resnet50: 256 channels at S / 4)
    H, Cc = S // 4, 256
    x = torch.randn(B, H + 2, H + 2, Cc, device=DEV).to(dt)
    xs = torch.empty((B, H // 2, H // 2, Cc), dtype=dt, device=DEV)
    dx = torch.empty((B, H, H, Cc), dtype=dt, device=DEV)
    rows.append(with_copy('fva_subsample2_fwd', lambda: _lib.call('fva_subsample2_fwd', code, p(x), 1, p(xs), B, H, H, Cc, st()),
                          2 * xs.numel() * E, it, (B, H, H, Cc)))
    rows.append(with_copy('fva_subsample2_bwd', lambda: _lib.call('fva_subsample2_bwd', code, p(xs), p(dx), B, H, H, Cc, st()),
                          (xs.numel() + dx.numel()) * E, it, (B, H, H, Cc)))
    del x, xs, dx
    # ---- BatchNorm + add + ReLU: the identity form at res2 of resnet50, the shortcut form at res3.0
    for form2, H, Cc in ((False, S // 4, 256), (True, S // 8, 512), (False, S // 32, 2048)):
        M = B * H * H
        n = M * Cc
        yv, dzv = torch.randn(M, Cc, device=DEV).to(dt), torch.randn(M, Cc, device=DEV).to(dt)
        q = torch.randn(M, Cc, device=DEV).to(dt) if form2 else torch.randn(B, H + 2, H + 2, Cc, device=DEV).to(dt)
        v = [torch.rand(Cc, **f32) + 0.5 for _ in range(8)]
        z = torch.empty((B, H + 2, H + 2, Cc), dtype=dt, device=DEV)
        z2, dr = torch.empty_like(z), torch.empty((M, Cc), dtype=dt, device=DEV)
        none = C.c_void_p(0)
        sec = (none, 0, p(q), p(v[4]), p(v[5])) if form2 else (p(q), 1, none, none, none)
        secb = (none, 0, p(q), p(v[4]), p(v[5]), p(v[6]), p(v[7])) if form2 else (p(q), 1, none, none, none, none, none)
        main = (code, p(dzv), p(yv), p(v[0]), p(v[1]), p(v[2]), p(v[3]))
        nb = lib.fva_bn_add_relu_bwd_blocks(code, M, Cc)
        part, part_d = torch.empty((lib.fva_bn_partial_rows(nb), 2, Cc), **f32), torch.empty((lib.fva_bn_partial_rows(nb), 2, Cc), **f32)
        coef = torch.rand(3, Cc, **f32)
        tag = ' (shortcut form)' if form2 else ' (identity form)'
        rows.append(with_copy('fva_bn_add_relu_apply' + tag, lambda: _lib.call('fva_bn_add_relu_apply', code, p(yv), p(v[0]), p(v[1]), *sec, p(z), 1, B, H, H,
                                                                               Cc, st()), 3 * n * E, it, (B, H, H, Cc)))
        rows.append(with_copy('fva_bn_add_relu_bwd_reduce' + tag, lambda: _lib.call('fva_bn_add_relu_bwd_reduce', *main, *secb, p(part),
                                                                                    p(part_d) if form2 else none, nb, B, H, H, Cc, st()),
                              3 * n * E, it, (B, H, H, Cc)))
        rows.append(with_copy('fva_bn_add_relu_bwd_apply' + tag, lambda: _lib.call('fva_bn_add_relu_bwd_apply', *main, p(coef), *secb,
                                                                                   p(coef) if form2 else none, p(z), p(z2) if form2 else none, 1,
                                                                                   none if form2 else p(dr), B, H, H, Cc, st()),
                              5 * n * E, it, (B, H, H, Cc)))
        del yv, dzv, q, z, z2, dr
    return rows, stem


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--size', type=int, default=224)
    ap.add_argument('--models', default='resnet50,resnet18')
    ap.add_argument('--modes', default='eager,torch')
    ap.add_argument('--no-kernels', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_resnet: no GPU -- nothing to measure here')
    gen = torch.Generator().manual_seed(0)
    images = torch.randn(args.batch, 3, args.size, args.size, generator=gen).to(DEV)
    labels = torch.randint(0, NUM_CLASSES, (args.batch,), generator=gen).to(DEV)
    out = {'workload': f'ResNet classification train step B={args.batch} 3x{args.size}x{args.size} {NUM_CLASSES} classes bf16, SGD nesterov',
           'steps': args.steps, 'warmup': args.warmup, 'rounds': args.rounds, 'device': torch.cuda.get_device_name(0),
           'reference': 'torch: the same network from stock torch.nn on the same device, bf16 autocast, channels_last, torch.optim.SGD'}
    with fastvision_amd.compute_dtype(torch.bfloat16):
        out.update(bench_models(args, images, labels))
        if not args.no_kernels:
            rows, stem = bench_kernels(args)
            out['kernels'] = rows
            out['kernels_measured_against'] = 'a device-to-device copy of the same number of bytes (half read, half written), same process'
            for name in args.models.split(','):
                if 'eager' in out.get(name, {}):
                    stem[f'share_of_{name}_eager_step'] = round(stem['total_us'] / 1e3 / out[name]['eager']['ms_per_step'], 4)
            out['stem_three_launches'] = stem
    print(json.dumps(out))


if __name__ == '__main__':
    main()
