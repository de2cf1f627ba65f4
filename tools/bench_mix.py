#!/usr/bin/env python3
"""What label smoothing + MixUp / CutMix cost on the device: the resnet50 train step (B=128, 3 x 224 x 224, 1000 classes, bf16 compute;
forward, CrossEntropyLoss, backward, FusedSGD nesterov), eager,

    plain     the step of tools/bench_resnet.py
    mix       the same step behind BatchMix (fva_mix_plan + fva_mix_apply on the fp32 batch) with CrossEntropyLoss(label_smoothing=0.1)
              reading lambda from the plan on the device (fva_softmax_ce_soft)

ALTERNATING in one process, --rounds times each after warm-up; the figure per mode is the median of its rounds, the spread
(max - min) / median beside it (the method of tools/bench_resnet.py).

Alone, by device events over --iters launches after warm-up, each beside a device-to-device copy of the same number of bytes measured in
the same process (alternating twice, the better of each):
    fva_mix_apply        per mode (0 copy, 1 MixUp, 2 CutMix with a half-image box), fp32 and bf16; bytes = what the mode must move
    fva_softmax_ce_soft  128 x 1000 logits, pair form with smoothing, value + gradient (latency-bound: 1 MB)
    fva_mix_plan         the one-thread tick
    ATen                 the sequence a user would otherwise write: images.roll(1, 0).mul_(1 - lam).add_(images * lam) and
                         F.cross_entropy(label_smoothing=0.1) on the two label sets, value and gradient

Prints one JSON line.  usage: python tools/bench_mix.py [--steps K] [--warmup W] [--rounds R] [--iters N] [--batch B] [--size S] [--no-model]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

import fastvision_amd
from fastvision_amd import BatchMix, FusedSGD, MixedLabels, _lib, ops
from fastvision_amd.classfication import models
from fastvision_amd.loss import CrossEntropyLoss

DEV = 'cuda:0'
NUM_CLASSES = 1000
SGD_KW = dict(lr=0.01, momentum=0.9, nesterov=True, weight_decay=5e-4)


def make_step(mixed, images, labels):
    torch.manual_seed(0)
    net = models.resnet50(num_classes=NUM_CLASSES).to(DEV).train()
    opt = FusedSGD(net.parameters(), capturable=True, **SGD_KW)
    crit = CrossEntropyLoss(label_smoothing=0.1 if mixed else 0.0)
    mix = BatchMix(seed=1).to(DEV) if mixed else None

    def step():
        x, y = (images, labels) if mix is None else mix(images, labels)
        pred = net(x)
        opt.zero_grad(set_to_none=True)
        loss = crit(pred, y)
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


def bench_model(args, images, labels):
    steps = {'plain': make_step(False, images, labels), 'mix': make_step(True, images, labels)}
    for st in steps.values():
        for _ in range(args.warmup):
            st()
    torch.cuda.synchronize()
    runs, last = {m: [] for m in steps}, {}
    for _ in range(args.rounds):
        for m, st in steps.items():
            ms, last[m] = timed(st, args.steps)
            runs[m].append(ms)
    out = {m: {'ms_per_step': round(statistics.median(v), 3), 'img_per_s': round(args.batch / statistics.median(v) * 1e3, 1),
               'spread': round((max(v) - min(v)) / statistics.median(v), 4), 'last_loss': round(last[m], 5)} for m, v in runs.items()}
    out['mix_over_plain'] = round(out['mix']['ms_per_step'] / out['plain']['ms_per_step'], 4)
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


def with_copy(name, fn, nbytes, iters, note=''):
    """the kernel and a device copy of the same bytes (half read, half written), alternating twice; the better of each"""
    src = torch.empty(max(nbytes // 2, 16), dtype=torch.uint8, device=DEV)
    dst = torch.empty_like(src)
    k, c = [], []
    for _ in range(2):
        k.append(event_us(fn, iters))
        c.append(event_us(lambda: dst.copy_(src), iters))
    ku, cu = min(k), min(c)
    return {'kernel': name, 'note': note, 'bytes': nbytes, 'us': round(ku, 1), 'gb_per_s': round(nbytes / ku / 1e3, 1), 'copy_us': round(cu, 1),
            'copy_gb_per_s': round(nbytes / cu / 1e3, 1), 'share_of_copy_rate': round(cu / ku, 3)}


def plan_tensor(mode, lam, box=(0, 0, 0, 0)):
    t = torch.zeros(9, dtype=torch.int32)
    t[0] = mode
    t[1:3] = torch.tensor([lam, lam], dtype=torch.float32).view(torch.int32)
    t[5:9] = torch.tensor(box, dtype=torch.int32)
    return t.to(DEV)


def bench_kernels(args):
    p, st = ops._p, ops._stream
    B, S, it = args.batch, args.size, args.iters
    rows = []
    half = int(S * 0.5 ** 0.5 / 2)                           # lam_raw = 0.5: r = 0.5 * sqrt(0.5), a centred box of half the pixels
    box = (S // 2 - half, S // 2 - half, S // 2 + half, S // 2 + half)
    frac = (box[2] - box[0]) * (box[3] - box[1]) / (S * S)
    for dt, code, E in ((torch.float32, _lib.F32, 4), (torch.bfloat16, _lib.BF16, 2)):
        x = torch.randn(B, 3, S, S, device=DEV).to(dt)
        out = torch.empty_like(x)
        n = x.numel()
        for mode, plan, moved, note in ((0, plan_tensor(0, 1.0), 2 * n, 'copy'), (1, plan_tensor(1, 0.3), 3 * n, 'MixUp: two images read per image written'),
                                        (2, plan_tensor(2, 0.5, box), int((2 + frac) * n), f'CutMix, box {box}: the partner is read inside the box only')):
            fn = lambda plan=plan: _lib.call('fva_mix_apply', code, p(x), p(out), p(plan), B, 3, S, S, st())
            rows.append(with_copy(f'fva_mix_apply mode {mode} {str(dt).split(".")[1]}', fn, moved * E, it, note))
        if dt == torch.float32:
            lam = 0.3
            aten = lambda: x.roll(1, 0).mul_(1 - lam).add_(x * lam)
            rows.append(with_copy('ATen roll / mul_ / add_ float32 (MixUp)', aten, 3 * n * E, it, 'bytes as fva_mix_apply mode 1; ATen moves more'))
        del x, out
    R, Cc = B, NUM_CLASSES
    z = torch.randn(R, Cc, device=DEV)
    y = torch.randint(0, Cc, (R,), device=DEV)
    grad, loss = torch.empty_like(z), torch.empty(1, device=DEV)
    ws = torch.empty(max(_lib.load().fva_softmax_ce_workspace(R), 4), dtype=torch.uint8, device=DEV)
    plan = plan_tensor(1, 0.3)
    soft = lambda: _lib.call('fva_softmax_ce_soft', p(z), p(y), _lib.LABEL_I64, None, None, R, Cc, _lib.REDUCE_MEAN, 0.1, p(plan), p(loss), p(grad), p(ws), st())
    hard = lambda: _lib.call('fva_softmax_ce', p(z), p(y), _lib.LABEL_I64, None, R, Cc, _lib.REDUCE_MEAN, p(loss), p(grad), p(ws), st())
    rows.append(with_copy('fva_softmax_ce_soft (pair form, smoothing 0.1, value + gradient; two launches)', soft, 2 * z.numel() * 4, it, 'latency-bound'))
    rows.append(with_copy('fva_softmax_ce (hard labels; two launches)', hard, 2 * z.numel() * 4, it, 'latency-bound'))
    zl = z.clone().requires_grad_(True)
    y2 = y.roll(1, 0)

    def aten_ce():
        zl.grad = None
        (0.3 * F.cross_entropy(zl, y, label_smoothing=0.1) + 0.7 * F.cross_entropy(zl, y2, label_smoothing=0.1)).backward()
    rows.append(with_copy('ATen F.cross_entropy(label_smoothing=0.1) on both label sets + backward', aten_ce, 2 * z.numel() * 4, it, 'latency-bound'))
    state = torch.tensor([1, 0, 0, 0], dtype=torch.int64, device=DEV)
    pl = torch.zeros(9, dtype=torch.int32, device=DEV)
    tick = lambda: _lib.call('fva_mix_plan', p(state), 0.2, 1.0, 1.0, 0.5, S, S, p(pl), st())
    rows.append({'kernel': 'fva_mix_plan (one thread)', 'us': round(min(event_us(tick, it), event_us(tick, it)), 1)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--size', type=int, default=224)
    ap.add_argument('--no-model', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_mix: no GPU -- nothing to measure here')
    gen = torch.Generator().manual_seed(0)
    images = torch.randn(args.batch, 3, args.size, args.size, generator=gen).to(DEV)
    labels = torch.randint(0, NUM_CLASSES, (args.batch,), generator=gen).to(DEV)
    out = {'workload': f'resnet50 train step B={args.batch} 3x{args.size}x{args.size} {NUM_CLASSES} classes bf16, SGD nesterov, eager; '
                       'mix = BatchMix(0.2, 1.0) + label smoothing 0.1',
           'steps': args.steps, 'warmup': args.warmup, 'rounds': args.rounds, 'iters': args.iters, 'device': torch.cuda.get_device_name(0)}
    with fastvision_amd.compute_dtype(torch.bfloat16):
        if not args.no_model:
            out['resnet50'] = bench_model(args, images, labels)
        out['kernels'] = bench_kernels(args)
        out['kernels_measured_against'] = 'a device-to-device copy of the same number of bytes (half read, half written), same process'
    print(json.dumps(out))


if __name__ == '__main__':
    main()
