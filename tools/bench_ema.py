#!/usr/bin/env python3
"""ModelEMA's update (fva_ema_update), measured on the state dict of the library YOLOv3 (about 220 parameters and 220 buffers, 62 M fp32
elements).

  * one update five ways, alternating in one process: the kernel (the bare `fva_ema_update` call on prepared tables: its GPU time is
    the kernel's) and `ModelEMA.update` (the same launch with its host side: the per-tensor pointer check and the version counters;
    issued back to back its "GPU time" is the larger of kernel and host time); the per-tensor loop
    `for k, v in ema_sd.items(): v.mul_(d).add_(model_sd[k], alpha=1 - d)` (floating-point tensors; the others `copy_`); the same with
    `torch._foreach_mul_` / `torch._foreach_add_`; and a device copy that moves the update's 12 B per fp32 element (the update reads 8 and
    writes 4, `copy_` reads 6 and writes 6: the same bytes over the same bus).  Each variant: GPU time per call from
    device events around `reps` calls, host time per call from a host clock around the same calls before the final synchronise.  The
    figure is the median of the rounds; the spread (max - min) / median stands beside it.
  * the YOLOv3 train step at 32 x 3 x 640^2 bf16 (eager, FusedAdam) with and without `ema.update(model)` after the optimizer step,
    alternating.

usage: python tools/bench_ema.py [--rounds 5] [--reps 20] [--steps 10] [--warmup 3] [--no-step] [--out profiles/bench_ema.json]"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import fastvision_amd  # noqa: E402
from fastvision_amd import FusedAdam, ModelEMA, _lib  # noqa: E402
from fastvision_amd.ops import _stream  # noqa: E402

DEV = 'cuda:0'


def lib_model():
    from fastvision_amd.classfication.models import darknet53
    from fastvision_amd.detection.head import yolov3head
    from fastvision_amd.detection.models import yolov3
    from fastvision_amd.detection.neck import yolov3neck
    from fastvision_amd.synthetic import coco_anchors_px
    torch.manual_seed(20220504)
    return yolov3(backbone=darknet53, neck=yolov3neck, head=yolov3head, anchors=coco_anchors_px(), num_anchors_per_level=[3, 3, 3],
                  in_channels=3, num_classes=80, training=True).to(DEV).train()


def time_call(fn, reps, warm=3):
    """(GPU us per call by events, host us per call: the time the calls took to issue)."""
    for _ in range(warm):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    host = time.perf_counter() - t0
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) * 1e3 / reps, host * 1e6 / reps


def summary(rows):
    out = {}
    for k, v in rows.items():
        gpu, host = [a for a, _ in v], [b for _, b in v]
        mg, mh = statistics.median(gpu), statistics.median(host)
        out[k] = {'gpu_us': round(mg, 1), 'gpu_spread': round((max(gpu) - min(gpu)) / mg, 3),
                  'host_us': round(mh, 1), 'host_spread': round((max(host) - min(host)) / mh, 3)}
    return out


def bench_update(rounds, reps):
    net = lib_model()
    ema = ModelEMA(net)
    with torch.no_grad():
        for p in net.parameters():                       # a model that has moved away from its average
            p.add_(0.01 * torch.randn_like(p))
    ema_sd, model_sd = ema.module.state_dict(), net.state_dict()
    fl = [(v, model_sd[k]) for k, v in ema_sd.items() if v.dtype.is_floating_point]
    other = [(v, model_sd[k]) for k, v in ema_sd.items() if not v.dtype.is_floating_point]
    fe, fp = [a for a, _ in fl], [b for _, b in fl]
    elems = sum(v.numel() for v in fe)
    d = 0.9999 * (1 - math.exp(-1 / 2000.0))
    src = torch.empty(3 * elems // 2, dtype=torch.float32, device=DEV).normal_()      # 6 B per element read ...
    dst = torch.empty_like(src)                                                      # ... and 6 B written: 12 B per fp32 element

    def update():
        ema.update(net)

    def kernel():                                        # the bare C call on the tables of the last update: no host work beside it
        _lib.call('fva_ema_update', C.c_void_p(t['tab'].data_ptr()), t['n'], C.c_void_p(t['chunks'].data_ptr()), t['nchunks'], ema.decay, ema.tau,
                  C.c_void_p(ema._state.data_ptr()), _stream())
    update()
    t = ema._tab

    @torch.no_grad()
    def loop():
        for v, m in fl:
            v.mul_(d).add_(m, alpha=1 - d)
        for v, m in other:
            v.copy_(m)

    @torch.no_grad()
    def foreach():
        torch._foreach_mul_(fe, d)
        torch._foreach_add_(fe, fp, alpha=1 - d)
        for v, m in other:
            v.copy_(m)

    def copy():
        dst.copy_(src)
    variants = {'fva_ema_update': kernel, 'ModelEMA.update': update, 'per_tensor_loop': loop, 'foreach': foreach, 'copy_same_bytes': copy}
    rows = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            rows[k].append(time_call(fn, reps))
    out = summary(rows)
    byts = 12 * elems
    res = {'tensors': len(ema_sd), 'fp32_tensors': len(fl), 'other_tensors': len(other), 'fp32_elements': elems, 'MB_moved': round(byts / 1e6, 1),
           'table_rows': ema._tab['n'], 'blocks': ema._tab['nchunks'], 'reps': reps, 'rounds': rounds, **out}
    res['kernel_TBps'] = round(byts / out['fva_ema_update']['gpu_us'] / 1e6, 2)
    res['copy_TBps'] = round(byts / out['copy_same_bytes']['gpu_us'] / 1e6, 2)
    res['kernel_over_copy'] = round(out['fva_ema_update']['gpu_us'] / out['copy_same_bytes']['gpu_us'], 3)
    res['loop_over_kernel_gpu'] = round(out['per_tensor_loop']['gpu_us'] / out['fva_ema_update']['gpu_us'], 2)
    res['foreach_over_kernel_gpu'] = round(out['foreach']['gpu_us'] / out['fva_ema_update']['gpu_us'], 2)
    return res


def bench_step(batch, size, steps, warmup, rounds):
    from fastvision_amd.loss import Yolov3Loss
    from fastvision_amd.synthetic import synthetic_batch
    net = lib_model()
    crit = Yolov3Loss(net, 0.5, 0.05, 1.0, 0.5)
    opt = FusedAdam(net.parameters(), lr=1e-5, betas=(0.937, 0.999), weight_decay=5e-4)
    ema = ModelEMA(net)
    images, tg = synthetic_batch(batch, size)
    images, tg = images.to(DEV), tg.to(DEV)

    def step(with_ema):
        pred = net(images)
        opt.zero_grad()
        loss = crit(pred, tg)
        loss.backward()
        opt.step()
        if with_ema:
            ema.update(net)
        return loss

    def window(with_ema):
        for _ in range(warmup):
            step(with_ema)
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(steps):
            loss = step(with_ema)
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / steps, float(loss.detach())
    ms = {'plain': [], 'with_ema': []}
    last = {}
    for _ in range(rounds):
        for k, flag in (('plain', False), ('with_ema', True)):
            t, last[k] = window(flag)
            ms[k].append(t)
    out = {'workload': f'YOLOv3 train step B={batch} 3x{size}x{size} bf16, eager, FusedAdam', 'steps': steps, 'warmup': warmup, 'rounds': rounds}
    for k, v in ms.items():
        med = statistics.median(v)
        out[k] = {'ms_per_step': round(med, 3), 'img_per_s': round(batch * 1e3 / med, 1), 'spread': round((max(v) - min(v)) / med, 4), 'last_loss': last[k]}
    out['ema_cost_ms'] = round(out['with_ema']['ms_per_step'] - out['plain']['ms_per_step'], 3)
    out['with_ema_over_plain'] = round(out['with_ema']['ms_per_step'] / out['plain']['ms_per_step'], 4)
    out['ema_updates'] = ema.updates
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--no-step', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bench_ema.json'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_ema needs a GPU'
    res = {'device': torch.cuda.get_device_name(0),
           'note': 'gpu_us: device events around reps calls, per call; host_us: host clock around issuing the same calls, per call; median of '
                   'the rounds, spread = (max - min) / median; the variants alternate within each round'}
    res['update'] = bench_update(a.rounds, a.reps)
    print('update', json.dumps(res['update']), flush=True)
    if not a.no_step:
        with fastvision_amd.compute_dtype(torch.bfloat16):
            res['step'] = bench_step(32, 640, a.steps, a.warmup, a.rounds)
        print('step', json.dumps(res['step']), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', a.out)


if __name__ == '__main__':
    main()
