#!/usr/bin/env python3
"""The one-pass BatchNorm backward with frozen statistics (fva_bn_silu_frozen_bwd / fva_bn_relu_frozen_bwd), measured.

  * the kernel, bf16, at the BatchNorm layer shapes of the YOLOv3 step on 32 x 3 x 640^2 (SiLU) and at the five stage shapes of vgg16_bn
    on 64 x 3 x 224^2 (ReLU): the pass with its sums and table fold, the pass without sums, a device copy of the same 6 M C bytes, and the
    training-mode pair on the same tensors (reduce + finalize + apply) with its apply pass alone beside it.  The variants alternate in one
    process; the figure is the median of the rounds, the spread (max - min) / median stands beside it.
  * the bytes of the partial table (written once, read once) as a share of the pass's own 6 M C bytes, counted from the shapes.
  * the YOLOv3 train step at 32 x 3 x 640^2 bf16 with every BatchNorm frozen against the training-mode step of the same build, alternating.

usage: python tools/bench_frozen_bn.py [--rounds 3] [--steps 10] [--warmup 3] [--no-step] [--out profiles/bench_frozen_bn.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import fastvision_amd  # noqa: E402
from fastvision_amd import _lib, ops  # noqa: E402

DEV = 'cuda:0'
#         C     H     the BatchNorm layers of YOLOv3 (Darknet-53, neck) at 640^2
YOLO = [(32, 640), (64, 320), (32, 320), (128, 160), (64, 160), (256, 80), (128, 80), (512, 40), (256, 40), (1024, 20), (512, 20)]
VGG = [(64, 224), (128, 112), (256, 56), (512, 28), (512, 14)]


def time_us(fn, reps=10, warm=2):
    for _ in range(warm):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) * 1e3 / reps


def table_share(code, B, H, Cc):
    nb = _lib.load().fva_bn_frozen_bwd_blocks(code, B, H, H, Cc, 1)
    return nb, 2 * nb * 2 * Cc * 4 / (B * H * H * Cc * 6)


def bench_shape(act, B, Cc, H, rounds, dt=torch.bfloat16):
    lib, code, p, st = _lib.load(), ops._code(dt), ops._p, ops._stream
    M = B * H * H
    g = torch.Generator().manual_seed(Cc + H)
    y = (torch.randn(M, Cc, generator=g) * 1.5).to(dt).to(DEV)
    dz = torch.randn(M, Cc, generator=g).to(dt).to(DEV)
    scale, shift = (torch.rand(Cc, generator=g) + 0.5).to(DEV), (0.5 * torch.randn(Cc, generator=g)).to(DEV)
    mean, rstd = (0.3 * torch.randn(Cc, generator=g)).to(DEV), (torch.rand(Cc, generator=g) + 0.5).to(DEV)
    gamma = torch.ones(Cc, device=DEV)
    dy = torch.empty((B, H + 2, H + 2, Cc), dtype=dt, device=DEV)
    nbf = lib.fva_bn_frozen_bwd_blocks(code, B, H, H, Cc, 1)
    partf = torch.empty((lib.fva_bn_partial_rows(nbf), 2, Cc), dtype=torch.float32, device=DEV)
    nbt = lib.fva_bn_bwd_blocks(code, M, Cc)
    partt = torch.empty((lib.fva_bn_partial_rows(nbt), 2, Cc), dtype=torch.float32, device=DEV)
    coef = torch.empty((3, Cc), dtype=torch.float32, device=DEV)
    dg, db = torch.empty(Cc, device=DEV), torch.empty(Cc, device=DEV)
    src, dst = torch.empty(3 * M * Cc // 2, dtype=dt, device=DEV), torch.empty(3 * M * Cc // 2, dtype=dt, device=DEV)     # 3 M C bytes read + 3 M C written

    def frozen():
        _lib.call(f'fva_bn_{act}_frozen_bwd', code, p(dz), p(y), p(scale), p(shift), p(mean), p(rstd), p(partf), p(dy), 1, B, H, H, Cc, st())
        _lib.call('fva_bn_frozen_bwd_finalize', p(partf), nbf, partf.shape[0], Cc, p(scale), p(dg), p(db), None, st())

    def frozen_no_sums():
        _lib.call(f'fva_bn_{act}_frozen_bwd', code, p(dz), p(y), p(scale), p(shift), None, None, None, p(dy), 1, B, H, H, Cc, st())

    def apply():
        _lib.call(f'fva_bn_{act}_bwd_apply', code, p(dz), p(y), p(scale), p(shift), p(mean), p(rstd), p(coef), p(dy), 1, B, H, H, Cc, st())

    def pair():
        _lib.call(f'fva_bn_{act}_bwd_reduce', code, p(dz), p(y), p(scale), p(shift), p(mean), p(rstd), p(partt), nbt, M, Cc, st())
        _lib.call('fva_bn_bwd_finalize', p(partt), nbt, partt.shape[0], M, Cc, p(gamma), p(rstd), p(dg), p(db), 0, p(coef), st())
        apply()
    pair()
    variants = {'copy': lambda: dst.copy_(src), 'frozen': frozen, 'frozen_no_sums': frozen_no_sums, 'train_apply': apply, 'train_pair': pair}
    us = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            us[k].append(time_us(fn))
    row = {'shape': [B, H, H, Cc], 'act': act, 'pass_MB': round(6 * M * Cc / 1e6, 1), 'blocks': nbf, 'table_share': round(table_share(code, B, H, Cc)[1], 5)}
    for k, v in us.items():
        med = statistics.median(v)
        row[k] = {'us': round(med, 1), 'spread': round((max(v) - min(v)) / med, 3)}
    row['frozen_TBps'] = round(6 * M * Cc / row['frozen']['us'] / 1e6, 2)
    row['frozen_share_of_copy_rate'] = round(row['copy']['us'] / row['frozen']['us'], 3)
    row['frozen_over_train_apply'] = round(row['frozen']['us'] / row['train_apply']['us'], 3)
    row['frozen_over_train_pair'] = round(row['frozen']['us'] / row['train_pair']['us'], 3)
    return row


def bench_step(batch, size, steps, warmup, rounds):
    from fastvision_amd import FusedAdam
    from fastvision_amd.classfication.models import darknet53
    from fastvision_amd.detection.head import yolov3head
    from fastvision_amd.detection.models import yolov3
    from fastvision_amd.detection.neck import yolov3neck
    from fastvision_amd.loss import Yolov3Loss
    from fastvision_amd.synthetic import coco_anchors_px, synthetic_batch
    from fastvision_amd.utils import freeze_batchnorm, unfreeze_batchnorm
    torch.manual_seed(20220504)
    net = yolov3(backbone=darknet53, neck=yolov3neck, head=yolov3head, anchors=coco_anchors_px(), num_anchors_per_level=[3, 3, 3],
                 in_channels=3, num_classes=80, training=True).to(DEV).train()
    crit = Yolov3Loss(net, 0.5, 0.05, 1.0, 0.5)
    opt = FusedAdam(net.parameters(), lr=1e-5, betas=(0.937, 0.999), weight_decay=5e-4)
    images, tg = synthetic_batch(batch, size)
    images, tg = images.to(DEV), tg.to(DEV)

    def step():
        pred = net(images)
        opt.zero_grad()
        loss = crit(pred, tg)
        loss.backward()
        opt.step()
        return loss

    def window():
        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(steps):
            loss = step()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / steps, float(loss.detach())
    ms = {'training': [], 'frozen': []}
    last = {}
    for _ in range(rounds):
        unfreeze_batchnorm(net)
        net.train()
        t, last['training'] = window()          # (these steps also move the running statistics towards the batch: healthy ones to freeze)
        ms['training'].append(t)
        freeze_batchnorm(net)
        net.train()
        t, last['frozen'] = window()
        ms['frozen'].append(t)
    out = {'workload': f'YOLOv3 train step B={batch} 3x{size}x{size} bf16, eager, FusedAdam', 'steps': steps, 'warmup': warmup, 'rounds': rounds}
    for k, v in ms.items():
        med = statistics.median(v)
        out[k] = {'ms_per_step': round(med, 3), 'img_per_s': round(batch * 1e3 / med, 1), 'spread': round((max(v) - min(v)) / med, 4), 'last_loss': last[k]}
    out['frozen_over_training'] = round(out['frozen']['ms_per_step'] / out['training']['ms_per_step'], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--no-step', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bench_frozen_bn.json'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_frozen_bn needs a GPU'
    res = {'device': torch.cuda.get_device_name(0), 'dtype': 'bf16', 'rounds': a.rounds,
           'note': 'us: median of the rounds; spread: (max - min) / median; table_share: partial-table bytes written + read / (6 M C), counted from shapes'}
    res['yolov3_32x640'] = [bench_shape('silu', 32, Cc, H, a.rounds) for Cc, H in YOLO]
    res['vgg16_bn_64x224'] = [bench_shape('relu', 64, Cc, H, a.rounds) for Cc, H in VGG]
    for key in ('yolov3_32x640', 'vgg16_bn_64x224'):
        rows = res[key]
        res[key + '_sum_us'] = {k: round(sum(r[k]['us'] for r in rows), 1) for k in ('copy', 'frozen', 'frozen_no_sums', 'train_apply', 'train_pair')}
        for r in rows:
            print(f"{r['act']} C={r['shape'][3]:4d} @{r['shape'][1]:3d}: frozen {r['frozen']['us']:7.1f} us ({r['frozen_TBps']:.2f} TB/s, {r['frozen_share_of_copy_rate']:.2f} of copy, "
                  f"spread {r['frozen']['spread']:.3f}) no sums {r['frozen_no_sums']['us']:7.1f} | train apply {r['train_apply']['us']:7.1f} pair {r['train_pair']['us']:7.1f} | "
                  f"copy {r['copy']['us']:7.1f} | table {100 * r['table_share']:.2f} %", flush=True)
        print(key, 'sum us', res[key + '_sum_us'], flush=True)
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
