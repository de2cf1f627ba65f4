#!/usr/bin/env python3
"""The ship demo's training step (reference demos/yolov3_huaweiShip/train.py + cfg/_fit.py:40-69): YoloV3 + the CIoU ComputeLoss +
Nesterov SGD (momentum 0.937) in the script's three parameter groups (BatchNorm weights, other weights with decay 5e-4, biases), stepped
eagerly and replayed through graphs.GraphedTrainStep at the exact target count, with torch's CosineAnnealingWarmRestarts stepping between
replays (the device-resident learning rate is refreshed before each replay).

Size: the demo's default 32 x 3 x 608 x 608 in bf16 if the convolution entry points accept the 19 / 38 / 76 grids, else 640 x 640; the
result line says which (``size``, ``size_608_refused`` holds the error).  Beside the step, ``fva_demo_ciou_loss`` against ``fva_demo_loss``
on the same heads and targets (value + gradients, HIP events, median).  Prints one JSON line.

usage: python tools/bench_ship.py [--batch B] [--steps K] [--warmup W] [--classes C] [--iters N] [--size S]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import fastvision_amd
from fastvision_amd import FusedSGD
from fastvision_amd.demos.yolov3_huaweiShip.inference import anchor_fn
from fastvision_amd.demos.yolov3_huaweiShip.models import YoloV3
from fastvision_amd.demos.yolov3_huaweiShip.utils import ComputeLoss
from fastvision_amd.demos.yolov3_u.utils import ComputeLoss as FirstDemoLoss
from fastvision_amd.graphs import GraphedTrainStep
from fastvision_amd.synthetic import synthetic_batch

DEV = 'cuda:0'


def three_groups(model):
    """train.py:70-87"""
    g0, g1, g2 = [], [], []
    for v in model.modules():
        if hasattr(v, 'bias') and isinstance(v.bias, torch.nn.Parameter):
            g2.append(v.bias)
        if isinstance(v, torch.nn.BatchNorm2d):
            g0.append(v.weight)
        elif hasattr(v, 'weight') and isinstance(v.weight, torch.nn.Parameter):
            g1.append(v.weight)
    return [{'params': g0}, {'params': g1, 'weight_decay': 5e-4}, {'params': g2}]


def make(classes, init_lr=1e-3, total_epoch=100, warmup_epoch=5, no_aug_epoch=10):
    torch.manual_seed(20220504)
    net = YoloV3(num_classes=classes, anchors=anchor_fn(DEV)).to(DEV).train()
    crit = ComputeLoss()
    opt = FusedSGD(three_groups(net), lr=init_lr, momentum=0.937, nesterov=True, capturable=True)
    sched = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(optimizer=opt, T_0=total_epoch - warmup_epoch - no_aug_epoch, T_mult=2,
                                                                 eta_min=init_lr * 0.01)

    def loss_fn(pred, tg):
        box, cls, conf = crit(pred, tg, net)
        return box + cls + conf
    return net, loss_fn, opt, sched


def batch_of(B, size, classes):
    im, tg = synthetic_batch(B, size, num_classes=classes, seed=7)
    return im.to(DEV), tg.to(DEV)


def pick_size(B, classes, want):
    """608 if one training step runs there, else 640"""
    if want:
        return want, None
    try:
        net, loss_fn, opt, _ = make(classes)
        im, tg = batch_of(B, 608, classes)
        with fastvision_amd.compute_dtype(torch.bfloat16):
            loss_fn(net(im), tg).backward()
        torch.cuda.synchronize()
        return 608, None
    except RuntimeError as e:
        return 640, str(e).splitlines()[0][:200]
    finally:
        torch.cuda.empty_cache()


def time_steps(fn, steps, warmup):
    for _ in range(max(1, warmup)):
        loss = fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3, float(loss.detach().sum())


def step_times(B, size, classes, steps, warmup):
    out = {}
    im, tg = batch_of(B, size, classes)
    with fastvision_amd.compute_dtype(torch.bfloat16):
        net, loss_fn, opt, sched = make(classes)

        def eager():
            pred = net(im)
            opt.zero_grad()
            loss = loss_fn(pred, tg)
            loss.backward()
            opt.step()
            sched.step()
            return loss
        out['eager_ms'], out['eager_loss'] = time_steps(eager, steps, warmup)
        del net, loss_fn, opt, sched
        torch.cuda.empty_cache()
        net, loss_fn, opt, sched = make(classes)
        graph = GraphedTrainStep(net, loss_fn, opt, im, tg)          # the demo loss assigns every row: exact target count

        def replay():
            loss = graph(im, tg)
            sched.step()
            return loss
        out['graphed_ms'], out['graphed_loss'] = time_steps(replay, steps, warmup)
    out['targets'] = int(tg.shape[0])
    out['img_per_s_eager'] = round(B / out['eager_ms'] * 1e3, 1)
    out['img_per_s_graphed'] = round(B / out['graphed_ms'] * 1e3, 1)
    return {k: (round(v, 3) if isinstance(v, float) else v) for k, v in out.items()}


def loss_times(B, size, classes, iters):
    """the two demo losses on the same random heads and targets, value + gradients"""
    g = torch.Generator().manual_seed(3)
    _, tg = batch_of(B, size, classes)
    anchors = anchor_fn(DEV)
    heads = [(torch.randn(B, 3 * (5 + classes), size // s, size // s, generator=g) * 1.5).clamp(-6, 6).to(DEV).requires_grad_(True) for s in (32, 16, 8)]

    class Shell:
        pass
    Shell.anchors = anchors
    res = {}
    for name, crit in (('fva_demo_ciou_loss_ms', ComputeLoss()), ('fva_demo_loss_ms', FirstDemoLoss())):
        ms = []
        for i in range(iters + 2):
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            crit(heads, tg, Shell)
            b.record()
            torch.cuda.synchronize()
            if i >= 2:
                ms.append(a.elapsed_time(b))
        res[name] = round(statistics.median(ms), 4)
    res['loss_cells'] = sum(B * 3 * (size // s) ** 2 for s in (32, 16, 8))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--classes', type=int, default=10)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--size', type=int, default=0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_ship needs a GPU'
    size, refused = pick_size(args.batch, args.classes, args.size)
    out = {'metric': 'ship demo train step ms (YoloV3 + CIoU ComputeLoss + Nesterov FusedSGD in three groups, bf16)', 'batch': args.batch,
           'size': size, 'size_608_refused': refused, 'classes': args.classes}
    out.update(step_times(args.batch, size, args.classes, args.steps, args.warmup))
    out.update(loss_times(args.batch, size, args.classes, args.iters))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
