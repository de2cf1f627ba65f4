#!/usr/bin/env python3
"""Darknet-53 classification train step (the pre-training of the detector's backbone_weights): B=128, 3 x 224 x 224, 1000 classes,
bf16 compute; forward, CrossEntropyLoss, backward, FusedSGD(momentum=0.9, nesterov=True, weight_decay=5e-4), and (eager modes)
top-1 accuracy of the batch.

Modes (each on a fresh, identically seeded model; wall time over --steps steps after --warmup, device synchronised at both ends):
    eager     the library step: classifier top on fva_gap_fwd / fc_ops.linear, loss on fva_softmax_ce, metrics.Accuracy
    graphed   the train step (no metric) captured once by graphs.GraphedTrainStep and replayed, labels as a float [N, 1] target buffer
    aten_top  A/B leg built here, not in the product: darknet53(including_top=False) + torch's adaptive_avg_pool2d / nn.Linear on the
              fp32 copy of res5 + the reference's CrossEntropyLoss and accuracy expressions (log_softmax, one-hot scatter_, argmax), eager
Prints one JSON line: img/s and ms/step per mode.  --modes picks a subset (e.g. `--modes eager` for a kernel trace of a few steps).

usage: python tools/bench_classify.py [--steps K] [--warmup W] [--batch B] [--size S] [--modes eager,graphed,aten_top]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn as nn
import torch.nn.functional as F

import fastvision_amd
from fastvision_amd import FusedSGD
from fastvision_amd.classfication.models import darknet53
from fastvision_amd.loss import CrossEntropyLoss
from fastvision_amd.metrics import Accuracy

DEV = 'cuda:0'
NUM_CLASSES = 1000
SGD_KW = dict(lr=0.01, momentum=0.9, nesterov=True, weight_decay=5e-4)


def batch(B, S):
    g = torch.Generator().manual_seed(0)
    images = torch.randn(B, 3, S, S, generator=g).to(DEV)
    labels = torch.randint(0, NUM_CLASSES, (B,), generator=g).to(DEV)
    return images, labels


class AtenTop(nn.Module):
    """The classifier top as the repository had it before the HIP top: backbone without top, torch ops on the fp32 copy of res5."""

    def __init__(self):
        super().__init__()
        torch.manual_seed(0)
        self.backbone = darknet53(num_classes=NUM_CLASSES, including_top=False)
        self.fc = nn.Linear(1024, NUM_CLASSES)

    def forward(self, x):
        res5 = self.backbone(x)[0]
        return self.fc(torch.flatten(F.adaptive_avg_pool2d(res5.float(), (1, 1)), 1))


def aten_ce(z, y):                      # loss/classification_loss.py:8-33 of the reference, torch ops
    onehot = torch.zeros_like(z).scatter_(1, y.view(-1, 1), 1)
    return torch.mean(-torch.sum(onehot * F.log_softmax(z, dim=-1), dim=1))


def aten_accuracy(z, y):                # metrics/accuracy.py of the reference, torch ops
    pred = torch.argmax(z, dim=1)
    return pred.eq(y.expand_as(pred)).float().sum(0, keepdim=True) / pred.size(0)


def make(mode):
    if mode == 'aten_top':
        net = AtenTop().to(DEV).train()
        crit = aten_ce
    else:
        torch.manual_seed(0)
        net = darknet53(num_classes=NUM_CLASSES).to(DEV).train()
        crit = CrossEntropyLoss()
    opt = FusedSGD(net.parameters(), capturable=(mode == 'graphed'), **SGD_KW)
    return net, crit, opt, (aten_accuracy if mode == 'aten_top' else Accuracy())


def eager_step(net, crit, opt, metric, images, labels):
    pred = net(images)
    opt.zero_grad(set_to_none=True)
    loss = crit(pred, labels)
    loss.backward()
    opt.step()
    with torch.no_grad():
        metric(pred.detach(), labels)
    return loss.detach()


def run(mode, images, labels, steps, warmup):
    net, crit, opt, metric = make(mode)
    if mode == 'graphed':
        from fastvision_amd.graphs import GraphedTrainStep
        target = labels.float().view(-1, 1)
        step = GraphedTrainStep(net, lambda p, t: crit(p, t), opt, images, target)
        fn = lambda: step()                                             # the captured buffers already hold this batch
    else:
        fn = lambda: eager_step(net, crit, opt, metric, images, labels)
    for _ in range(warmup):
        loss = fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = fn()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    out = {'ms_per_step': round(ms, 3), 'img_per_s': round(images.shape[0] * 1e3 / ms, 1), 'last_loss': round(float(loss), 5)}
    del net, crit, opt, metric, fn
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--size', type=int, default=224)
    ap.add_argument('--modes', default='eager,graphed,aten_top')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_classify needs a GPU'
    images, labels = batch(a.batch, a.size)
    res = {'workload': f'darknet53 classification train step B={a.batch} 3x{a.size}x{a.size} {NUM_CLASSES} classes bf16, FusedSGD nesterov',
           'steps': a.steps, 'warmup': a.warmup, 'device': torch.cuda.get_device_name(0)}
    with fastvision_amd.compute_dtype(torch.bfloat16):
        for mode in a.modes.split(','):
            res[mode] = run(mode, images, labels, a.steps, a.warmup)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
