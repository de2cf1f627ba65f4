#!/usr/bin/env python3
"""FusedSGD against the Faster R-CNN demo's optimizer step (cfg/_fit.py: clip_gradient at 10, then torch.optim.SGD(momentum=0.937,
nesterov=True)) on the parameters of BASELINE config 5's model (VGG16 + RPN + Fast head, 20 classes: ~137 M fp32, mostly fc6).

Isolated launches: fixed random gradients (global norm above 10, so the clip scales), each optimizer step timed alone between device
synchronisations with HIP events (gradients restored before every timed call, untimed), median of --iters calls.  Bytes are counted
against the fused floor: 24 B per parameter (one read of g for the norm; p, g, buffer read and p, buffer written by the update), 20 B
for the update pass alone.  With --step, also the whole config-5 training step (4 x 3 x 800 x 1333, bf16 compute, the loop of
tools/bench_faster.py) with each optimizer.  Prints one JSON line.

--fused-only skips the torch paths (for a kernel trace of FusedSGD alone).

usage: python tools/bench_sgd.py [--iters N] [--step] [--steps K] [--warmup W] [--fused-only]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import fastvision_amd
from fastvision_amd import FusedSGD
from fastvision_amd.demos.faster_rcnn.cfg._fit import clip_gradient
from fastvision_amd.demos.faster_rcnn.models import Faster_Rcnn

DEV = 'cuda:0'
HBM_GBS = 6300.0          # measured float4-copy ceiling of the MI355X (MI355X_MICROARCH: 6.29 TB/s)
SGD_KW = dict(lr=1e-3, momentum=0.937, nesterov=True)       # demos/faster_rcnn/train.py:102


def cfg5_model(NC=20):
    torch.manual_seed(0)
    scales, ratios = [128, 256, 512], [0.5, 1, 2]
    base = torch.tensor([[(s * s / r) ** 0.5, s * s / (s * s / r) ** 0.5] for r in ratios for s in scales], dtype=torch.float32)
    return Faster_Rcnn(training=True, num_classes=NC, base_anchors=base).to(DEV)


def time_isolated(model, grads, fn, iters):
    ms = []
    for i in range(iters + 2):
        for p, g in zip(model.parameters(), grads):
            p.grad.copy_(g)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= 2:                      # two warm-up calls: tables, buffers, code objects
            ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def isolated(iters, fused_only=False):
    model = cfg5_model()
    params = list(model.parameters())
    n = sum(p.numel() for p in params)
    g = torch.Generator(device=DEV).manual_seed(1)
    grads = [torch.randn(p.shape, device=DEV, generator=g) * 1e-2 for p in params]
    for p in params:
        p.grad = torch.empty_like(p)
    norm = torch.linalg.vector_norm(torch.stack([x.double().norm() for x in grads])).item()
    out = {'params': n, 'tensors': len(params), 'grad_norm': round(norm, 3)}
    ref = torch.optim.SGD(params, **SGD_KW)

    def torch_step():
        clip_gradient(model, 10.)
        ref.step()
    if not fused_only:
        out['torch_clip_sgd_ms'] = round(time_isolated(model, grads, torch_step, iters), 4)
    fused = FusedSGD(params, clip_norm=10., **SGD_KW)
    out['fused_clip_sgd_ms'] = round(time_isolated(model, grads, fused.step, iters), 4)
    upd = FusedSGD(params, **SGD_KW)
    out['fused_update_only_ms'] = round(time_isolated(model, grads, upd.step, iters), 4)
    b24, b20 = 24 * n, 20 * n
    out['floor_bytes'] = b24
    out['floor_ms_at_hbm'] = round(b24 / (HBM_GBS * 1e9) * 1e3, 4)
    out['fused_gbs'] = round(b24 / (out['fused_clip_sgd_ms'] * 1e-3) / 1e9, 1)
    out['update_pass_gbs'] = round(b20 / (out['fused_update_only_ms'] * 1e-3) / 1e9, 1)
    out['update_pass_frac_of_hbm'] = round(out['update_pass_gbs'] / HBM_GBS, 3)
    if not fused_only:
        out['torch_gbs_at_floor_bytes'] = round(b24 / (out['torch_clip_sgd_ms'] * 1e-3) / 1e9, 1)
    del model, params, grads, ref, fused, upd
    torch.cuda.empty_cache()
    return out


def whole_step(fused, steps, warmup):
    B, H, W, NC = 4, 800, 1333, 20
    model = cfg5_model(NC)
    opt = FusedSGD(model.parameters(), clip_norm=10., **SGD_KW) if fused else torch.optim.SGD(model.parameters(), **SGD_KW)
    g = torch.Generator().manual_seed(1)
    images = torch.rand(B, 3, H, W, generator=g).to(DEV)
    T = 28
    tb = torch.sort(torch.cat([torch.arange(B), torch.randint(0, B, (T - B,), generator=g)]))[0].float()
    wh = torch.exp(np.log(0.08) + (np.log(0.6) - np.log(0.08)) * torch.rand(T, 2, generator=g))
    xy = wh / 2 + (1 - wh) * torch.rand(T, 2, generator=g)
    targets = torch.cat([tb[:, None], torch.randint(0, NC, (T, 1), generator=g).float(), xy, wh], 1).to(DEV)

    def step():
        _, a, b, c, d = model(images, targets.clone())
        opt.zero_grad()
        loss = a + b + c + d
        loss.backward()
        if not fused:
            clip_gradient(model, 10.)
        opt.step()
        return loss
    with fastvision_amd.compute_dtype(torch.bfloat16):
        for _ in range(max(1, warmup)):
            loss = step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            loss = step()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / steps * 1e3
    out = (round(ms, 3), round(float(loss.detach()), 4))
    del model, opt, images
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--step', action='store_true')
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--fused-only', action='store_true')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_sgd needs a GPU'
    out = {'metric': 'optimizer step ms, Faster R-CNN config-5 parameters (clip at 10 + Nesterov SGD)'}
    out.update(isolated(args.iters, args.fused_only))
    if args.step:
        if not args.fused_only:
            out['step_torch_ms'], out['step_torch_loss'] = whole_step(False, args.steps, args.warmup)
        out['step_fused_ms'], out['step_fused_loss'] = whole_step(True, args.steps, args.warmup)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
