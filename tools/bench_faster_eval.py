#!/usr/bin/env python3
"""Faster R-CNN evaluation, per image against batched: B x 3 x 800 x 1333, bf16 compute, VGG16 backbone, random weights (fixed seed).

    per_image   the reference's shape of the work: ``model(images)`` (Fast.forward's eval branch: heads, decode and background mask image by
                image) and ``inference.postProcess`` (frame change, clamps, size filter, NMS) for every image
    batched     ``model.detect(images, ...)``: one heads pass over every image's RoIs, one fva_fast_decode launch, one batched NMS

Both see the same images, the same weights and the same proposals: the RPN runs as it is, and its output is then filled up with fixed random
boxes (or cut) to exactly ``--top-n`` rows per image, so that an untrained RPN does not decide how much work the second stage has.  Each
size is measured at the two ends of what NMS can get: with the random weights as they are (background wins every RoI, nothing reaches NMS)
and with background taken out of the race (every RoI is a candidate); a trained model lies between.  The thresholds are fixed (--conf, --iou), the frame is the
input image's for both (ratio 1, no pads).

Timing as tools/bench_vgg.py: --warmup calls of each path, then the paths ALTERNATE, --rounds rounds of --steps calls; per round the wall time
per batch (device synchronised at both ends), the device time from events around the same calls, and the host time: a host clock around
issuing the calls, read before the final synchronise (what the host spends per batch, read-backs included).  Median over the rounds, spread =
(max - min) / median.  Prints one JSON line and writes it to --out.

usage: python tools/bench_faster_eval.py [--batch 4] [--height 800] [--width 1333] [--top-n 2000,300] [--steps 5] [--warmup 2] [--rounds 3]
       [--commit ID] [--out profiles/bench_faster_eval.json]"""
import argparse
import json
import os
import socket
import statistics
import subprocess
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import fastvision_amd
from fastvision_amd.demos.faster_rcnn.inference import anchor_fn, postProcess
from fastvision_amd.demos.faster_rcnn.models import Faster_Rcnn

DEV = 'cuda:0'
NUM_CLASSES = 20


def commit_id(given):
    if given:
        return given
    try:
        return subprocess.run(['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        return 'unknown'


def clock_mhz():
    try:
        return int(torch.cuda.clock_rate())          # the current shader clock, where the management library is present
    except Exception:
        return None


def build(top_n, H, W, foreground):
    torch.manual_seed(0)
    model = Faster_Rcnn(training=False, num_classes=NUM_CLASSES, base_anchors=anchor_fn([128, 256, 512], [0.5, 1, 2]),
                        rpn_post_nms_top_n=top_n).to(DEV).eval()
    if foreground:                                   # at random weights background wins every RoI and nothing reaches NMS: take it out of
        with torch.no_grad():                        # the race and spread the class logits, so that EVERY RoI is an NMS candidate
            model.fast.classifier.weight.mul_(40.0)
            model.fast.classifier.weight[0].zero_()
            model.fast.classifier.bias[0] = -100.0
    fh, fw = H // 16, W // 16
    g = torch.Generator().manual_seed(1)
    wh = torch.exp(torch.rand(top_n, 2, generator=g) * 2.5) * 1.5
    filler = torch.cat([torch.rand(top_n, 2, generator=g) * torch.tensor([float(fw), float(fh)]), wh], 1).to(DEV)
    real = model.rpn.filter_proposals

    def forced(*a, **k):                                          # the RPN's proposals, filled up / cut to exactly top_n rows per image
        return [torch.cat([p, filler], 0)[:top_n] for p in real(*a, **k)]
    model.rpn.filter_proposals = forced
    return model


def measure(fns, steps, warmup, rounds):
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    rec = {m: {'wall': [], 'gpu': [], 'host': []} for m in fns}
    for _ in range(rounds):
        for m, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            for _ in range(steps):
                fn()
            e1.record()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            rec[m]['wall'].append((t2 - t0) * 1e3 / steps)
            rec[m]['host'].append((t1 - t0) * 1e3 / steps)
            rec[m]['gpu'].append(e0.elapsed_time(e1) / steps)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--height', type=int, default=800)
    ap.add_argument('--width', type=int, default=1333)
    ap.add_argument('--top-n', default='2000,300')
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--conf', type=float, default=0.05)
    ap.add_argument('--iou', type=float, default=0.5)
    ap.add_argument('--commit', default='')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bench_faster_eval.json'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_faster_eval needs a GPU'
    B, H, W = a.batch, a.height, a.width
    props = torch.cuda.get_device_properties(0)
    res = {'workload': f'Faster R-CNN (VGG16, {NUM_CLASSES} classes) eval B={B} 3x{H}x{W} bf16, random weights seed 0, conf {a.conf} iou {a.iou}',
           'steps': a.steps, 'warmup': a.warmup, 'rounds': a.rounds, 'box': socket.gethostname(), 'device': torch.cuda.get_device_name(0),
           'compute_units': props.multi_processor_count, 'clock_mhz': clock_mhz(),
           'commit': commit_id(a.commit),
           'note': 'ms per batch, median of the rounds: wall = device synchronised at both ends; gpu = device events around the same calls; '
                   'host = host clock around issuing the calls, before the final synchronise.  Not measured: eval under a captured graph '
                   '(both paths read counts back), a trained model (fewer candidates reach NMS), other batch sizes.'}
    images = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(2)).to(DEV)
    args = types.SimpleNamespace(backbone_stride=16, inference_conf_thres=a.conf, inference_iou_thres=a.iou)
    frame = [(1.0, 0, 0, W, H)] * B
    with torch.no_grad(), fastvision_amd.compute_dtype(torch.bfloat16):
        for top_n, foreground in [(int(v), fg) for v in a.top_n.split(',') if v for fg in (False, True)]:
            model = build(top_n, H, W, foreground)
            found = {}

            def per_image():
                preds = model(images)
                out = [postProcess(p, args, 1.0, 0, 0, W, H) for p in preds]
                found['per_image'] = sum(o[2].size(0) for o in out)
                return out

            def batched():
                dets, kept = model.detect(images, a.conf, a.iou, max_det=300, letterboxes=frame)
                found['batched'] = kept
                return dets, kept
            rec = measure({'per_image': per_image, 'batched': batched}, a.steps, a.warmup, a.rounds)
            row = {'rois_per_image': top_n, 'detections': {'per_image': int(found['per_image']), 'batched': int(found['batched'].sum())}}
            for m, r in rec.items():
                wall = statistics.median(r['wall'])
                row[m] = {'wall_ms': round(wall, 3), 'img_per_s': round(B * 1e3 / wall, 1), 'gpu_ms': round(statistics.median(r['gpu']), 3),
                          'host_ms': round(statistics.median(r['host']), 3), 'spread': round((max(r['wall']) - min(r['wall'])) / wall, 4)}
            row['batched_over_per_image'] = round(row['per_image']['wall_ms'] / row['batched']['wall_ms'], 3)
            res[f'top_n_{top_n}_' + ('all_foreground' if foreground else 'all_background')] = row
            del model
            torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
