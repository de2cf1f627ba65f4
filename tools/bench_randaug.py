#!/usr/bin/env python3
"""What RandAugment and RandomErasing cost on the device: 256 x 224 x 224 x 3 uint8 canvases (38.5 MB),

    pipeline   RandAugment(num_ops=2, magnitude=9): fva_randaug_plan + 2 x (fva_randaug_stats + fva_randaug_apply), a new plan per call
    <op>       one round with EVERY image on that op (apply_plan: fva_randaug_plan_fixed + stats + apply), at the value of bin 9 of 31
    erase      RandomErasing(p=0.5) on the normalised fp32 batch, out of place and in place
    copy       a device-to-device copy of the canvases (the same bytes read and written once: the floor of one apply pass)

The variants ALTERNATE in one process, --rounds times each after warm-up, --iters launches per round timed by device events; the figure
per variant is the median of its rounds, the spread (max - min) / median beside it, and its ratio to the copy's median.  No ratio is
asserted anywhere.  Prints one JSON line (kept as profiles/bench_randaug.json).

usage: python tools/bench_randaug.py [--batch B] [--size S] [--rounds R] [--iters N]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from fastvision_amd import RandAugment, RandomErasing
from fastvision_amd.augment import OPS

DEV = 'cuda:0'


def event_us(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3


def bin_value(op, S, frac=9 / 30):
    return {'ShearX': 0.3 * frac, 'ShearY': 0.3 * frac, 'TranslateX': float(int(150 / 331 * S * frac)), 'TranslateY': float(int(150 / 331 * S * frac)),
            'Rotate': 30 * frac, 'Posterize': 7.0, 'Solarize': 255 - 255 * frac, 'Identity': 0.0, 'AutoContrast': 0.0, 'Equalize': 0.0}.get(op, 0.9 * frac)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--size', type=int, default=224)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_randaug: no GPU -- nothing to measure here')
    B, S = args.batch, args.size
    gen = torch.Generator().manual_seed(0)
    canv = torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, generator=gen).to(DEV)
    dst = torch.empty_like(canv)
    batch = torch.randn(B, 3, S, S, generator=gen).to(DEV)
    variants = {'copy': lambda: dst.copy_(canv)}
    pipe = RandAugment(num_ops=2, magnitude=9, seed=1).to(DEV)
    variants['pipeline N=2'] = lambda: pipe(canv)
    for op in OPS:
        one = RandAugment(num_ops=1, seed=1).to(DEV)
        ops = torch.full((B, 1), OPS.index(op), dtype=torch.int32, device=DEV)
        vals = torch.full((B, 1), bin_value(op, S), dtype=torch.float32, device=DEV)
        variants[op] = lambda one=one, ops=ops, vals=vals: one.apply_plan(canv, ops, vals)
    out_of_place, in_place = RandomErasing(seed=2).to(DEV), RandomErasing(seed=2, inplace=True).to(DEV)
    scratch = batch.clone()
    variants['erase fp32 out of place'] = lambda: out_of_place(batch)
    variants['erase fp32 in place'] = lambda: in_place(scratch)
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    runs = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            runs[k].append(event_us(fn, args.iters))
    copy_us = statistics.median(runs['copy'])
    canvas_bytes = canv.numel()
    rows = {}
    for k, v in runs.items():
        med = statistics.median(v)
        rows[k] = {'us': round(med, 1), 'spread': round((max(v) - min(v)) / med, 3), 'over_copy': round(med / copy_us, 2)}
    rows['copy']['gb_per_s'] = round(2 * canvas_bytes / copy_us / 1e3, 1)
    print(json.dumps({'workload': f'{B} x {S} x {S} x 3 uint8 canvases ({canvas_bytes / 1e6:.1f} MB); erase on the fp32 batch ({batch.numel() * 4 / 1e6:.1f} MB)',
                      'method': f'variants alternating, median of {args.rounds} rounds of {args.iters} launches, device events; over_copy = median / the copy\'s median '
                                '(the copy reads and writes the canvases once; the erase rows move four times the bytes out of place)',
                      'device': torch.cuda.get_device_name(0), 'rows': rows}))


if __name__ == '__main__':
    main()
