#!/usr/bin/env python3
"""One optimizer step of FusedLAMB beside FusedAdam and of FusedLARS beside FusedSGD on the real parameter sets: Darknet-53 + YOLOv3
(61.9 M parameters) and resnet50, with fixed random gradients.

Per model and optimizer two figures, both from device events over --iters steps after warm-up:
    eager    ``optimizer.step()`` as a training loop calls it (host table checks included where the device is faster than the host)
    replay   the same step captured in a HIP graph and replayed: the launches alone
The pair of a comparison ALTERNATES --rounds times in one process; per figure the median, the best and the spread of its rounds.  The
yardstick of the new step is the existing optimizer's median scaled by the bytes each moves per parameter (LAMB 40 / Adam 28; LARS 28 /
SGD 20, momentum, no clipping) plus two launches of an empty kernel measured the same way in the same run (the norm and the trust pass).

Writes one JSON object to --out (default profiles/bench_layerwise.json) and prints it as one line.
usage: python tools/bench_layerwise.py [--iters N] [--rounds R] [--models yolov3,resnet50] [--out PATH]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch          # noqa: E402

from fastvision_amd import FusedAdam, FusedLAMB, FusedLARS, FusedSGD, layerwise_groups          # noqa: E402

DEV = 'cuda:0'
PAIRS = [('FusedAdam', 'FusedLAMB', 40 / 28), ('FusedSGD', 'FusedLARS', 28 / 20)]
MAKE = {'FusedAdam': lambda g: FusedAdam(g, lr=1e-4, betas=(0.937, 0.999), capturable=True),
        'FusedLAMB': lambda g: FusedLAMB(g, lr=1e-4, betas=(0.937, 0.999), capturable=True),
        'FusedSGD': lambda g: FusedSGD(g, lr=1e-4, momentum=0.9, nesterov=True, capturable=True),
        'FusedLARS': lambda g: FusedLARS(g, lr=1e-4, momentum=0.9, nesterov=True, capturable=True)}


def model(name):
    from fastvision_amd.classfication import models
    if name == 'resnet50':
        return models.resnet50()
    from fastvision_amd.detection.head import yolov3head
    from fastvision_amd.detection.models import yolov3
    from fastvision_amd.detection.neck import yolov3neck
    from fastvision_amd.synthetic import coco_anchors_px
    return yolov3(backbone=models.darknet53, neck=yolov3neck, head=yolov3head, anchors=coco_anchors_px(), num_anchors_per_level=[3, 3, 3],
                  in_channels=3, num_classes=80, training=True)


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


def graphed(fn):
    """``fn`` (already run once eagerly) captured; returns (replay, what must stay alive)."""
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph.replay, graph


def steps_of(name, net):
    """{'eager': step, 'replay': replay of the captured step} of optimizer ``name`` on its own copy of ``net``'s parameters."""
    gen = torch.Generator(device=DEV).manual_seed(0)
    copy = torch.nn.Module()
    for i, p in enumerate(net.parameters()):
        q = torch.nn.Parameter(p.detach().clone())
        q.grad = torch.randn(p.shape, generator=gen, device=DEV) * 1e-2
        copy.register_parameter(f'p{i}', q)
    opt = MAKE[name](layerwise_groups(copy, 5e-4))
    opt.step()
    keep = opt.begin_capture()
    replay, graph = graphed(opt.step)
    return {'eager': opt.step, 'replay': replay}, (opt, keep, graph, copy)


def stats(runs):
    med = statistics.median(runs)
    return {'median_us': round(med, 1), 'best_us': round(min(runs), 1), 'spread_pct': round((max(runs) - min(runs)) / med * 100, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--models', default='yolov3,resnet50')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bench_layerwise.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_layerwise needs a GPU')
    one = torch.zeros(1, device=DEV).zero_()
    empty = {'eager': lambda: one.zero_()}
    empty['replay'], keep_empty = graphed(lambda: [one.zero_() for _ in range(100)])
    out = {'iters': args.iters, 'rounds': args.rounds, 'models': {}}
    for name in args.models.split(','):
        net = model(name).to(DEV)
        row = out['models'][name] = {'parameters': sum(p.numel() for p in net.parameters()), 'tensors': len(list(net.parameters()))}
        for old, new, ratio in PAIRS:
            (so, ko), (sn, kn) = steps_of(old, net), steps_of(new, net)
            runs = {(o, m): [] for o in (old, new, 'empty') for m in ('eager', 'replay')}
            for _ in range(args.rounds):
                for m in ('eager', 'replay'):
                    runs[old, m].append(event_us(so[m], args.iters))
                    runs[new, m].append(event_us(sn[m], args.iters))
                    runs['empty', m].append(event_us(empty[m], args.iters) / (100 if m == 'replay' else 1))
            for m in ('eager', 'replay'):
                o, n, e = stats(runs[old, m]), stats(runs[new, m]), stats(runs['empty', m])
                yard = o['median_us'] * ratio + 2 * e['median_us']
                row[f'{new}/{m}'] = {old: o, new: n, 'empty_launch': e, 'byte_ratio': round(ratio, 3), 'yardstick_us': round(yard, 1),
                                     'new_over_yardstick': round(n['median_us'] / yard, 3), 'new_over_old': round(n['median_us'] / o['median_us'], 3)}
            del ko, kn
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
