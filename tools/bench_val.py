#!/usr/bin/env python3
"""The matching stage of one validation batch, two ways, in one process on the GPU:

  (a) per image, as Fit._val ran it before process_batch existed: read ``kept`` back, slice the NMS buffer, select the image's labels
      with a boolean mask, convert them, CalculateMAP.process_one (one IoU launch, seven device-to-host copies, numpy matching);
  (b) the NMS buffer as detect_ops.nms_batch_padded leaves it: the labels of the batch converted at once, one
      CalculateMAP.process_batch (one fva_map_match launch, no read-back); the host-side materialize() that fetch() runs once per epoch is
      timed separately (``materialize_ms``, per batch).

Both start from the same device tensors and end in a device synchronise inside the timed region; the two are timed alternately, after a
warm-up, and reported as median / min / max over the repeats.  The rows both produce are compared first (``rows_equal``).
``--forward`` adds the eval forward (decode included) of a YOLOv3 on a batch of the same size, for scale.  Prints one JSON line.

    python tools/bench_val.py [--batch 32] [--max-det 300] [--repeats 30] [--warmup 3] [--forward]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def synthetic_val_batch(B, max_det, size, seed=7, max_targets=20, n_cls=80):
    """(out [B,max_det,6] = xyxy, score, category, kept [B] int32, labels [T,6] = image, class, normalised xywh), on the CPU: 0..max_targets
    targets per image, one or two jittered detections for most of them and clutter up to 40..max_det rows, highest score first."""
    g = torch.Generator().manual_seed(seed)
    out = torch.zeros(B, max_det, 6)
    kept = torch.zeros(B, dtype=torch.int32)
    labels = []
    for b in range(B):
        nt = int(torch.randint(0, max_targets + 1, (1,), generator=g))
        wh = 0.04 + torch.rand(nt, 2, generator=g) * 0.4
        xy = wh / 2 + torch.rand(nt, 2, generator=g) * (1 - wh)
        cls = torch.randint(0, n_cls, (nt,), generator=g).float()
        labels.append(torch.cat([torch.full((nt, 1), float(b)), cls.view(-1, 1), xy, wh], dim=1))
        tbox = torch.cat([xy - wh / 2, xy + wh / 2], dim=1) * size
        boxes, classes = [], []
        for keep_p, sigma in ((0.8, 4.0), (0.4, 8.0)):
            m = torch.rand(nt, generator=g) < keep_p
            boxes.append(tbox[m] + torch.randn(int(m.sum()), 4, generator=g) * sigma)
            classes.append(cls[m])
        n = int(torch.randint(40, max_det + 1, (1,), generator=g))
        nf = max(n - sum(len(x) for x in boxes), 0)
        fxy = torch.rand(nf, 2, generator=g) * size * 0.8
        boxes.append(torch.cat([fxy, fxy + 16 + torch.rand(nf, 2, generator=g) * size * 0.2], dim=1))
        classes.append(torch.randint(0, n_cls, (nf,), generator=g).float())
        box, c = torch.cat(boxes)[:max_det], torch.cat(classes)[:max_det]
        perm = torch.randperm(box.size(0), generator=g)
        score = torch.sort(0.25 + 0.75 * torch.rand(box.size(0), generator=g), descending=True).values
        out[b, :box.size(0), 0:4], out[b, :box.size(0), 4], out[b, :box.size(0), 5] = box[perm], score, c[perm]
        kept[b] = box.size(0)
    return out, kept, torch.cat(labels)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--max-det', type=int, default=300)
    ap.add_argument('--size', type=int, default=640)
    ap.add_argument('--repeats', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--forward', action='store_true', help='also time the eval forward of a YOLOv3 on a batch of this size')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_val.py measures on the GPU: there is no CPU figure'
    from fastvision_amd.detection.tools import xywh2xyxy
    from fastvision_amd.metrics import CalculateMAP
    dev = torch.device('cuda:0')
    thr = np.linspace(0.5, 0.95, 10)
    out, kept, labels = (t.to(dev) for t in synthetic_val_batch(args.batch, args.max_det, args.size))
    scale = torch.tensor([args.size] * 4).to(labels)
    B = args.batch

    def per_image():
        est = CalculateMAP(thr)
        kept_h = kept.cpu().tolist()
        for b in range(B):
            det = out[b, :kept_h[b]]
            conf, cls, xyxy = det[:, 4:5], det[:, 5:6].long(), det[:, 0:4]
            predict = torch.cat([cls.float(), conf, xyxy], dim=1)
            target = labels[labels[:, 0] == b, 1:].clone()
            target[:, 1:] = xywh2xyxy(target[:, 1:]) * scale
            est.process_one(predict, target)
        torch.cuda.synchronize()
        return est

    def batched():
        est = CalculateMAP(thr)
        targets = torch.cat([labels[:, :2], xywh2xyxy(labels[:, 2:6]) * scale], dim=1)
        est.process_batch(out, kept, targets)
        torch.cuda.synchronize()
        return est

    a, b = per_image(), batched()
    b.materialize()
    rows_equal = len(a.correct_all_images) == len(b.correct_all_images) and \
        all(np.array_equal(x, y) for x, y in zip(a.correct_all_images, b.correct_all_images))
    true_pos = int(sum(c[:, 2].sum() for c in a.correct_all_images))
    for _ in range(args.warmup):
        per_image()
        batched().materialize()
    ta, tb, tm = [], [], []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        per_image()
        t1 = time.perf_counter()
        est = batched()
        t2 = time.perf_counter()
        est.materialize()
        t3 = time.perf_counter()
        ta.append((t1 - t0) * 1e3), tb.append((t2 - t1) * 1e3), tm.append((t3 - t2) * 1e3)

    def stats(v):
        return {'median': round(statistics.median(v), 4), 'min': round(min(v), 4), 'max': round(max(v), 4)}

    res = {'bench': 'val_matching', 'batch': B, 'max_det': args.max_det, 'detections': int(kept.sum()), 'targets': int(labels.size(0)),
           'true_positives_at_0.5': true_pos, 'thresholds': len(thr), 'repeats': args.repeats, 'rows_equal': bool(rows_equal),
           'per_image_ms': stats(ta), 'batched_ms': stats(tb), 'materialize_ms': stats(tm),
           'ratio_per_image_over_batched': round(statistics.median(ta) / statistics.median(tb), 2),
           'ratio_with_materialize': round(statistics.median(ta) / (statistics.median(tb) + statistics.median(tm)), 2),
           'device': torch.cuda.get_device_name(0)}
    if args.forward:
        import fastvision_amd  # noqa: F401
        from fastvision_amd.classfication.models import darknet53
        from fastvision_amd.detection.head import yolov3head
        from fastvision_amd.detection.models import yolov3
        from fastvision_amd.detection.neck import yolov3neck
        from fastvision_amd.synthetic import coco_anchors_px
        torch.manual_seed(0)
        m = yolov3(backbone=darknet53, neck=yolov3neck, head=yolov3head, anchors=coco_anchors_px(), num_anchors_per_level=[3, 3, 3],
                   in_channels=3, num_classes=80, training=True).to(dev).eval()
        images = torch.rand(B, 3, args.size, args.size, device=dev)
        tf = []
        with torch.no_grad():
            for i in range(3 + 10):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                m(images, val=True)
                torch.cuda.synchronize()
                if i >= 3:
                    tf.append((time.perf_counter() - t0) * 1e3)
        res['eval_forward_ms'] = stats(tf)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
