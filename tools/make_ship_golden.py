#!/usr/bin/env python3
"""Writes tests/golden/ship_loss.npz from the reference's own ship-demo ComputeLoss (demos/yolov3_huaweiShip/utils/lossv3.py), fp32 on the
CPU.  Run by hand where a checkout of the reference is at hand; no test runs it:

    python tools/make_ship_golden.py /path/to/reference

Inputs are tests/loss_restatement.demo_case('c65' / 'c1' / 'c80'), regenerated from their seeds by the test and not stored.  Stored per case:
the three values (box, cls, conf), and the gradients of their sum -- every level of c65 and c1, level 0 of c80.
"""
import importlib
import importlib.machinery
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import loss_restatement as lr  # noqa: E402

CASES = {'c65': None, 'c1': None, 'c80': 1}      # name -> number of levels whose gradient is stored (None: all)


def reference_loss(ref_root):
    """The reference's ComputeLoss, loaded by path: its ``utils`` package is entered without running its __init__ (which pulls in the
    plotting helpers), so that lossv3's relative imports of .iou and .box resolve to the reference's files."""
    pkg = types.ModuleType('ship_reference_utils')
    pkg.__path__ = [os.path.join(ref_root, 'demos', 'yolov3_huaweiShip', 'utils')]
    pkg.__spec__ = importlib.machinery.ModuleSpec('ship_reference_utils', None, is_package=True)
    sys.modules['ship_reference_utils'] = pkg
    return importlib.import_module('ship_reference_utils.lossv3').ComputeLoss()


def main():
    crit = reference_loss(sys.argv[1])
    out = {}
    for name, stored in CASES.items():
        layers, tg, anchors = lr.demo_case(name)
        leaves = [l.clone().requires_grad_(True) for l in layers]
        shell = types.SimpleNamespace(anchors=[a.clone() for a in anchors])
        parts = crit(leaves, tg.clone(), shell)
        (parts[0] + parts[1] + parts[2]).backward()
        out[f'{name}_values'] = np.array([p.item() for p in parts], dtype=np.float32)
        for l, leaf in enumerate(leaves[:stored]):
            out[f'{name}_grad{l}'] = leaf.grad.numpy().astype(np.float32)
        print(name, out[f'{name}_values'])
    path = os.path.join(ROOT, 'tests', 'golden', 'ship_loss.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
