"""Zero-edit drop-in (north_star: "demos/yolov3_u drops in unchanged"): the import lines of the reference's own entry scripts must
resolve, verbatim, to this implementation -- ``fastvision.*`` through the alias package at the repository root, the demo's
top-level ``models`` / ``utils`` / ``cfg`` / ``data_gen`` through the shim directory ``demos/yolov3_u`` used as a path entry.
The statements below are quoted from generate/template-yolov3/train.py:8-13,67-70, generate/template-yolov3/inference.py:10-14
(minus the plotting helper's text rendering) and demos/yolov3_u/train.py:9-15.  CPU only: nothing here computes on a device."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TEMPLATE_IMPORTS = '''
from fastvision.datasets.detection_dataloader import create_dataloader, show_dataset
from fastvision.detection.tools import AnchorGenerator
from fastvision.utils.checkpoints import LoadStatedict
from fastvision.loss import Yolov3Loss
from fastvision.utils import Fit
from fastvision.utils.sheduler import CosineLR, LinearLR
from fastvision.detection.tools import non_max_suppression
from fastvision.detection.plot import draw_box_label
from fastvision.utils.seed import set_random_seeds
from fastvision.utils.device import set_device
from fastvision.classfication.models import darknet53
from fastvision.detection.neck import yolov3neck
from fastvision.detection.head import yolov3head
from fastvision.detection.models import yolov3
'''

DEMO_IMPORTS = '''
from data_gen import create_dataset
from utils.anchor_generator import AnchorGenerator
from utils.map import mean_average_precision
from cfg._fit import Fit
from models.yolov3 import YoloV3

from utils.lossv3 import ComputeLoss
'''


def _run(code, extra_path):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(extra_path + [os.environ.get('PYTHONPATH', '')]), PYTHONDONTWRITEBYTECODE='1')
    return subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=300, cwd='/tmp')


def test_template_import_lines_resolve_to_this_implementation():
    code = TEMPLATE_IMPORTS + '''
import fastvision, fastvision_amd
import fastvision.detection.models.yolov3 as a, fastvision_amd.detection.models.yolov3 as b
assert a is b and fastvision.loss.yolov3_loss is fastvision_amd.loss.yolov3_loss          # ONE copy of every module
assert Yolov3Loss.__module__ == 'fastvision_amd.loss.yolov3_loss'
m = yolov3(backbone=darknet53, neck=yolov3neck, head=yolov3head, anchors=__import__('torch').ones(9, 2), num_anchors_per_level=[3, 3, 3],
           in_channels=3, num_classes=80, training=True)
assert len(m.state_dict()) == 438 and len(list(m.parameters())) == 222      # the reference's state_dict keys (parameters + BatchNorm buffers)
try:
    import fastvision.videoRecognition
    raise SystemExit('out-of-scope package resolved')
except ModuleNotFoundError:
    pass
print('ok')
'''
    r = _run(code, [ROOT])
    assert r.returncode == 0 and r.stdout.strip().endswith('ok'), r.stdout + r.stderr


def test_demo_import_lines_resolve_through_the_path_entry():
    code = DEMO_IMPORTS + '''
import fastvision_amd.demos.yolov3_u as real
assert YoloV3 is real.models.yolov3.YoloV3 and ComputeLoss is real.utils.lossv3.ComputeLoss and Fit is real.cfg._fit.Fit
assert create_dataset is real.data_gen.create_dataset
print('ok')
'''
    r = _run(code, [os.path.join(ROOT, 'demos', 'yolov3_u'), ROOT])
    assert r.returncode == 0 and r.stdout.strip().endswith('ok'), r.stdout + r.stderr


def test_anchor_generator_recovers_planted_clusters(tmp_path):
    from fastvision_amd.detection.tools import AnchorGenerator
    rng = np.random.RandomState(3)
    centres = np.array([[0.05, 0.08], [0.2, 0.15], [0.5, 0.6]])
    wh = np.concatenate([c * (1 + 0.03 * rng.randn(200, 2)) for c in centres]).astype(np.float32)
    labels = torch.from_numpy(np.concatenate([np.zeros((600, 4), np.float32), wh], axis=1))
    loader = [(torch.zeros(2, 3, 320, 640), labels[:300]), (torch.zeros(2, 3, 320, 640), labels[300:])]
    np.random.seed(0)
    got = AnchorGenerator([loader], k=3, iters=30, cache=str(tmp_path / 'anchors')).get_anchors()
    want = centres[::-1] * np.array([640, 320])                       # largest area first, input pixels
    assert got.shape == (3, 2) and np.allclose(got, want, rtol=0.05)
    again = AnchorGenerator([loader], k=3, cache=str(tmp_path / 'anchors'), use_cache=True).get_anchors()
    assert np.allclose(again, got)


def test_demo_mean_average_precision():
    from fastvision_amd.demos.yolov3_u.utils.map import mean_average_precision
    m = mean_average_precision(np.linspace(0.5, 0.95, 10))
    true = torch.tensor([[0, 10, 10, 50, 50], [1, 60, 60, 90, 90.]])
    m.process_one(torch.tensor([[0, 0.9, 10, 10, 50, 50], [1, 0.8, 60, 60, 90, 90.]]), true)      # two perfect detections
    ap, classes, per_class = m.fetch()
    assert np.allclose(ap, 1.0, atol=1e-2) and classes.tolist() == [0.0, 1.0]
    m = mean_average_precision([0.5, 0.75])
    # class 0: one good box (IoU 1), one duplicate (loses the pairing), class 1: IoU 0.63 -> correct at 0.5 only
    m.process_one(torch.tensor([[0, 0.9, 10, 10, 50, 50], [0, 0.7, 12, 12, 50, 50], [1, 0.8, 60, 60, 90, 79.]]), true)
    ap, classes, per_class = m.fetch()
    assert per_class.shape == (2, 2)
    assert per_class[0, 0] > 0.99 and per_class[1, 0] > 0.99 and per_class[1, 1] == 0.0
    m.process_one(torch.zeros(0, 6), torch.zeros(0, 5))                                             # empty image: no effect
    assert np.allclose(m.fetch()[0], ap)


def _write_dataset(root, n=6, seed=0):
    from PIL import Image
    rng = np.random.RandomState(seed)
    os.makedirs(os.path.join(root, 'images'))
    os.makedirs(os.path.join(root, 'labels'))
    for i in range(n):
        h, w = int(rng.randint(40, 90)), int(rng.randint(40, 90))
        Image.fromarray(rng.randint(0, 255, (h, w, 3), dtype=np.uint8)).save(os.path.join(root, 'images', f'im{i}.png'))
        with open(os.path.join(root, 'labels', f'im{i}.txt'), 'w') as f:
            for _ in range(int(rng.randint(1, 4))):
                x0, y0 = rng.randint(0, w // 2), rng.randint(0, h // 2)
                f.write(f'{rng.randint(0, 5)} {x0} {y0} {x0 + rng.randint(4, w // 2)} {y0 + rng.randint(4, h // 2)}\n')


def test_loader_workers_only_pack_bytes_and_never_touch_the_gpu(tmp_path):
    """create_dataloader with num_workers=2: the worker-side collate must neither pin memory nor ask for a device (a forked worker
    has no GPU context); the host batch arrives as plain tensors.  Iterated on the CPU side only (DeviceLoader.loader)."""
    from fastvision_amd.datasets import create_dataloader, show_dataset
    _write_dataset(str(tmp_path))
    loader = create_dataloader('train', str(tmp_path), batch_size=3, input_size=64, device=torch.device('cpu'), num_workers=2,
                               cache=str(tmp_path / 'cache'), shuffle=False)
    seen = 0
    for buf, offsets, shapes, flips, labels in loader.loader:                   # the host half: what the workers produce
        assert buf.dtype == torch.uint8 and not buf.is_pinned() and labels.shape[1] == 6
        assert int(offsets[-1]) + shapes[-1][0] * shapes[-1][1] * 3 == buf.numel()
        assert labels[:, 0].max() == len(shapes) - 1
        seen += len(shapes)
    assert seen == 6
    written = show_dataset('train', str(tmp_path), [str(c) for c in range(5)], cache=str(tmp_path / 'cache'), use_cache=True, limit=2)
    assert len(written) == 2 and all(os.path.getsize(p) > 100 for p in written)


def test_demo_dataset_surface_with_workers(tmp_path):
    """The demo's loaders as its train.py builds them: create_dataset + DataLoader(collate_fn=dataset.collate_fn, num_workers=2).
    The image half of a batch is a HostImageBatch (bytes + plan; its .cuda() runs the kernels), the label half the final [T,6]
    table -- equal to what DeviceAugmenter computes for the same draws."""
    from torch.utils.data import DataLoader
    from fastvision_amd.demos.yolov3_u.data_gen import DeviceAugmenter, HostImageBatch, create_dataset
    _write_dataset(str(tmp_path), n=5, seed=1)
    np.random.seed(0)
    for mode in ('val', 'train'):
        ds = create_dataset(str(tmp_path), 64, mode)
        loader = DataLoader(dataset=ds, batch_size=2, shuffle=False, pin_memory=False, drop_last=False, num_workers=2, collate_fn=ds.collate_fn)
        n = 0
        for images, target in loader:
            assert isinstance(images, HostImageBatch) and images.size() == (len(images), 3, 64, 64)
            assert target.dtype == torch.float32 and target.shape[1] == 6 and target[:, 0].max() == len(images) - 1
            assert target[:, 2:].min() >= 0 and target[:, 2:].max() <= 1.0 + 1e-6
            plan = DeviceAugmenter(64, 'cpu')
            want = plan.train_labels(images.samples) if mode == 'train' else plan.val_labels(images.samples)
            for i, l in enumerate(want):
                l[:, 0] = i
            assert torch.equal(torch.cat(want, 0), target)
            n += len(images)
        assert n == 5
