"""RandAugment and RandomErasing on the device (not in the reference: the per-image augmentation its classifiers are usually trained with).

``RandAugment(...)(canvases)`` takes the uint8 ``[B, H, W, 3]`` canvases that ``pipeline_ops.paste_batch_u8`` leaves on the device and
returns augmented canvases of the same shape: one ``fva_randaug_plan`` launch (a one-block tick kernel that draws, per image and round,
one of the enabled ops and the sign of its value from Philox-4x32-10 keyed by a seed and a call counter in device memory), then per round
``fva_randaug_stats`` (histograms, for the images whose op needs them) and ``fva_randaug_apply`` (one pass, ping-pong between two
canvases).  No host synchronisation, no ATen compute; a captured graph draws a new plan on every replay.

``RandomErasing(...)(batch)`` erases one box per image of the normalised ``[B, C, H, W]`` batch (``fva_random_erase``), the box drawn on the
device as torchvision draws it.  ``normalise`` is the step between the two: canvases -> planar fp32 through the byte -> value table of
``fva_colour_blur_shuffle_normalize``.  canvases -> RandAugment -> normalise -> RandomErasing -> BatchMix -> model never leaves the device.
"""
import torch
import torch.nn as nn

from . import _lib
from .ops import _code, _p, _stream, require_gpu
from .pipeline_ops import _colour_jobs, value_table

__all__ = ['RandAugment', 'RandomErasing', 'normalise', 'OPS', 'MAX_OPS']

# the order of fva_randaug_op (include/fastvision_amd.h)
OPS = ('Identity', 'ShearX', 'ShearY', 'TranslateX', 'TranslateY', 'Rotate', 'Brightness', 'Color', 'Contrast', 'Sharpness', 'Posterize',
       'Solarize', 'AutoContrast', 'Equalize')
MAX_OPS = 4


def _state(seed):
    seed = torch.initial_seed() if seed is None else int(seed)
    return torch.tensor([seed & 0x7FFFFFFFFFFFFFFF, 0, 0, 0], dtype=torch.int64)


class RandAugment(nn.Module):
    """torchvision's ``RandAugment(num_ops, magnitude, num_magnitude_bins, fill)`` for a whole batch on the device.  ``ops``: the names
    (of ``OPS``) to draw from, default all 14.  ``seed`` defaults to ``torch.initial_seed()`` (read, not drawn).  ``_state`` is a
    non-persistent buffer that follows ``.to(device)``; the plan of the last call stays in ``plan`` (int32 ``[B, num_ops, 2]``: op, and the
    bits of the fp32 value).  In ``.eval()`` the module is the identity."""

    def __init__(self, num_ops=2, magnitude=9, num_magnitude_bins=31, fill=(0, 0, 0), ops=None, seed=None):
        super().__init__()
        if not 1 <= int(num_ops) <= MAX_OPS:
            raise ValueError(f'RandAugment: num_ops = {num_ops} must lie in 1 .. {MAX_OPS}')
        if int(num_magnitude_bins) < 2 or not 0 <= int(magnitude) < int(num_magnitude_bins):
            raise ValueError(f'RandAugment: magnitude = {magnitude} is no bin of {num_magnitude_bins}')
        fill = (fill,) * 3 if isinstance(fill, (int, float)) else tuple(fill)
        if len(fill) != 3 or any(not 0 <= int(f) <= 255 for f in fill):
            raise ValueError(f'RandAugment: fill = {fill} must be one byte or three')
        names = OPS if ops is None else tuple(ops)
        unknown = [n for n in names if n not in OPS]
        if unknown or not names:
            raise ValueError(f'RandAugment: ops must name some of {OPS}, got {unknown or names}')
        self.num_ops, self.magnitude, self.num_magnitude_bins = int(num_ops), int(magnitude), int(num_magnitude_bins)
        self.fill = tuple(int(f) for f in fill)
        self.op_mask = sum(1 << OPS.index(n) for n in set(names))
        self.register_buffer('_state', _state(seed), persistent=False)
        self.plan = None
        self._work = None                                      # (B, histogram workspace): zero once, then owned by the kernels

    def _buffers_for(self, canvases):
        require_gpu(canvases, 'RandAugment')
        if canvases.dim() != 4 or canvases.shape[3] != 3 or canvases.dtype != torch.uint8:
            raise RuntimeError(f'RandAugment: expected uint8 [B, H, W, 3] canvases, got {tuple(canvases.shape)} {canvases.dtype}')
        B = canvases.shape[0]
        dev = canvases.device
        if self.plan is None or self.plan.shape[0] != B or self.plan.device != dev:
            self.plan = torch.zeros(B, self.num_ops, 2, dtype=torch.int32, device=dev)
            self._work = torch.zeros(_lib.load().fva_randaug_workspace(B) // 4, dtype=torch.int32, device=dev)
        return canvases if canvases.is_contiguous() else canvases.contiguous()

    def _rounds(self, x):
        B, H, W, _ = x.shape
        stream = _stream()
        fill = self.fill[0] | self.fill[1] << 8 | self.fill[2] << 16
        pong = [torch.empty_like(x) for _ in range(min(self.num_ops, 2))]
        for r in range(self.num_ops):
            out = pong[r & 1]
            _lib.call('fva_randaug_stats', _p(x), _p(self.plan), r, self.num_ops, B, H, W, _p(self._work), stream)
            _lib.call('fva_randaug_apply', _p(x), _p(out), _p(self.plan), r, self.num_ops, B, H, W, fill, _p(self._work), stream)
            x = out
        return x

    def forward(self, canvases):
        if not self.training:
            return canvases
        x = self._buffers_for(canvases)
        if self._state.device != x.device:
            raise RuntimeError(f'RandAugment: its state is on {self._state.device}, the canvases on {x.device}: move the module with .to(device)')
        B, H, W, _ = x.shape
        _lib.call('fva_randaug_plan', _p(self._state), B, self.num_ops, self.magnitude, self.num_magnitude_bins, H, W, self.op_mask, _p(self.plan),
                  _stream())
        return self._rounds(x)

    def apply_plan(self, canvases, ops, values):
        """Run a caller-given plan: ``ops`` (names of ``OPS`` or their indices) and ``values``, both ``[B, num_ops]``."""
        x = self._buffers_for(canvases)
        B = x.shape[0]
        if not torch.is_tensor(ops):
            ops = torch.tensor([[OPS.index(o) if isinstance(o, str) else int(o) for o in row] for row in ops], dtype=torch.int32)
        ops = ops.to(device=x.device, dtype=torch.int32).contiguous()
        values = torch.as_tensor(values, dtype=torch.float32).to(x.device).contiguous()
        if tuple(ops.shape) != (B, self.num_ops) or tuple(values.shape) != (B, self.num_ops):
            raise RuntimeError(f'RandAugment.apply_plan: ops {tuple(ops.shape)} and values {tuple(values.shape)} must both be [{B}, {self.num_ops}]')
        _lib.call('fva_randaug_plan_fixed', _p(ops), _p(values), B, self.num_ops, _p(self.plan), _stream())
        return self._rounds(x)

    def plan_arrays(self):
        """(ops int64 [B, N], values float32 [B, N]) of the last plan as numpy arrays: reads the device (tests, logging)."""
        words = self.plan.detach().cpu()
        return words[..., 0].long().numpy(), words[..., 1].contiguous().view(torch.float32).numpy()


class RandomErasing(nn.Module):
    """torchvision's ``RandomErasing(p, scale, ratio, value, inplace)`` for a batch ``[B, C, H, W]`` (fp32 or bf16) on the device, one box
    per image.  ``value``: a number, or ``'random'`` for N(0, 1) noise.  The boxes of the last call stay in ``boxes`` (int32 ``[B, 4]``:
    top, left, height, width; zeros where nothing was erased).  In ``.eval()`` the module is the identity."""

    def __init__(self, p=0.5, scale=(0.02, 0.33), ratio=(0.3, 3.3), value=0, inplace=False, seed=None):
        super().__init__()
        if not 0.0 <= float(p) <= 1.0:
            raise ValueError(f'RandomErasing: p = {p} must lie in [0, 1]')
        if not 0.0 <= scale[0] <= scale[1] <= 1.0 or not 0.0 < ratio[0] <= ratio[1]:
            raise ValueError(f'RandomErasing: scale = {scale} must be ordered in [0, 1] and ratio = {ratio} ordered and positive')
        if value != 'random' and not isinstance(value, (int, float)):
            raise ValueError(f"RandomErasing: value = {value!r} must be a number or 'random'")
        self.p, self.scale, self.ratio = float(p), (float(scale[0]), float(scale[1])), (float(ratio[0]), float(ratio[1]))
        self.value, self.inplace = value, bool(inplace)
        self.register_buffer('_state', _state(seed), persistent=False)
        self.boxes = None

    def forward(self, batch):
        if not self.training:
            return batch
        require_gpu(batch, 'RandomErasing')
        if batch.dim() != 4 or batch.dtype not in (torch.float32, torch.bfloat16):
            raise RuntimeError(f'RandomErasing: expected [B, C, H, W] fp32 / bf16, got {tuple(batch.shape)} {batch.dtype}')
        if self._state.device != batch.device:
            raise RuntimeError(f'RandomErasing: its state is on {self._state.device}, the batch on {batch.device}: move the module with .to(device)')
        if self.inplace and not batch.is_contiguous():
            raise RuntimeError('RandomErasing(inplace=True) needs a contiguous batch')
        x = batch.detach()
        x = x if x.is_contiguous() else x.contiguous()
        B, Cc, H, W = x.shape
        if self.boxes is None or self.boxes.shape[0] != B or self.boxes.device != x.device:
            self.boxes = torch.zeros(B, 4, dtype=torch.int32, device=x.device)
        out = x if self.inplace else torch.empty_like(x)
        noise = self.value == 'random'
        _lib.call('fva_random_erase', _code(x.dtype), _p(x), _p(out), _p(self._state), B, Cc, H, W, self.p, self.scale[0], self.scale[1], self.ratio[0],
                  self.ratio[1], int(noise), 0.0 if noise else float(self.value), _p(self.boxes), _stream())
        return batch if self.inplace else out


_tables = {}


def normalise(canvases, mean, std, dtype=torch.float32):
    """uint8 canvases ``[B, H, W, 3]`` -> planar ``[B, 3, H, W]`` of ``(x / 255 - mean) / std``: ``fva_colour_blur_shuffle_normalize`` with
    no blur and the identity permutation.  The job and value tables are made on the first call for a shape (a host-to-device copy: make
    that call before a graph capture) and kept.  That kernel writes fp32; another ``dtype`` raises."""
    require_gpu(canvases, 'normalise')
    if dtype != torch.float32:
        raise NotImplementedError(f'normalise: fva_colour_blur_shuffle_normalize writes fp32, not {dtype}')
    if canvases.dim() != 4 or canvases.shape[3] != 3 or canvases.dtype != torch.uint8:
        raise RuntimeError(f'normalise: expected uint8 [B, H, W, 3] canvases, got {tuple(canvases.shape)} {canvases.dtype}')
    B, H, W, _ = canvases.shape
    key = (B, H, W, tuple(float(m) for m in mean), tuple(float(s) for s in std), canvases.device)
    if key not in _tables:
        jobs = _colour_jobs([(H, W)] * B, [0] * B, [0] * B, [0] * B, [(0, 1, 2)] * B, canvases.device)
        _tables[key] = (jobs, torch.from_numpy(value_table(key[3], key[4])).to(canvases.device))
    jobs, lut = _tables[key]
    x = canvases if canvases.is_contiguous() else canvases.contiguous()
    out = torch.empty(B, 3, H, W, dtype=torch.float32, device=x.device)
    _lib.call('fva_colour_blur_shuffle_normalize', _p(x), B, H, W, _p(jobs), _p(lut), _p(out), _stream())
    return out
