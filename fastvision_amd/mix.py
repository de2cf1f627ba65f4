"""MixUp and CutMix on the device (not in the reference: the recipe its ResNet / ResNeXt / VGG classifiers are usually trained with).

``BatchMix.mix(images, labels)`` is two launches and no host synchronisation:

  * ``fva_mix_plan`` -- a one-thread tick kernel that draws, on the device, whether this batch is mixed at all, MixUp or CutMix, lambda ~
    Beta(alpha, alpha) and torchvision's CutMix box, from Philox-4x32-10 keyed by (seed, call counter).  Seed and counter live in the
    int64[4] buffer ``_state`` (the protocol of the dropout state) and the launch advances the counter itself: a captured graph draws a
    new plan on every replay.  A lambda drawn on the host would be frozen into the graph.
  * ``fva_mix_apply`` -- one streaming pass: image b is mixed with image (b - 1) % B (``images.roll(1, 0)``: no permutation, the loader
    already shuffles) as the plan, read on the device, says.

The labels are not mixed into [N, C] rows: ``mix`` returns ``MixedLabels(labels, plan)`` and ``loss.CrossEntropyLoss`` reads lambda from
the plan on the device (``fva_softmax_ce_soft``), pairing row r with row r - 1 as the images were.
"""
import torch
import torch.nn as nn

from . import _lib
from .ops import _code, _p, _stream, require_gpu

__all__ = ['BatchMix', 'MixedLabels', 'PLAN_WORDS', 'plan_fields']

PLAN_WORDS = 9          # fva_mix_plan_t: mode, lam_raw, lam, rx, ry, x1, y1, x2, y2 (32-bit each)


def plan_fields(plan):
    """A plan tensor (int32[9]) as a dict of Python numbers: reads the device, so it synchronises the host (tests, logging)."""
    words = plan.detach().cpu()
    lam_raw, lam = words[1:3].view(torch.float32).tolist()
    mode, _, _, rx, ry, x1, y1, x2, y2 = words.tolist()
    return dict(mode=mode, lam_raw=lam_raw, lam=lam, rx=rx, ry=ry, x1=x1, y1=y1, x2=x2, y2=y2)


class MixedLabels:
    """The labels of a mixed batch: ``labels`` [N] or [N, 1] as the loader gave them and the int32[9] ``plan`` tensor that holds lambda.
    Row r's target is lam * onehot(labels[r]) + (1 - lam) * onehot(labels[r - 1])."""

    def __init__(self, labels, plan):
        self.labels, self.plan = labels, plan

    def lam(self):
        """lambda as a one-element fp32 view of the plan (on the plan's device; no copy, no synchronisation)"""
        return self.plan[2:3].view(torch.float32)

    @property
    def device(self):
        return self.labels.device

    def to(self, *args, **kwargs):
        return MixedLabels(self.labels.to(*args, **kwargs), self.plan.to(*args, **kwargs))


class BatchMix(nn.Module):
    """``mixed_images, mixed_labels = BatchMix(...)(images, labels)`` for a batch that is on the device: planar [B, C, H, W] fp32 or
    bf16.  ``prob``: the share of batches that are mixed at all; ``switch_prob``: the share of CutMix among them when both alphas are
    positive (an alpha of 0 switches that mode off).  0 <= alpha <= 1: lambda comes from Johnk's method, alpha > 1 raises ValueError.
    ``seed`` defaults to ``torch.initial_seed()`` (read, not drawn).  In ``.eval()`` the module is the identity.  ``_state`` and ``_plan``
    are non-persistent buffers: they follow ``.to(device)`` and stay out of checkpoints."""

    def __init__(self, mixup_alpha=0.2, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5, seed=None):
        super().__init__()
        for name, a in (('mixup_alpha', mixup_alpha), ('cutmix_alpha', cutmix_alpha)):
            if not 0.0 <= float(a) <= 1.0:
                raise ValueError(f'BatchMix: {name} = {a} must lie in [0, 1] (lambda ~ Beta(alpha, alpha) by Johnk\'s method; alpha > 1 is not supported)')
        for name, p in (('prob', prob), ('switch_prob', switch_prob)):
            if not 0.0 <= float(p) <= 1.0:
                raise ValueError(f'BatchMix: {name} = {p} must lie in [0, 1]')
        self.mixup_alpha, self.cutmix_alpha, self.prob, self.switch_prob = float(mixup_alpha), float(cutmix_alpha), float(prob), float(switch_prob)
        seed = torch.initial_seed() if seed is None else int(seed)
        self.register_buffer('_state', torch.tensor([seed & 0x7FFFFFFFFFFFFFFF, 0, 0, 0], dtype=torch.int64), persistent=False)
        self.register_buffer('_plan', torch.zeros(PLAN_WORDS, dtype=torch.int32), persistent=False)

    def mix(self, images, labels):
        if not self.training:
            return images, labels
        require_gpu(images, 'BatchMix')
        if images.dim() != 4 or images.dtype not in (torch.float32, torch.bfloat16):
            raise RuntimeError(f'BatchMix: expected [B, C, H, W] fp32 / bf16 images, got {tuple(images.shape)} {images.dtype}')
        if not self._state.is_cuda or self._state.device != images.device:
            raise RuntimeError(f'BatchMix: its state is on {self._state.device}, the images on {images.device}: move the module with .to(device)')
        if labels.device != images.device:
            raise RuntimeError(f'BatchMix: labels are on {labels.device} but the images on {images.device}')
        B, Cc, H, W = images.shape
        if labels.numel() != B:
            raise RuntimeError(f'BatchMix: {labels.numel()} labels for {B} images')
        x = images.detach()
        x = x if x.is_contiguous() else x.contiguous()
        out = torch.empty_like(x)
        stream = _stream()
        _lib.call('fva_mix_plan', _p(self._state), self.mixup_alpha, self.cutmix_alpha, self.prob, self.switch_prob, H, W, _p(self._plan), stream)
        _lib.call('fva_mix_apply', _code(x.dtype), _p(x), _p(out), _p(self._plan), B, Cc, H, W, stream)
        return out, MixedLabels(labels, self._plan)

    forward = mix

    # ---- graphs.GraphedTrainStep: warm-up steps run on a copy of the state ---------------------------------------------
    def snapshot_state(self):
        return {'state': self._state.clone(), 'plan': self._plan.clone()}

    def restore_state(self, snap):
        """In place: the buffers keep their addresses (captured graphs stay valid)."""
        with torch.no_grad():
            self._state.copy_(snap['state'])
            self._plan.copy_(snap['plan'])
