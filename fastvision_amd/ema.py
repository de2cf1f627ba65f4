"""ModelEMA: the exponential moving average of a model's weights that a YOLO trainer validates and checkpoints instead of the raw
model, as ONE multi-tensor HIP launch per step (``fva_ema_update``: a tick kernel + one chunked launch over every tensor of the
state dict) instead of ~2 x 440 ATen launches from Python.

    ema = ModelEMA(model, decay=0.9999, tau=2000.0)
    ...
    optimizer.step()
    ema.update(model)                 # e += w * (p - e),  w = 1 - decay * (1 - exp(-updates / tau))
    ...
    validate(ema.module)              # the averaged model, in eval mode

The update counter and the weight of the current update live in device memory (the kernel advances them), so a training step captured
in a HIP graph (graphs.GraphedTrainStep(..., ema=ema)) replays with the right ramp; nothing is read back, ``update`` never
synchronises the host (``ema.updates`` is the one place that does).  fp32 tensors are averaged; every other tensor of the state dict
(``num_batches_tracked``, integer / bool / non-fp32 float buffers) is copied from the model, so a checkpoint of the average is
consistent with the model it follows.  After an update the autograd version counters of the averaged model's tensors are advanced:
its packed MFMA weights and eval-mode BatchNorm coefficients (both cached by version) are rebuilt at its next forward.
"""
import ctypes as C
import math
import weakref
from copy import deepcopy

import torch

from . import _lib
from .multi_tensor import WordTable, chunk_words, chunks_of, upload_words
from .ops import _stream, require_gpu

__all__ = ['ModelEMA']


def _slots_of(model, tensors):
    """Where ``model`` holds each of ``tensors`` (its state-dict values): [(a module's _parameters / _buffers dict, name)], or None when
    one of them is not held that way (a custom state_dict): then every update pairs the state dicts anew."""
    where = {}
    for m in model.modules():
        for d in (m._parameters, m._buffers):
            for name, t in d.items():
                if t is not None:
                    where.setdefault(id(t), (d, name))
    slots = [where.get(id(t)) for t in tensors]
    return None if any(s is None for s in slots) else slots


def _unwrap(model):
    from .utils.checkpoints import is_parallel
    return model.module if is_parallel(model) else model


def build_tables(pairs, table=None, key=None):
    """The device tables of ``fva_ema_update`` for ``pairs`` = [(name, EMA tensor, model tensor)]: (table int64 [4][n] = EMA pointer |
    model pointer | count | kind, n, chunk table, nchunks, the host words or None), uploaded at once or through the WordTable ``table``
    (cached by ``key``).  fp32 pairs are averaged (kind 0, count in elements), all others copied (kind 1, count in bytes, four times
    as many to a chunk); pairs whose EMA tensor was already listed (tied tensors appear under several keys) and empty tensors are
    left out."""
    per = _lib.call('fva_ema_chunk_elems')
    rows, seen = [], set()
    for k, e, p in pairs:
        require_gpu(e, 'ModelEMA')
        require_gpu(p, 'ModelEMA')
        if p.shape != e.shape or p.dtype != e.dtype or p.device != e.device:
            raise RuntimeError(f'ModelEMA: {k} is {tuple(p.shape)} {p.dtype} on {p.device} in the model, '
                               f'{tuple(e.shape)} {e.dtype} on {e.device} in the average')
        if not p.is_contiguous() or not e.is_contiguous():
            raise RuntimeError(f'ModelEMA needs contiguous parameters and buffers ({k})')
        if e.numel() == 0 or e.data_ptr() in seen:
            continue
        seen.add(e.data_ptr())
        if e.dtype == torch.float32:
            rows.append((e.data_ptr(), p.data_ptr(), e.numel(), 0, per))
        else:
            rows.append((e.data_ptr(), p.data_ptr(), e.numel() * e.element_size(), 1, 4 * per))
    if not rows:
        raise RuntimeError('ModelEMA: nothing to average')
    n, dev = len(rows), pairs[0][1].device
    words = [r[c] for c in range(4) for r in rows] + chunk_words(chunks_of(r[2], r[4]) for r in rows)
    host, both = upload_words(words, dev) if table is None else (None, table.get(key, lambda: words, dev))
    return both[:4 * n], n, both[4 * n:], len(words) - 4 * n, host


class ModelEMA:
    def __init__(self, model, decay=0.9999, tau=2000.0, updates=0):
        decay, tau = float(decay), float(tau)
        if not 0.0 <= decay < 1.0:
            raise ValueError(f'ModelEMA: decay must be in [0, 1) (got {decay})')
        if not tau >= 0.0:
            raise ValueError(f'ModelEMA: tau must be >= 0 (got {tau})')
        if int(updates) < 0:
            raise ValueError(f'ModelEMA: updates must be >= 0 (got {updates})')
        model = _unwrap(model)
        tensors = list(model.state_dict(keep_vars=True).values())
        if not tensors:
            raise ValueError('ModelEMA: the model has no parameters or buffers')
        for t in tensors:
            require_gpu(t, 'ModelEMA')
            if not t.is_contiguous():
                raise RuntimeError('ModelEMA needs contiguous parameters and buffers')
        self.decay, self.tau = decay, tau
        self.module = deepcopy(model).eval()
        self.module.requires_grad_(False)
        self._device = tensors[0].device
        self._state = torch.tensor([float(int(updates)), 1.0], dtype=torch.float64).to(self._device)      # updates done | weight of the last update
        self._own = None          # tensors of the averaged model, in state-dict order (they keep their addresses)
        self._tab = None          # the device tables of the last pairing (see _table)
        self._words = WordTable('ModelEMA: run at least one eager update(model) before capturing a graph')      # no staging: see begin_capture

    # ---- the ramp ----------------------------------------------------------------------------------------------------
    def weight(self, k):
        """w = 1 - d of update number ``k`` (1-based), as the tick kernel computes it."""
        d = self.decay * (1.0 - math.exp(-k / self.tau)) if self.tau > 0 else self.decay
        return 1.0 - d

    @property
    def updates(self):
        """Updates done: reads the device counter (synchronises the host)."""
        return int(self._state[0].item())

    # ---- tables ------------------------------------------------------------------------------------------------------
    def _tensors(self):
        if self._own is None:
            self._own = self.module.state_dict(keep_vars=True)
        return self._own

    def _table(self, model):
        """Device table [4][n] = EMA pointer | model pointer | count | kind and the chunk table: the two state dicts paired by key once,
        rebuilt only when a tensor of either side was replaced or moved.  Between rebuilds an update costs one identity check and one
        ``data_ptr()`` per tensor, not two walks over the module trees."""
        base = _unwrap(model)
        hit = self._tab
        if hit is not None and hit['model']() is base and hit['slots'] is not None:
            own, theirs = hit['own'], hit['theirs']
            if all(d.get(name) is t for (d, name), t in zip(hit['slots'], theirs)):      # no parameter / buffer object was replaced
                if [t.data_ptr() for t in own] + [t.data_ptr() for t in theirs] == hit['key']:
                    return hit
        own, theirs = self._tensors(), base.state_dict(keep_vars=True)
        if len(own) != len(theirs):
            raise RuntimeError(f'ModelEMA.update: the model has {len(theirs)} state-dict entries, the average {len(own)}')
        missing = [k for k in own if k not in theirs]
        if missing:
            raise RuntimeError(f'ModelEMA.update: the model has no state-dict entry {missing[0]!r}')
        pairs = [(k, e, theirs[k]) for k, e in own.items()]
        key = [e.data_ptr() for _, e, _ in pairs] + [p.data_ptr() for _, _, p in pairs]
        # other tensor objects over the same memory, shapes and types find the device words cached: only the quick check's objects change
        tab, n, chunks, nchunks, _ = build_tables(pairs, self._words, (key, [(p.shape, p.dtype) for _, _, p in pairs]))
        self._tab = {'key': key, 'tab': tab, 'n': n, 'chunks': chunks, 'nchunks': nchunks, 'model': weakref.ref(base),
                     'own': [e for _, e, _ in pairs], 'theirs': [p for _, _, p in pairs], 'slots': _slots_of(base, [p for _, _, p in pairs])}
        return self._tab

    # ---- the update --------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def update(self, model):
        """One update from ``model`` (call it after ``optimizer.step()``), on the current stream; no host synchronisation."""
        t = self._table(model)
        _lib.call('fva_ema_update', C.c_void_p(t['tab'].data_ptr()), t['n'], C.c_void_p(t['chunks'].data_ptr()), t['nchunks'], self.decay,
                  self.tau, C.c_void_p(self._state.data_ptr()), _stream())
        self.bump_versions()

    def bump_versions(self):
        """The kernel wrote the averaged model in place (also: a graph replay did): invalidate what is cached by version."""
        torch.autograd.graph.increment_version(self._tensors().values())

    # ---- checkpoints -------------------------------------------------------------------------------------------------
    def state_dict(self):
        return {'module': self.module.state_dict(), 'updates': self.updates, 'decay': self.decay, 'tau': self.tau}

    def load_state_dict(self, sd):
        self.module.load_state_dict(sd['module'])          # in-place copies: addresses stay, versions advance
        self.decay, self.tau = float(sd['decay']), float(sd['tau'])
        self._state.copy_(torch.tensor([float(int(sd['updates'])), self.weight(max(int(sd['updates']), 1))], dtype=torch.float64))
        self._own = None

    # ---- graphs.GraphedTrainStep -------------------------------------------------------------------------------------
    def begin_capture(self):
        """What a graph that captures ``update`` must keep alive: the device tables of the last eager update.  They are built once
        per pairing and never rewritten, so graphs share them and there is no staging ("Multi-tensor tables")."""
        return [] if self._tab is None else [self._tab['tab'], self._tab['chunks']]

    def snapshot_state(self):
        """A device copy of the averaged model's tensors and of the device counter."""
        return {'tensors': [t.detach().clone() for t in self._tensors().values()], 'state': self._state.clone()}

    def restore_state(self, snap):
        """Put back what ``snapshot_state`` copied, in place: the tensors keep their addresses (captured graphs stay valid)."""
        with torch.no_grad():
            for t, v in zip(self._tensors().values(), snap['tensors']):
                t.copy_(v)
            self._state.copy_(snap['state'])
