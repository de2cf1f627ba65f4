"""FusedAdam: torch.optim.Adam semantics (the optimizer the reference builds, demos/yolov3_u/train.py:66-70) as
ONE multi-tensor HIP launch per step (``fva_adam_step``) instead of ~10 foreach kernels over 222 tensors.

Drop-in for ``torch.optim.Adam(params, lr, betas, eps, weight_decay)`` (no amsgrad / maximize).  State lives in the
usual ``state[p] = {'step', 'exp_avg', 'exp_avg_sq'}`` entries; ``state_dict()`` / ``load_state_dict()`` exchange
checkpoints with torch's Adam in both directions (torch stores ``step`` as a float tensor: it is coerced on use).

``capturable=True`` keeps the step count and the learning rate in device memory (``fva_adam_step_dev``) so that the
whole training step can be captured in a HIP graph (graphs.GraphedTrainStep): a replay advances the device counter
itself and reads the current learning rate from a device scalar that ``step()`` / the graph wrapper refresh whenever
``param_groups[i]['lr']`` changes (LR schedules keep working).
"""
import ctypes as C

import torch

from . import _lib
from .multi_tensor import WordTable, capturing, chunk_words, chunks_of, upload_words
from .ops import _stream, join_side_stream

__all__ = ['FusedAdam', 'FusedSGD']


class _FusedOptimizer(torch.optim.Optimizer):
    """The frame of ``step()`` that the two optimizers share; ``_launch()`` returns the parameters its kernels wrote."""

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        join_side_stream()          # weight gradients may still be in flight on the library's side stream
        torch.autograd.graph.increment_version(self._launch())      # written in place: invalidate packed-weight caches
        return loss


class FusedAdam(_FusedOptimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, grad_scale=1.0, capturable=False):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.grad_scale = grad_scale
        self.capturable = capturable
        self._tables = {}         # group index -> WordTable of [4][n] pointers + sizes
        self._max = {}            # group index -> largest tensor of that table
        self._dev = {}            # group index -> {'state': double[3], 'lr': float[1], 'lr_host': float}

    # ---- checkpoints -------------------------------------------------------------------------------------------------
    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for t in self._tables.values():           # the moment tensors were replaced: pointer tables are stale
            t.invalidate()
        for gi, d in self._dev.items():           # device step counters follow the loaded step
            ps = [p for p in self.param_groups[gi]['params'] if p in self.state and self.state[p]]
            if ps:
                d['state'][0] = float(self._step_of(ps[0]))
                d['lr_host'] = None

    def _step_of(self, p):
        st = self.state[p].get('step', 0)
        return int(st.item()) if torch.is_tensor(st) else int(st)

    # ---- pointer table -----------------------------------------------------------------------------------------------
    def _table(self, gi, group):
        """(parameters with a gradient, device words [4][n] = param | grad | exp_avg | exp_avg_sq followed by n sizes, n, largest
        size), rebuilt only when a parameter, gradient or moment tensor moved.  Gradients are fresh tensors every step, so eager
        training re-uploads this small table every step."""
        ps = [p for p in group['params'] if p.grad is not None]
        for p in ps:
            st = self.state[p]
            if not st:
                st['step'] = 0
                st['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
            if p.dtype != torch.float32 or not p.is_contiguous() or not p.grad.is_contiguous() or p.grad.dtype != torch.float32:
                raise RuntimeError('FusedAdam needs contiguous fp32 parameters and gradients')
        key = tuple((p.data_ptr(), p.grad.data_ptr(), self.state[p]['exp_avg'].data_ptr(), self.state[p]['exp_avg_sq'].data_ptr())
                    for p in ps)

        def words():
            sizes = [p.numel() for p in ps]
            self._max[gi] = max(sizes)
            return [k[c] for c in range(4) for k in key] + sizes

        if gi not in self._tables:
            self._tables[gi] = WordTable('FusedAdam: run at least one eager step() (capturable=True) and begin_capture() before '
                                         'capturing a graph', self.capturable)
        return ps, self._tables[gi].get(key, words, ps[0].device), len(ps), self._max[gi]

    def begin_capture(self):
        """This graph's own staging for every group's table, as [(pinned, device)] ("Multi-tensor tables")."""
        return [s for t in self._tables.values() for s in t.begin_capture()]

    def _dev_state(self, gi, group, dev):
        d = self._dev.get(gi)
        if d is None:
            d = self._dev[gi] = {'state': torch.zeros(3, dtype=torch.float64, device=dev),
                                 'lr': torch.zeros(1, dtype=torch.float32, device=dev), 'lr_host': None}
            started = [p for p in group['params'] if p in self.state and self.state[p]]
            if started:
                d['state'][0] = float(self._step_of(started[0]))
        return d

    def sync_lr(self):
        """Refresh the device learning-rate scalars from param_groups (capturable mode; call between graph replays -- the graph
        wrapper does -- after an LR scheduler changed them).  One tiny fill kernel per changed group, no host sync."""
        for gi, group in enumerate(self.param_groups):
            d = self._dev.get(gi)
            if d is not None and d['lr_host'] != group['lr']:
                d['lr'].fill_(float(group['lr']))
                d['lr_host'] = group['lr']

    def note_replayed_steps(self, k=1):
        """Host mirrors of the step count after ``k`` replays of a captured step (the device counter advanced by itself)."""
        for group in self.param_groups:
            for p in group['params']:
                st = self.state.get(p)
                if st:
                    st['step'] = self._step_of(p) + k

    # ---- graphs.GraphedTrainStep --------------------------------------------------------------------------------------
    def snapshot_state(self):
        """A device copy of the optimizer state a training step changes: moments, host step counts and device step counters."""
        started = [p for g in self.param_groups for p in g['params'] if self.state.get(p)]
        return {'moments': {p: (self.state[p]['exp_avg'].clone(), self.state[p]['exp_avg_sq'].clone(), self._step_of(p)) for p in started},
                'dev': {gi: d['state'].clone() for gi, d in self._dev.items()}}

    def restore_state(self, snap):
        """Put back what ``snapshot_state`` copied, in place (the tensors keep their addresses: captured graphs stay valid)."""
        for p in (p for g in self.param_groups for p in g['params']):
            st = self.state.get(p)
            if not st:
                continue
            if p in snap['moments']:
                m, v, k = snap['moments'][p]
                st['exp_avg'].copy_(m)
                st['exp_avg_sq'].copy_(v)
                st['step'] = k
            else:                                   # state born after the snapshot: back to a fresh optimizer's zeros
                st['exp_avg'].zero_()
                st['exp_avg_sq'].zero_()
                st['step'] = 0
        for gi, d in self._dev.items():
            if gi in snap['dev']:
                d['state'].copy_(snap['dev'][gi])
            else:
                d['state'].zero_()

    def host_state(self):
        """What the host side of one ``step()`` changes (the step counts): saved before a capture, put back after it."""
        return [(p, self._step_of(p)) for g in self.param_groups for p in g['params'] if self.state.get(p)]

    def set_host_state(self, saved):
        for p, k in saved:
            self.state[p]['step'] = k

    def _launch(self):
        written = []
        for gi, group in enumerate(self.param_groups):
            if not any(p.grad is not None for p in group['params']):
                continue
            ps, words, n, mx = self._table(gi, group)
            if not ps[0].is_cuda:
                raise RuntimeError('FusedAdam: parameters must live on the GPU (no CPU path)')
            tab, sizes = C.c_void_p(words.data_ptr()), C.c_void_p(words.data_ptr() + 32 * n)
            d = self._dev_state(gi, group, ps[0].device) if self.capturable else None     # starts from the host step count: before it moves
            step = self._step_of(ps[0]) + 1
            for p in ps:
                self.state[p]['step'] = step
            b1, b2 = group['betas']
            if self.capturable:
                if not capturing(ps[0].device) and d['lr_host'] != group['lr']:
                    d['lr'].fill_(float(group['lr']))
                    d['lr_host'] = group['lr']
                _lib.call('fva_adam_step_dev', tab, sizes, n, mx, C.c_void_p(d['lr'].data_ptr()),
                          b1, b2, group['eps'], group['weight_decay'], C.c_void_p(d['state'].data_ptr()), self.grad_scale, _stream())
            else:
                _lib.call('fva_adam_step', tab, sizes, n, mx, group['lr'], b1, b2,
                          group['eps'], group['weight_decay'], step, self.grad_scale, _stream())
            written += ps
        return written


class FusedSGD(_FusedOptimizer):
    """torch.optim.SGD semantics (the optimizer of the reference's Faster R-CNN demo, demos/faster_rcnn/train.py:91-109: momentum
    0.937, Nesterov, parameter groups) as ONE multi-tensor HIP launch per step for every group (``fva_sgd_step``), with the demo's
    gradient-norm clipping (cfg/_fit.py:6-17) optionally on the device.

    Drop-in for ``torch.optim.SGD(params, lr, momentum, dampening, weight_decay, nesterov)``: same argument checks, same update
    order (single-tensor path of torch/optim/sgd.py), same state (``state[p]['momentum_buffer']``, no entry when momentum is 0), so
    ``state_dict()`` / ``load_state_dict()`` exchange checkpoints with torch's SGD in both directions.  Parameters whose ``.grad`` is
    None are skipped as torch skips them: no buffer, nothing added to the norm (the reference's clip_gradient would fail on them).

    ``clip_norm``: ``step()`` first computes the global L2 norm of all groups' gradients (``fva_sgd_clip_coef``: fp64 per chunk,
    fixed order, no atomics) and the reference's coefficient ``clip_norm / max(norm, clip_norm)`` into device scalars, then the
    update multiplies each gradient by it as it reads it.  Nothing is read back: no host synchronisation.  ``p.grad`` itself is NOT
    rewritten (the reference scales it in place); ``last_grad_norm`` is the fp32 device scalar of the norm (overwritten by the next
    step).  A non-finite norm behaves as the reference: NaN gives NaN parameters, infinity a coefficient of 0.

    ``capturable=True`` serves graphs.GraphedTrainStep (the table protocol: DESIGN.md, "Multi-tensor tables"): the hyper-parameters
    (lr of each group) live in a device table that ``step()`` / ``sync_lr()`` refresh when ``param_groups`` change, and at least one
    eager ``step()`` must run before a capture.  Whether a momentum buffer still has to be initialised is a device flag, so a
    captured step restored to a fresh optimizer's state initialises it exactly once.
    Parameters and gradients must be contiguous fp32 tensors on the GPU (no CPU path).  ``lr`` defaults to 1e-3 as in torch's SGD;
    ``maximize``, ``foreach``, ``fused`` and ``differentiable`` are accepted only at torch's defaults (False, None, None, False):
    any other value, ``foreach=False`` included, is refused rather than silently ignored.
    """

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, clip_norm=None, capturable=False,
                 *, maximize=False, foreach=None, differentiable=False, fused=None):
        if maximize is not False or differentiable is not False or foreach is not None or fused is not None:
            raise ValueError('FusedSGD: maximize, foreach, fused and differentiable are not supported (it is its own fused kernel); '
                             'leave them at their defaults (False, None, None, False)')
        if torch.is_tensor(lr) and lr.numel() != 1:
            raise ValueError('Tensor lr must be 1-element')
        if lr < 0.0:
            raise ValueError(f'Invalid learning rate: {lr}')
        if momentum < 0.0:
            raise ValueError(f'Invalid momentum value: {momentum}')
        if weight_decay < 0.0:
            raise ValueError(f'Invalid weight_decay value: {weight_decay}')
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError('Nesterov momentum requires a momentum and zero dampening')
        if clip_norm is not None and not (0.0 < float(clip_norm) < float('inf')):
            raise ValueError(f'Invalid clip_norm value: {clip_norm}')
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                                      maximize=False, foreach=None, differentiable=False, fused=None))
        self.clip_norm = None if clip_norm is None else float(clip_norm)
        self.capturable = capturable
        self._tab = WordTable('FusedSGD: run at least one eager step() (capturable=True) and begin_capture() before capturing a graph',
                              capturable)                                                              # [6][n], see _table
        self._chunks = WordTable('FusedSGD: run at least one eager step() before capturing a graph')   # one word per block
        self._partial = None      # device double per chunk: the clipping norm's partial sums
        self._hyper = None        # (host values, device float [G][5])
        self._fresh = None        # device int32 per parameter slot: the momentum buffer has no history yet
        self._clip_out = None     # device float [2]: norm, coefficient

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:
            group.setdefault('nesterov', False)

    # ---- checkpoints -------------------------------------------------------------------------------------------------
    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._tab.invalidate()                    # the buffers were replaced: the pointer table is stale
        for p, st in self.state.items():          # a loaded buffer has history (torch's SGD continues it)
            buf = st.get('momentum_buffer')
            if buf is not None and not buf.is_contiguous():
                st['momentum_buffer'] = buf.contiguous()
        if self._fresh is not None:
            self._fresh.zero_()

    @property
    def last_grad_norm(self):
        """fp32 device scalar of the global gradient norm of the last clipped step (None before one)."""
        return None if self._clip_out is None else self._clip_out[0]

    # ---- tables ------------------------------------------------------------------------------------------------------
    def _params(self):
        return [p for g in self.param_groups for p in g['params']]

    def _slots(self, dev):
        allp = self._params()
        if self._fresh is None or self._fresh.numel() < len(allp):
            fresh = torch.zeros(len(allp), dtype=torch.int32, device=dev)
            if self._fresh is not None:
                fresh[:self._fresh.numel()].copy_(self._fresh)
            self._fresh = fresh
        return {p: i for i, p in enumerate(allp)}

    def _sync_hyper(self, dev):
        vals = []
        for g in self.param_groups:
            vals += [float(g['lr']), float(g['weight_decay']), float(g['momentum']), 1.0 - float(g['dampening']), 1.0 if g['nesterov'] else 0.0]
        vals = tuple(vals)
        if self._hyper is not None and self._hyper[0] == vals:
            return
        if capturing(dev):
            raise RuntimeError('FusedSGD: hyper-parameters changed during a graph capture; call sync_lr() before capturing')
        same = self._hyper is not None and self._hyper[1].numel() == len(vals)       # captured steps read this address: refill it
        self._hyper = (vals, upload_words(vals, dev, torch.float32, out=self._hyper[1] if same else None)[1])

    def sync_lr(self):
        """Refresh the device hyper-parameter table from param_groups (capturable mode; graphs.GraphedTrainStep calls it before each
        replay, after an LR scheduler changed them).  One small asynchronous upload when something changed, no host sync."""
        if self._hyper is not None:
            self._sync_hyper(self._hyper[1].device)

    def _table(self):
        """(parameters that have a gradient (all groups), their device table [6][n] = param | grad | momentum buffer (0: none) | size |
        group | fresh-flag slot, n, chunk table, any momentum buffer), each table rebuilt only when its words changed."""
        ps, gids = [], []
        for gi, group in enumerate(self.param_groups):
            for p in group['params']:
                if p.grad is None:
                    continue
                if not p.is_cuda:
                    raise RuntimeError('FusedSGD: parameters must live on the GPU (no CPU path)')
                if p.dtype != torch.float32 or p.grad.dtype != torch.float32 or not p.is_contiguous() or not p.grad.is_contiguous():
                    raise RuntimeError('FusedSGD needs contiguous fp32 parameters and gradients')
                if p.grad.is_sparse:
                    raise RuntimeError('FusedSGD does not support sparse gradients')
                ps.append(p)
                gids.append(gi)
        if not ps:
            return None
        dev = ps[0].device
        slots = self._slots(dev)
        born = []
        for p, gi in zip(ps, gids):
            if self.param_groups[gi]['momentum'] != 0 and self.state[p].get('momentum_buffer') is None:
                if capturing(dev):
                    raise RuntimeError(self._tab.capture_error)
                self.state[p]['momentum_buffer'] = torch.empty_like(p, memory_format=torch.contiguous_format)
                born.append(slots[p])
        if born:                                  # their first update is torch's clone(grad)
            self._fresh.index_fill_(0, upload_words(born, dev)[1], 1)
        bufs = [self.state[p]['momentum_buffer'].data_ptr() if self.param_groups[gi]['momentum'] != 0 else 0 for p, gi in zip(ps, gids)]
        key = (tuple(p.data_ptr() for p in ps), tuple(p.grad.data_ptr() for p in ps), tuple(bufs), tuple(gids))
        sizes = tuple(p.numel() for p in ps)

        def chunk_table():
            per = _lib.call('fva_sgd_chunk_elems')
            words = chunk_words(chunks_of(n, per) for n in sizes)
            self._partial = torch.empty(len(words), dtype=torch.float64, device=dev)
            return words

        chunks = self._chunks.get(sizes, chunk_table, dev)
        tab = self._tab.get(key, lambda: [w for col in key[:3] for w in col] + list(sizes) + list(gids) + [slots[p] for p in ps], dev)
        # the device flags are the only record of which buffers still need torch's clone(grad): every update that has momentum
        # buffers clears the flags of its tensors afterwards (one tiny launch, idempotent), so eager steps, captured steps and
        # replays after restore_state() all agree without any host-side bookkeeping
        return ps, tab, len(ps), chunks, any(b != 0 for b in bufs)

    def begin_capture(self):
        """This graph's own staging for the pointer table, as [(pinned, device)] ("Multi-tensor tables")."""
        return self._tab.begin_capture()

    # ---- graphs.GraphedTrainStep --------------------------------------------------------------------------------------
    def snapshot_state(self):
        """A device copy of the momentum buffers and their fresh flags."""
        started = [p for p in self._params() if self.state.get(p, {}).get('momentum_buffer') is not None]
        return {'bufs': {p: self.state[p]['momentum_buffer'].clone() for p in started},
                'fresh': None if self._fresh is None else self._fresh.clone()}

    def restore_state(self, snap):
        """Put back what ``snapshot_state`` copied, in place.  A buffer born after the snapshot keeps its address and is flagged
        fresh again: the next update initialises it as a new optimizer's first step would."""
        if self._fresh is not None:
            if snap['fresh'] is not None:
                self._fresh[:snap['fresh'].numel()].copy_(snap['fresh'])
            else:
                self._fresh.zero_()
        slots = self._slots(self._fresh.device) if self._fresh is not None else {}
        born = []
        for p in self._params():
            buf = self.state.get(p, {}).get('momentum_buffer')
            if buf is None:
                continue
            if p in snap['bufs']:
                buf.copy_(snap['bufs'][p])
            else:
                buf.zero_()
                born.append(slots[p])
        if born:
            self._fresh.index_fill_(0, torch.tensor(born, dtype=torch.int64, device=self._fresh.device), 1)

    def host_state(self):
        return None                       # the host side of step() keeps no counters

    def set_host_state(self, saved):
        pass

    def note_replayed_steps(self, k=1):
        pass

    def _launch(self):
        got = self._table()
        if got is None:
            return []
        ps, tab, n, chunks, clear = got
        dev = ps[0].device
        self._sync_hyper(dev)
        tab, chunks, nchunks = C.c_void_p(tab.data_ptr()), C.c_void_p(chunks.data_ptr()), chunks.numel()
        coef = C.c_void_p(0)
        if self.clip_norm is not None:
            if self._clip_out is None:
                if capturing(dev):
                    raise RuntimeError('FusedSGD: run at least one eager step() before capturing a graph')
                self._clip_out = torch.zeros(2, dtype=torch.float32, device=dev)
            _lib.call('fva_sgd_clip_coef', tab, n, chunks, nchunks, C.c_void_p(self._partial.data_ptr()), self.clip_norm,
                      C.c_void_p(self._clip_out.data_ptr()), _stream())
            coef = C.c_void_p(self._clip_out.data_ptr() + 4)
        _lib.call('fva_sgd_step', tab, n, chunks, nchunks, C.c_void_p(self._hyper[1].data_ptr()), C.c_void_p(self._fresh.data_ptr()),
                  1 if clear else 0, coef, _stream())
        return ps
