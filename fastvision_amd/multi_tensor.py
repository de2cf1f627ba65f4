"""Host side of the multi-tensor launches (FusedAdam, FusedSGD, ModelEMA): small int64 device tables of pointers, sizes and chunk
words.  DESIGN.md ("Multi-tensor tables") states the protocol; this module is its only implementation."""
import torch


def capturing(device):
    """True while the current stream of a GPU ``device`` records a graph (never on the CPU)."""
    return device.type == 'cuda' and torch.cuda.is_current_stream_capturing()


def upload_words(words, device, dtype=torch.int64, out=None):
    """(host tensor, device tensor) of ``words``, copied on the current stream without stalling the host: the host tensor is pinned
    when ``device`` is a GPU (a pageable copy would wait for the stream).  ``out``: a device tensor to refill instead of a new one
    (captured graphs read its address).  The host words need NOT outlive the call: torch's pinned-memory allocator records the stream
    of a non-blocking copy and hands the block out again only after that copy has run."""
    host = torch.tensor(words, dtype=dtype)
    if device.type == 'cuda':
        host = host.pin_memory()
    return host, host.to(device, non_blocking=True) if out is None else out.copy_(host, non_blocking=True)


def chunks_of(count, per):
    """Chunks of ``per`` units (elements or bytes) in a tensor of ``count`` units."""
    return (count + per - 1) // per


def chunk_words(chunks_per_tensor):
    """One word ``(tensor << 32) | chunk`` per block, tensor by tensor (decoded by csrc/multi_tensor.h)."""
    return [(t << 32) | c for t, k in enumerate(chunks_per_tensor) for c in range(k)]


class WordTable:
    """A cached int64 device table.  ``capture_error``: the owner's message for a rebuild inside a graph capture that finds no staging
    of the right size; only a ``capturable`` owner ever has staging."""

    def __init__(self, capture_error, capturable=False):
        self.capture_error, self.capturable = capture_error, capturable
        self._key = self._dev = self._stage = None

    def _restage(self, n, device):
        self._stage = torch.empty(n, dtype=torch.int64).pin_memory(), torch.empty(n, dtype=torch.int64, device=device)

    def get(self, key, make_words, device):
        """The device tensor of ``make_words()``, cached while ``key`` is unchanged."""
        if self._dev is None or self._key != key:
            if capturing(device):      # allocate nothing: write the staging words; the recorded copy re-reads them on every replay
                words = make_words() if self._stage is not None else ()
                if self._stage is None or self._stage[0].numel() != len(words):
                    raise RuntimeError(self.capture_error)
                self._stage[0].copy_(torch.tensor(words, dtype=torch.int64))
                dev = self._stage[1].copy_(self._stage[0], non_blocking=True)
            else:
                words = make_words()
                dev = upload_words(words, device)[1]
                if self.capturable and device.type == 'cuda' and (self._stage is None or self._stage[0].numel() != len(words)):
                    self._restage(len(words), device)
            self._key, self._dev = key, dev
        return self._dev

    def invalidate(self):
        self._key = self._dev = None

    def begin_capture(self):
        """Fresh [(pinned, device)] staging of the same size for ONE graph, whose owner keeps it alive ([] before an eager step made
        staging); drops the cache, so that the capture-time step writes its own words and records their upload."""
        self.invalidate()
        if self._stage is None:
            return []
        self._restage(self._stage[0].numel(), self._stage[1].device)
        return [self._stage]
