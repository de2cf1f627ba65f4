"""The multi-tensor table protocol without a GPU (fastvision_amd/multi_tensor.py; DESIGN.md, "Multi-tensor tables"): chunk words,
the ceiling rule of the chunk counts against the chunk size the library reports, the WordTable cache on the CPU device, and the
words FusedAdam puts into its table."""
import pytest
import torch


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as ge
    ge.build()
    from fastvision_amd import _lib
    return _lib.load()


def test_chunk_words_are_tensor_and_chunk_number():
    from fastvision_amd.multi_tensor import chunk_words
    assert chunk_words((1, 1, 2, 0)) == [0, 1 << 32, 2 << 32, (2 << 32) | 1]
    assert chunk_words(()) == []


def test_both_chunk_sizes_are_the_one_constant(lib):
    assert lib.fva_sgd_chunk_elems() == lib.fva_ema_chunk_elems() > 0


def test_chunk_counts_are_ceilings_of_the_reported_chunk_size(lib):
    from fastvision_amd.multi_tensor import chunks_of
    per = lib.fva_sgd_chunk_elems()
    assert [chunks_of(n, per) for n in (5, per, per + 1)] == [1, 1, 2]                 # elements: SGD, EMA kind 0
    assert [chunks_of(n, 4 * per) for n in (8, 4 * per + 1)] == [1, 2]                 # bytes: EMA kind 1
    assert chunks_of(0, per) == 0


def test_upload_words_on_the_cpu_is_an_unpinned_copy():
    from fastvision_amd.multi_tensor import upload_words
    host, dev = upload_words([3, 1 << 40], torch.device('cpu'))
    assert not host.is_pinned() and dev.dtype == torch.int64 and dev.tolist() == [3, 1 << 40]
    out = torch.zeros(2, dtype=torch.float32)
    _, same = upload_words([0.5, 2.0], torch.device('cpu'), torch.float32, out=out)
    assert same is out and out.tolist() == [0.5, 2.0]


def test_word_table_caches_by_key():
    from fastvision_amd.multi_tensor import WordTable
    cpu, calls = torch.device('cpu'), []

    def make(words):
        def f():
            calls.append(words)
            return words
        return f

    t = WordTable('owner: no staging', capturable=True)        # capturable makes no staging off the GPU
    a = t.get(('k', 1), make([1, 2, 3]), cpu)
    assert a.tolist() == [1, 2, 3] and len(calls) == 1
    assert t.get(('k', 1), make([9, 9, 9]), cpu) is a and len(calls) == 1          # same key: same tensor, words not made again
    b = t.get(('k', 2), make([4, 5]), cpu)
    assert b is not a and b.tolist() == [4, 5] and len(calls) == 2                 # changed key: new words uploaded
    t.invalidate()
    c = t.get(('k', 2), make([4, 5]), cpu)
    assert c is not b and c.tolist() == [4, 5] and len(calls) == 3                 # invalidate() forces a rebuild
    assert t.begin_capture() == []                                                 # no staging yet: nothing to own ...
    assert t.get(('k', 2), make([6, 7]), cpu).tolist() == [6, 7] and len(calls) == 4    # ... and the cache is dropped


def test_fused_adam_table_words():
    from fastvision_amd import FusedAdam
    torch.manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(s)) for s in ((3,), (2, 5), (7,))]
    for p in ps:
        p.grad = torch.randn_like(p)
    opt = FusedAdam(ps, lr=1e-3)
    got_ps, words, n, mx = opt._table(0, opt.param_groups[0])
    m = [opt.state[p]['exp_avg'] for p in ps]
    v = [opt.state[p]['exp_avg_sq'] for p in ps]
    want = ([p.data_ptr() for p in ps] + [p.grad.data_ptr() for p in ps] + [t.data_ptr() for t in m] + [t.data_ptr() for t in v]
            + [p.numel() for p in ps])
    assert words.tolist() == want
    assert [id(p) for p in got_ps] == [id(p) for p in ps] and n == 3 and mx == 10
    assert opt._table(0, opt.param_groups[0])[1] is words                          # nothing moved: the cached table
    ps[1].grad = torch.randn_like(ps[1])
    again = opt._table(0, opt.param_groups[0])[1]
    want[3 + 1] = ps[1].grad.data_ptr()
    assert again is not words and again.tolist() == want
    with pytest.raises(RuntimeError, match='no CPU path'):                        # the table builds on CPU tensors, the step refuses them
        opt.step()
