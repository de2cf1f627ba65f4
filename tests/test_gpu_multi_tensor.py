"""The multi-tensor tables on the device (fastvision_amd/multi_tensor.py; DESIGN.md, "Multi-tensor tables"): the words FusedSGD and
ModelEMA upload, read back and compared with the words written out here, and the capture protocol of WordTable in its smallest form
(what test_gpu_graph.py::test_two_graphs_on_one_optimizer_alternate_like_eager checks end to end)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _per():
    from fastvision_amd import _lib
    return _lib.call('fva_sgd_chunk_elems')


def _param(n):
    return torch.nn.Parameter(torch.linspace(-1, 1, n, device=DEV))


def test_fused_sgd_tables_read_back():
    from fastvision_amd import FusedSGD
    per = _per()
    a, b, c, idle = _param(5), _param(per), _param(per + 1), _param(3)
    for p in (a, b, c):
        p.grad = torch.full_like(p, 0.5)
    a0, c0 = a.detach().clone(), c.detach().clone()
    opt = FusedSGD([{'params': [a, b], 'momentum': 0.9}, {'params': [idle, c]}], lr=0.1)       # idle has no gradient: slot 2, no row
    opt.step()
    ps, tab, n, chunks, clear = opt._table()
    assert [id(p) for p in ps] == [id(a), id(b), id(c)] and n == 3 and clear
    bufs = [opt.state[a]['momentum_buffer'].data_ptr(), opt.state[b]['momentum_buffer'].data_ptr(), 0]      # group 1 has no momentum
    assert 'momentum_buffer' not in opt.state[c]
    want = ([p.data_ptr() for p in ps] + [p.grad.data_ptr() for p in ps] + bufs + [5, per, per + 1] + [0, 0, 1] + [0, 1, 3])
    assert tab.tolist() == want
    assert chunks.tolist() == [0, 1 << 32, 2 << 32, (2 << 32) | 1]
    torch.cuda.synchronize()
    # the launch read these tables, to the last element of the last chunk: the first step is p - lr * grad with or without momentum
    # (0.1f * 0.5 is exact, so fused or not the update is one rounding of p - 0.05f)
    assert torch.equal(a, a0 - 0.1 * 0.5) and torch.equal(c, c0 - 0.1 * 0.5)

    opt.step()                                                                     # nothing moved: the same device tensors
    again = opt._table()
    assert again[1] is tab and again[3] is chunks

    old = c.grad
    c.grad = torch.full_like(c, 0.25)                                              # `old` stays alive: the new one has another address
    assert c.grad.data_ptr() != old.data_ptr()
    opt.step()
    moved = opt._table()
    want[3 + 2] = c.grad.data_ptr()
    assert moved[1] is not tab and moved[1].tolist() == want                       # exactly that word changed
    assert moved[3] is chunks                                                      # same sizes: same chunk table


def test_model_ema_tables_read_back():
    from fastvision_amd import ModelEMA
    per = _per()

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.linspace(-1, 1, per + 1))
            self.register_buffer('steps', torch.tensor(3, dtype=torch.int64))
            self.register_buffer('empty', torch.zeros(0))
            self.a = torch.nn.Linear(2, 2, bias=False)
            self.b = torch.nn.Linear(2, 2, bias=False)
            self.b.weight = self.a.weight                                          # one tensor under two keys

    net = Net().to(DEV)
    ema = ModelEMA(net, decay=0.5, tau=0.0)
    assert list(net.state_dict()) == ['w', 'steps', 'empty', 'a.weight', 'b.weight']
    e0 = ema.module.w.clone()                  # multiples of 2^-13 (per = 2^14): the update below is exact in fp32
    with torch.no_grad():
        net.w.add_(2.0)
        net.steps.add_(4)
    ema.update(net)
    t = ema._tab
    own, theirs = ema.module, net
    rows = [(own.w, theirs.w, per + 1, 0), (own.steps, theirs.steps, 8, 1), (own.a.weight, theirs.a.weight, 4, 0)]   # empty, b.weight: no row
    assert t['n'] == 3 and t['nchunks'] == 4
    assert t['tab'].tolist() == ([e.data_ptr() for e, _, _, _ in rows] + [p.data_ptr() for _, p, _, _ in rows]
                                 + [r[2] for r in rows] + [r[3] for r in rows])
    assert t['chunks'].tolist() == [0, 1, 1 << 32, 2 << 32]                        # w: two chunks of elements; steps: one of bytes
    torch.cuda.synchronize()
    assert torch.equal(own.w, e0 + 0.5 * 2.0) and int(own.steps) == 7              # e += 0.5 * (p - e); steps copied
    assert ema.begin_capture()[0] is t['tab']                                      # what a graph keeps alive
    ema.update(net)
    assert ema._tab is t                                                           # nothing moved: the same tables


def test_word_table_capture_protocol():
    from fastvision_amd.multi_tensor import WordTable
    dev = torch.device(DEV)
    out = torch.zeros(3, dtype=torch.int64, device=dev)
    plain = WordTable('owner: run an eager step first')                            # no staging, ever
    plain.get('eager', lambda: [1, 2], dev)
    with pytest.raises(RuntimeError, match='owner: run an eager step first'):
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            out.zero_()                                                            # (a graph with one node in it)
            plain.get('new key', lambda: [3, 4], dev)

    table = WordTable('owner: run an eager step first', capturable=True)
    assert table.begin_capture() == []                                             # before the first eager get: nothing to own
    out.copy_(table.get('eager', lambda: [1, 2, 3], dev))                          # makes the staging a capture writes into
    captured = []
    for words in ([10, 11, 12], [20, 21, 22]):
        (stage,) = table.begin_capture()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            tab = table.get(('captured', words[0]), lambda: words, dev)
            out.copy_(tab)
        assert stage[0].is_pinned() and tab is stage[1] and stage[0].tolist() == words
        captured.append((graph, stage))
    (g1, s1), (g2, s2) = captured
    assert s1[0].data_ptr() != s2[0].data_ptr() and s1[1].data_ptr() != s2[1].data_ptr()
    for graph, stage, want in ((g1, s1, [10, 11, 12]), (g2, s2, [20, 21, 22]), (g1, s1, [10, 11, 12])):
        stage[1].zero_()                                                           # the replay uploads its own words again
        graph.replay()
        torch.cuda.synchronize()
        assert out.tolist() == want
    s1[0][0] = 99                                                                  # the copy node re-reads the pinned words
    g1.replay()
    torch.cuda.synchronize()
    assert out.tolist() == [99, 11, 12] and s2[0].tolist() == [20, 21, 22]
    with pytest.raises(RuntimeError, match='owner: run an eager step first'):      # staging of another size is no staging
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            out.zero_()
            table.get('longer', lambda: [1, 2, 3, 4], dev)
