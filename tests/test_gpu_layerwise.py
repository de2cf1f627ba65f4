"""FusedLARS / FusedLAMB on the GPU (fva_lars_step, fva_lamb_step) against a plain float64 restatement of their update rules on the
same fp32 inputs: the update over the sizes at which the chunked kernels change path, bit-identical runs, a captured step against eager
steps, and checkpoint exchange with FusedAdam / torch.optim.SGD."""
import copy
import functools
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CHUNK = 16384                                     # MT_CHUNK (asserted against the library below)
BIG = 262 * CHUNK + 3                             # more chunks than the trust block has threads (256)
SIZES_A = [1, 255, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5, BIG, 300, 300, 7]      # group 0: trust ratio on
ZERO_P, ZERO_G, NO_G = 7, 8, 9                    # all-zero parameter, all-zero gradient, .grad is None
SIZES_B = [513, 1]                                # group 1: trust ratio off, no decay, its own lr
STEPS, LR_B, ETA, LARS_EPS, LAMB_EPS, BETAS = 3, 0.03, 0.05, 1e-8, 1e-6, (0.9, 0.999)
LARS = [dict(lr=0.5, momentum=m, nesterov=n, wd=wd, clip=c) for (m, n), wd, c in
        itertools.product([(0.0, False), (0.9, False), (0.9, True)], [0.0, 5e-4], [None, 10.0])]
LAMB = [dict(lr=0.01, wd=wd, clip=c) for wd, c in itertools.product([0.0, 1e-2], [None, 10.0])]
CASES = [('lars', c) for c in LARS] + [('lamb', c) for c in LAMB]
# Largest distance of the SAME restatement (reference() below) evaluated in float32 on the CPU from its float64 evaluation, over the
# cases of each optimizer, in units of 2^-24 * magnitude.  Magnitudes: p: |p| + the sum over the three steps of |lr * update| (with the
# last step's update alone, the few elements of the 4.3 M whose third update happens to be tiny carry the error of the first two: the
# float32 figure becomes 97 471 / 1 424 497 and the bound loose everywhere else); a state tensor: the magnitudes of its terms carried
# through its recurrence; the ratio: itself.  Measured: LARS p 340.8, state 293.3, ratio 313.8; LAMB p 8777.2, state 7.94, ratio 330.6
# (torch's float32 norm over 4.3 M elements is what costs ~300 units; LAMB's p is the same error divided by sqrt(v) + eps).
# The kernels get four times that: their order of additions and their fused multiply-adds differ from torch's, their algorithm may not.
TOL = {'lars': {'p': 4 * 340.8, 'state': 4 * 293.3, 'ratio': 4 * 313.8}, 'lamb': {'p': 4 * 8777.2, 'state': 4 * 7.94, 'ratio': 4 * 330.6}}


@functools.lru_cache(None)
def data():
    g = torch.Generator().manual_seed(7)
    params = [torch.randn(n, generator=g) for n in SIZES_A + SIZES_B]
    params[ZERO_P].zero_()
    grads = [[torch.randn(n, generator=g) * (1 + 0.25 * k) for n in SIZES_A + SIZES_B] for k in range(STEPS)]
    for gs in grads:
        gs[ZERO_G].zero_()
        gs[NO_G] = None
    return params, grads


def reference(kind, cfg, T):
    """The update rules of FusedLARS / FusedLAMB as plain torch on the CPU in dtype T: (p, state, ratio) and their magnitudes."""
    params, grads = data()
    P, S, SM = [p.to(T) for p in params], [{} for _ in params], [{} for _ in params]      # SM: magnitude of each state tensor
    moved = [0 * p for p in P]                                                             # sum over the steps of |lr * update|
    one = torch.ones((), dtype=T)
    for k in range(STEPS):
        G = [None if g is None else g.to(T) for g in grads[k]]
        c = one
        if cfg['clip']:
            norm = torch.sqrt(sum(g.square().sum() for g in G if g is not None))
            c = cfg['clip'] / torch.maximum(norm, cfg['clip'] * one)
        R = []
        for i, (p, g, st, sm) in enumerate(zip(P, G, S, SM)):
            if g is None:
                continue
            on = i < len(SIZES_A)
            lr, wd = (cfg['lr'], cfg['wd']) if on else (LR_B, 0.0)
            g, wn = c * g, p.norm()
            if kind == 'lars':
                gn, mom = g.norm(), cfg['momentum']
                r = ETA * wn / (gn + wd * wn + LARS_EPS) if on and wn > 0 and gn > 0 else one
                upd = g = r * (g + wd * p)
                if mom:
                    old = st.get('momentum_buffer')
                    st['momentum_buffer'] = g.clone() if old is None else mom * old + g
                    sm['momentum_buffer'] = g.abs() if old is None else mom * sm['momentum_buffer'] + g.abs()
                    upd = g + mom * st['momentum_buffer'] if cfg['nesterov'] else st['momentum_buffer']
                step = lr * one
            else:
                (b1, b2), t = BETAS, k + 1
                m, v = b1 * st.get('exp_avg', 0 * p), b2 * st.get('exp_avg_sq', 0 * p)
                st['exp_avg'], st['exp_avg_sq'] = m + (1 - b1) * g, v + (1 - b2) * g * g
                sm['exp_avg'], sm['exp_avg_sq'] = b1 * sm.get('exp_avg', 0 * p) + ((1 - b1) * g).abs(), st['exp_avg_sq']
                upd = (st['exp_avg'] / (1 - b1 ** t)) / (torch.sqrt(st['exp_avg_sq'] / (1 - b2 ** t)) + LAMB_EPS) + wd * p
                un = upd.norm()
                r = wn / un if on and wn > 0 and un > 0 else one
                step = lr * r
            P[i] = p - step * upd
            R.append(r)
            moved[i] = moved[i] + (step * upd).abs()
    return dict(p=P, state=S, ratio=torch.stack(R), mag_p=[p.abs() + d for p, d in zip(P, moved)], mag_state=SM)


def make(kind, groups, cfg, **kw):
    from fastvision_amd import FusedLAMB, FusedLARS
    if kind == 'lars':
        return FusedLARS(groups, lr=cfg['lr'], momentum=cfg['momentum'], nesterov=cfg['nesterov'], weight_decay=cfg['wd'],
                         trust_coefficient=ETA, eps=LARS_EPS, clip_norm=cfg['clip'], **kw)
    return FusedLAMB(groups, lr=cfg['lr'], betas=BETAS, eps=LAMB_EPS, weight_decay=cfg['wd'], clip_norm=cfg['clip'], **kw)


def run_fused(kind, cfg):
    params, grads = data()
    ps = [torch.nn.Parameter(p.to(DEV)) for p in params]
    na = len(SIZES_A)
    ps[na] = torch.nn.Parameter(torch.cat([torch.zeros(5), params[na]]).to(DEV)[5:])      # storage offset 5: the scalar path
    opt = make(kind, [{'params': ps[:na]}, {'params': ps[na:], 'lr': LR_B, 'weight_decay': 0.0, 'trust_coefficient': 0.0, 'trust': False}], cfg)
    for k in range(STEPS):
        for p, g in zip(ps, grads[k]):
            p.grad = None if g is None else g.to(DEV)
        opt.step()
        if k == 0:
            opt.first_ratio = opt.last_trust_ratio.clone()         # the all-zero parameter is all-zero in the first step only
    torch.cuda.synchronize()
    return ps, opt


def units(got, want, mag):
    """Largest |got - want| in units of 2^-24 * mag (where the magnitude is 0 the value must be exact)."""
    err = (got.detach().double().cpu() - want).abs() / (2.0 ** -24 * mag.double()).clamp_min(1e-300)
    return err.max().item()


@pytest.mark.parametrize('kind,cfg', CASES, ids=lambda v: v if isinstance(v, str) else '-'.join(f'{k}={x}' for k, x in v.items()))
def test_three_steps_match_the_float64_restatement(kind, cfg):
    from fastvision_amd import _lib
    assert _lib.call('fva_sgd_chunk_elems') == CHUNK
    ps, opt = run_fused(kind, cfg)
    ref = reference(kind, cfg, torch.float64)
    with_grad = [i for i in range(len(ps)) if i != NO_G]
    worst = {'p': 0.0, 'state': 0.0}
    for i in with_grad:
        worst['p'] = max(worst['p'], units(ps[i], ref['p'][i], ref['mag_p'][i]))
        assert opt.state[ps[i]].keys() - {'step'} == ref['state'][i].keys()
        for name, want in ref['state'][i].items():
            worst['state'] = max(worst['state'], units(opt.state[ps[i]][name], want, ref['mag_state'][i][name]))
    ratio = opt.last_trust_ratio
    worst['ratio'] = units(ratio, ref['ratio'], ref['ratio'])
    print(kind, cfg, worst)
    assert all(worst[k] <= TOL[kind][k] for k in worst), worst
    # exact: the parameter without a gradient is untouched and has no state; a zero norm gives the ratio 1; trust off gives 1
    assert torch.equal(ps[NO_G].cpu(), data()[0][NO_G]) and not opt.state[ps[NO_G]]
    assert opt.first_ratio[with_grad.index(ZERO_P)] == 1 and bool((ratio[-len(SIZES_B):] == 1).all())
    if kind == 'lars' or not cfg['wd']:           # LAMB with decay: u = wd * p has a norm
        assert ratio[with_grad.index(ZERO_G)] == 1
    if not cfg['wd']:
        assert torch.equal(ps[ZERO_G].cpu(), data()[0][ZERO_G])
    if cfg['clip']:
        norm = torch.sqrt(sum(g.double().square().sum() for g in data()[1][STEPS - 1] if g is not None))
        assert abs(opt.last_grad_norm.item() - norm.item()) <= 2.0 ** -23 * norm.item()


@pytest.mark.parametrize('kind,cfg', [('lars', LARS[-1]), ('lamb', LAMB[-1])], ids=['lars', 'lamb'])
def test_two_runs_are_bit_identical(kind, cfg):
    (pa, oa), (pb, ob) = run_fused(kind, cfg), run_fused(kind, cfg)
    for a, b in zip(pa, pb):
        assert torch.equal(a, b)
        assert all(torch.equal(oa.state[a][k], ob.state[b][k]) for k in oa.state[a] if k != 'step')
    assert torch.equal(oa.last_trust_ratio, ob.last_trust_ratio) and torch.equal(oa.last_grad_norm, ob.last_grad_norm)


# ---------------------------------------------------------------------------------------------------------------- graphs
LRS = [0.01, 0.01, 0.004, 0.004, 0.002]


class Params(torch.nn.Module):
    def __init__(self, sizes=(5, 1023, CHUNK * 16 + 3, 70000)):
        super().__init__()
        g = torch.Generator().manual_seed(1)
        self.ws = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(n, generator=g)) for n in sizes])


def _capturable(kind):
    m = Params().to(DEV)
    cfg = dict(lr=0.01, momentum=0.9, nesterov=True, wd=5e-4, clip=10.0)
    return m, make(kind, [{'params': list(m.ws[:3])}, {'params': [m.ws[3]], 'trust_coefficient': 0.0, 'trust': False}], cfg, capturable=True)


def _fwd_bwd(m):
    x = [torch.linspace(-2, 2, p.numel(), device=DEV) for p in m.ws]
    sum(((p * xi) ** 2).sum() * 0.5 + torch.sin(p).sum() for p, xi in zip(m.ws, x)).backward()


def _eager(m, opt, lr):
    opt.param_groups[0]['lr'] = lr
    opt.zero_grad(set_to_none=True)
    _fwd_bwd(m)
    opt.step()


@pytest.mark.parametrize('kind', ['lars', 'lamb'])
def test_captured_step_replays_like_eager_steps(kind):
    (a, oa), (b, ob) = _capturable(kind), _capturable(kind)
    _eager(a, oa, LRS[0])
    _eager(b, ob, LRS[0])                 # the eager step a capture needs (state, tables, staging)
    for lr in LRS:
        _eager(a, oa, lr)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ob.zero_grad(set_to_none=True)
    torch.cuda.current_stream().wait_stream(side)
    host, keep, graph = ob.host_state(), ob.begin_capture(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _fwd_bwd(b)
        ob.step()
    ob.set_host_state(host)
    assert keep
    for lr in LRS:
        ob.param_groups[0]['lr'] = lr
        ob.sync_lr()
        graph.replay()
        ob.note_replayed_steps(1)
    torch.cuda.synchronize()
    for p, q in zip(a.parameters(), b.parameters()):
        assert torch.equal(p, q)
        assert all(torch.equal(torch.as_tensor(oa.state[p][k]), torch.as_tensor(ob.state[q][k])) for k in oa.state[p])
    assert torch.equal(oa.last_trust_ratio, ob.last_trust_ratio) and torch.equal(oa.last_grad_norm, ob.last_grad_norm)


# ----------------------------------------------------------------------------------------------------------- checkpoints
def _step(m, opt, k):
    for i, p in enumerate(m.ws):
        p.grad = torch.cos(torch.arange(p.numel(), device=DEV) * (0.1 + i) + k)
    opt.step()


def test_lamb_checkpoints_exchange_with_fused_adam():
    from fastvision_amd import FusedAdam, FusedLAMB
    m, m2 = Params().to(DEV), Params().to(DEV)
    lamb = FusedLAMB(m.parameters(), lr=0.01)
    _step(m, lamb, 0)
    adam = FusedAdam(m2.parameters(), lr=0.01)
    adam.load_state_dict(copy.deepcopy(lamb.state_dict()))
    _step(m2, adam, 1)                                                   # Adam continues LAMB's moments and step count
    assert all(adam._step_of(p) == 2 for p in m2.parameters())
    back = FusedLAMB(m.parameters(), lr=0.01)
    back.load_state_dict(copy.deepcopy(adam.state_dict()))
    assert back.param_groups[0]['trust'] is True
    _step(m, lamb, 1)
    for p in m.parameters():                                             # the same gradient gives the same moments in both
        assert torch.allclose(lamb.state[p]['exp_avg'], back.state[p]['exp_avg'], rtol=1e-6, atol=1e-7)
    _step(m, back, 2)
    assert all(back._step_of(p) == 3 for p in m.parameters()) and all(torch.isfinite(p).all() for p in m.parameters())


def test_lars_checkpoints_exchange_with_torch_sgd():
    from fastvision_amd import FusedLARS
    m, m2 = Params().to(DEV), Params().to(DEV)
    lars = FusedLARS(m.parameters(), lr=0.01, momentum=0.9, trust_coefficient=0.02)
    _step(m, lars, 0)
    sgd = torch.optim.SGD(m2.parameters(), lr=0.01, momentum=0.9)
    sgd.load_state_dict(copy.deepcopy(lars.state_dict()))
    for p, q in zip(m.parameters(), m2.parameters()):
        assert torch.equal(sgd.state[q]['momentum_buffer'], lars.state[p]['momentum_buffer'])
    _step(m2, sgd, 1)
    back = FusedLARS(m.parameters(), lr=0.01, momentum=0.9, trust_coefficient=0.02)
    back.load_state_dict(copy.deepcopy(sgd.state_dict()))
    assert back.param_groups[0]['trust_coefficient'] == 0.02 and back.param_groups[0]['eps'] == 1e-8
    before = [(p.detach().clone(), sgd.state[q]['momentum_buffer'].clone()) for p, q in zip(m.parameters(), m2.parameters())]
    _step(m, back, 2)                                                    # a loaded buffer has history: momentum * buf + g, not buf = g
    for i, (p, (old, buf)) in enumerate(zip(m.parameters(), before)):
        g = back.last_trust_ratio[i] * p.grad
        want = 0.9 * buf + g
        assert torch.allclose(back.state[p]['momentum_buffer'], want, rtol=1e-5, atol=1e-7)
        assert torch.allclose(p, old - 0.01 * want, rtol=1e-5, atol=1e-7)
