"""tests/detect_restatement.py pinned without a GPU: the restatements equal the oracle's functions at the oracle's fixed parameters, every
constructed edge input has the property it is there for (bit-equal scores, IoUs exactly on the threshold, the intended candidate counts, the
excused-row shares within their caps), and the wrong kernels the GPU tests are there to catch give other results on these inputs."""
import numpy as np
import pytest
import torch

import detect_restatement as dr
import streaming_measure as sm
from oracle import detect as D
from oracle import rpn as R

F64, F32 = dr.F64, dr.F32


# ---- decode ------------------------------------------------------------------------------------------------------------------------------
def test_decode_restatement_equals_the_oracle_in_fp32():
    """non-square maps, 4 levels, mixed A: library rows (a, y, x) all of them; demo rows (y, x, a), those that survive, in order"""
    heads, anchors, strides, lb = dr.decode_case('four_levels_k85')
    got, _, _ = dr.decode_rows(heads, anchors, strides, 0, None, F32)
    want = D.decode_library(heads, strides, [torch.tensor(a) for a in anchors])
    assert torch.equal(got, want)
    for b in range(heads[0].shape[0]):                                  # the demo handles one image
        one = [h[b:b + 1] for h in heads]
        got, _, _ = dr.decode_rows(one, anchors, strides, 1, lb, F32)
        r64, mag, _ = dr.decode_rows(one, anchors, strides, 1, lb, F64)
        layers = [h.permute(0, 1, 4, 2, 3).reshape(1, -1, h.shape[2], h.shape[3]) for h in one]
        want = D.decode_demo(layers, strides, [torch.tensor(a) for a in anchors], *lb[:5])
        alive = got[0, :, 4] != -1
        assert torch.equal(alive, r64[0, :, 4] != -1) and 0 < int(alive.sum()) < got.size(1) and want.size(0) == int(alive.sum())
        # torch's fp32 sigmoid is not one function (its vector body and scalar tail differ in the last bit, and which elements get which
        # depends on the memory layout), so the surviving rows are compared in order with the measure itself: the oracle is an honest fp32
        # evaluation, and so is the restatement
        lim = sm.limit_of(r64, got, mag)[0][alive]
        assert sm.worst_f32(want, r64[0][alive], lim) <= 1.0
        assert (got[0][alive] - want).abs().max() <= 2.0 ** -20 * want.abs().max()


@pytest.mark.parametrize('name', sorted(dr.DECODE_CASES))
def test_decode_cases_have_their_properties(name):
    B, K, levels = dr.DECODE_CASES[name]
    heads, anchors, strides, lb = dr.decode_case(name)
    rows = sum(A * H * W for A, H, W, _ in levels)
    assert (rows * K) % 256 != 0 and all(1 <= A <= 8 for A, _, _, _ in levels) and K >= 6
    assert any(H != W for _, H, W, _ in levels)
    assert any((h == 30).all(-1).any() for h in heads) and any((h == -30).all(-1).any() for h in heads)
    # an honest fp32 evaluation passes the measure, in every variant
    for variant, box in ((0, None), (1, None), (1, lb)):
        r64, mag, e64 = dr.decode_rows(heads, anchors, strides, variant, box, F64)
        r32, _, e32 = dr.decode_rows(heads, anchors, strides, variant, box, F32)
        assert r64.shape == (B, rows, K) and torch.isfinite(r64).all()
        if box is not None:
            ex = dr.decode_excused(e64, e32, box[5])
            dropped = (r64[..., 4] == -1).double().mean().item()
            print(f'{name}: dropped {dropped:.3f}, excused {ex.double().mean().item():.4f}')
            assert ex.double().mean().item() <= dr.MAX_EXCUSED
            assert dropped >= dr.MIN_SHARE and 1 - dropped >= dr.MIN_SHARE
            r32 = r32.clone()
            r32[..., 4] = torch.where(ex, r64[..., 4].float(), r32[..., 4])
        assert sm.check(r32, r64, r32, mag, False, what=name) <= 0.25    # an honest fp32 evaluation: err = e32 <= limit / FACTOR
    # the two wrong kernels decode has never been able to show: H for W in the cell split, and the library's rows in (y, x, a) order
    r64, mag, _ = dr.decode_rows(heads, anchors, strides, 0, None, F64)
    r32, _, _ = dr.decode_rows(heads, anchors, strides, 0, None, F32)
    lim = sm.limit_of(r64, r32, mag)
    swapped = [h.transpose(2, 3).reshape(h.shape) for h in heads]       # the element at (y, x) read as if the row length were H
    bad, _, _ = dr.decode_rows(swapped, anchors, strides, 0, None, F32)
    if any(H != W and min(H, W) > 1 for _, H, W, _ in levels):
        assert sm.worst_f32(bad, r64, lim) > 100
    bad, _, _ = dr.decode_rows(heads, anchors, strides, 1, None, F32)
    if any(A > 1 for A, _, _, _ in levels):
        assert sm.worst_f32(bad, r64, lim) > 100


def test_rpn_rows_restatement_equals_the_oracle_in_fp32():
    for A in (1, 9):
        cls, d, base = dr.rpn_case(3, 5, A)
        got, mag = dr.rpn_rows(cls, d, base, F32)
        want = R.proposal_rows(cls, d, R.make_anchors_xywh(base, 3, 5), 3, 5)
        assert torch.equal(got[..., :4], want[..., 1:]) and torch.equal(got[..., 4], want[..., 0]) and (got[..., 5] == 1).all()
        r64, mag = dr.rpn_rows(cls, d, base, F64)
        assert sm.worst_f32(got, r64, sm.limit_of(r64, got, mag)) <= 1.0
        # the quirk: a height decoded with exp(d[3]) is another result
        d2 = d.clone()
        d2[..., 2] = d[..., 3]
        other, _ = dr.rpn_rows(cls, d2, base, F64)
        assert sm.worst_f32(other[..., 1].float(), r64[..., 1], sm.limit_of(r64, got, mag)[..., 1]) > 100


def test_rpn_tie_case_ties_across_the_cut():
    cls, d, base, tied = dr.rpn_tie_case()
    rows, _ = dr.rpn_rows(cls, d, base, F32)
    s = rows[0, :, 4]
    assert rows.size(1) == 130 and tied.numel() == 10 and len(set(s[tied].tolist())) == 1
    assert int((s > s[tied[0]]).sum()) == 60 and int((s == s[tied[0]]).sum()) == 10
    for k in (64, 65):
        prop, src = dr.proposals_from_rows(rows[0], k, 130, 0.7)
        stable = torch.from_numpy(np.argsort(-s.numpy(), kind='stable')[:k].copy())
        assert set(src.tolist()) <= set(stable.tolist())
        assert set(tied[:k - 60].tolist()) <= set(stable.tolist()) and not set(tied[k - 60:].tolist()) & set(stable.tolist())
        assert 0 < prop.size(0) < k                                     # NMS has removed something
        # a top-k that prefers the HIGHER row among equals selects other rows
        other = torch.from_numpy(np.argsort(-s.numpy()[::-1], kind='stable')[:k].copy())
        assert set((129 - other).tolist()) != set(stable.tolist())


# ---- candidates and NMS ------------------------------------------------------------------------------------------------------------------
def test_nms_restatement_equals_the_oracle_wrappers():
    from oracle.make_golden import synth_predictions
    for i, n_obj in enumerate((4, 0, 9, 2)):
        pred = synth_predictions(torch.Generator().manual_seed(40 + i), 3000, n_obj, 640)
        sc, cat, box = D.nms_library(pred, 0.25, 0.45, 50)
        det, rows = dr.nms_restatement(pred, 0.25, 0.45, 50, 0, 0, 0, 0.0, 0)
        if n_obj:
            assert torch.equal(det, torch.cat([box, sc, cat.float()], 1))
            assert torch.equal(D.xywh2xyxy(pred[rows, :4]), det[:, :4]) and (pred[rows, 4] > 0.25).all()
        else:
            assert det.shape == (0, 6) and rows.numel() == 0
        det, _ = dr.nms_restatement(pred, 0.25, 0.45, 50, 0, 0, 1, 4096.0, 30000)
        assert torch.equal(det, D.nms_demo_batch([pred], 0.25, 0.45, 50)[0].view(-1, 6))
        xyxy = pred.clone()
        xyxy[:, 2:4] = pred[:, 0:2] + pred[:, 2:4]
        det, rows = dr.nms_restatement(xyxy, 0.25, 0.45, 50, 1, 1, 0, 4096.0, 30000)
        assert torch.equal(det, D.nms_demo(xyxy, 0.25, 0.45, 50).view(-1, 6))
        assert torch.equal(xyxy[rows, :5], det[:, :5])


@pytest.mark.parametrize('C', [1, 2, 64, 65, 130])
def test_candidate_cases_have_their_properties(C):
    for Rn in (1, 63, 64, 65, 1023, 1024, 1025, 2049):
        pred, info = dr.candidate_case(Rn, C)
        assert pred.shape == (3, Rn, 5 + C)
        obj = pred[..., 4]
        assert int((obj[1] > dr.CONF).sum()) == 0 and int((obj[1] == dr.CONF).sum()) > 0
        assert int((obj[0] > dr.CONF).sum()) > 0 and int((obj[2] > dr.CONF).sum()) > 0
        for r in (0, 63, 64, Rn - 1):
            if r < Rn:
                assert obj[0, r] > dr.CONF and obj[2, r] > dr.CONF
        if Rn > 1:
            assert len(info['ties']) == 2 * len(dr.class_ties_for(C)) and len(info['at_conf']) == 2 and len(info['best_at_conf']) == 2
        for b, r, lo, hi in info['ties']:
            prod = pred[b, r, 5:] * pred[b, r, 4]
            assert prod[lo].item() == prod[hi].item() == prod.max().item() and int((prod == prod.max()).sum()) == 2 and lo < hi
            assert obj[b, r] > dr.CONF
        for b, r in info['at_conf']:
            assert obj[b, r].item() == dr.CONF
        for b, r in info['best_at_conf']:
            assert obj[b, r] > dr.CONF and (pred[b, r, 5:] * obj[b, r]).max().item() == dr.CONF
        for b in range(3):
            n = int((obj[b] > dr.CONF).sum())
            det, rows = dr.nms_restatement(pred[b], dr.CONF, 0.45, Rn, 0, 0, 0, 0.0, 0)
            assert det.size(0) == n, 'nothing overlaps: every candidate is a detection'
            det1, rows1 = dr.nms_restatement(pred[b], dr.CONF, 0.45, Rn, 0, 0, 1, 4096.0, 30000)
            ties = [t for t in info['ties'] if t[0] == b]
            for _, r, lo, hi in ties:
                assert det[rows == r, 5].item() == lo
            for bb, r in info['at_conf']:
                assert bb != b or r not in rows.tolist()
            for bb, r in info['best_at_conf']:
                assert bb != b or (r in rows.tolist() and r not in rows1.tolist())
            if ties:                                                    # the higher class winning a tie is another result
                flipped = pred[b].clone()
                flipped[:, 5:] = pred[b].flip(1)[:, :C]
                detf, rowsf = dr.nms_restatement(flipped, dr.CONF, 0.45, Rn, 0, 0, 0, 0.0, 0)
                _, r, lo, hi = ties[0]
                assert C - 1 - detf[rowsf == r, 5].item() == hi


@pytest.mark.parametrize('n', [1, 64, 65, 128, 129, 256, 257, 1100])
def test_rank_cases_have_their_ties(n):
    p, groups = dr.rank_case(n)
    s = p[:, 4]
    assert (s > 0).all() and len(groups) == (n > 64) + (n > 255)
    for grp in groups:
        assert len(set(s[grp].tolist())) == 1 and int((s == s[grp[0]]).sum()) == len(grp)
    assert len(set(s.tolist())) == n - sum(len(g) - 1 for g in groups)
    det, rows = dr.nms_restatement(p, 0.0, 0.45, n, 1, 1, 0, 0.0, 0)
    assert rows.numel() == n
    for grp in groups:
        pos = [rows.tolist().index(i) for i in grp]
        assert pos == list(range(pos[0], pos[0] + len(grp))), 'lower index first, next to each other'
    if n > 255:
        assert rows[:len(groups[0])].tolist() == groups[0] and groups[0][:2] == [0, 255]
    if n > 64:
        assert rows[-2:].tolist() == [63, 64]
    # max_det = 1, 64 and n cut the same order
    for md in (1, 64, n):
        assert torch.equal(dr.nms_restatement(p, 0.0, 0.45, md, 1, 1, 0, 0.0, 0)[1], rows[:md])


def test_all_equal_scores_keep_the_row_order():
    p = dr.all_equal_case()
    assert len(set(p[:, 4].tolist())) == 1 and p.size(0) == 300
    assert dr.nms_restatement(p, 0.0, 0.45, 300, 1, 1, 0, 0.0, 0)[1].tolist() == list(range(300))


@pytest.mark.parametrize('with_gap', [False, True])
@pytest.mark.parametrize('pair', dr.IOU_PAIRS, ids=['iou_0.5', 'iou_0.75'])
def test_pairs_sit_exactly_on_the_threshold(pair, with_gap):
    v, a, b = pair
    gap = np.float32(4096.0 if with_gap else 0.0)
    assert dr.iou_f32(np.float32(a) + gap, np.float32(b) + gap) == np.float32(v) == dr.iou_f32(a, b)
    assert np.float32(dr.below(v)) < np.float32(v) and dr.f32(v) == v
    p, idx = dr.pair_case(pair, with_gap)
    assert len(set(idx.values())) == 4
    order = np.argsort(-p[:, 4].numpy(), kind='stable').tolist()
    assert [order.index(idx[k]) for k in ('a1', 'b1', 'a2', 'b2')] == [0, 1, 2, p.size(0) - 1] and p.size(0) > 64
    if with_gap:
        assert all(int(p[i, 5:].argmax()) == 1 for i in idx.values())
    cg = 4096.0 if with_gap else 0.0
    at = dr.nms_restatement(p, 0.0, v, p.size(0), 1, 1, 0, cg, 0)[1].tolist()
    under = dr.nms_restatement(p, 0.0, dr.below(v), p.size(0), 1, 1, 0, cg, 0)[1].tolist()
    assert len(at) == p.size(0)
    assert sorted(set(at) - set(under)) == sorted([idx['b1'], idx['b2']])


def test_zero_area_and_chain_cases():
    p = dr.zero_area_case()
    b = p[:, :4]
    for i in (1, 70, 130, 65, 66):
        assert ((b[i, 2] - b[i, 0]) * (b[i, 3] - b[i, 1])).item() == 0
    assert np.isnan(dr.iou_f32(b[1], b[70])) and dr.iou_f32(b[2], b[1]) == 0 and dr.iou_f32(b[2], b[130]) == 0
    assert np.isnan(dr.iou_f32(b[65], b[66]))
    for thr in (0.0, 0.45):
        assert sorted(dr.nms_restatement(p, 0.0, thr, 140, 1, 1, 0, 0.0, 0)[1].tolist()) == list(range(140))
    p, (ia, ib, ic) = dr.chain_case()
    order = np.argsort(-p[:, 4].numpy(), kind='stable').tolist()
    assert [order.index(i) // 64 for i in (ia, ib, ic)] == [0, 1, 2]
    assert dr.iou_f32(dr.CHAIN_A, dr.CHAIN_B) > 0.5 and dr.iou_f32(dr.CHAIN_B, dr.CHAIN_C) > 0.5 and dr.iou_f32(dr.CHAIN_A, dr.CHAIN_C) < 0.5
    kept = dr.nms_restatement(p, 0.0, 0.5, 200, 1, 1, 0, 0.0, 0)[1].tolist()
    assert ia in kept and ic in kept and ib not in kept and len(kept) == 199


def test_max_nms_case_cuts_through_ties():
    p = dr.max_nms_case()
    s = p[:, 4].numpy()
    assert p.size(0) == 130
    srt = np.sort(s)[::-1]
    assert srt[62] == srt[63] == srt[64] == srt[65] and srt[61] > srt[62] and srt[66] < srt[65]
    assert srt[98] == srt[99] == srt[100] and srt[97] > srt[98] and srt[101] < srt[100]
    full = dr.nms_restatement(p, 0.0, 0.45, 130, 1, 1, 0, 0.0, 0)[1]
    assert 0 < full.numel() < 130
    stable = np.argsort(-s, kind='stable')
    for mn in (64, 65, 100):
        rows = dr.nms_restatement(p, 0.0, 0.45, 130, 1, 1, 0, 0.0, mn)[1]
        assert set(rows.tolist()) <= set(stable[:mn].tolist())
        tied = np.nonzero(s == s[stable[mn - 1]])[0]
        inside = [i for i in tied if i in stable[:mn]]
        assert 0 < len(inside) < len(tied) and max(inside) < min(i for i in tied if i not in inside), 'the lower indices of the tie stay'


# ---- matchers ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T', [1, 2, 5])
@pytest.mark.parametrize('Na', [1, 255, 256, 257])
def test_match_cases_have_their_properties(Na, T):
    anchors, targets, ties = dr.match_case(Na, T)
    iou = dr.match_iou(anchors, targets)
    assert iou.shape == (Na, T) and iou.dtype == F32
    assert len(ties) == min(T, (Na > 69) + (Na > 256))
    for t, i, j in ties:
        assert torch.equal(anchors[i], anchors[j]) and iou[i, t].item() == iou[j, t].item() == iou[:, t].max().item() < 0.3
        assert int((iou[:, t] == iou[:, t].max()).sum()) == 2
        lab = R.rpn_match(anchors, targets, 1, dr.FH, dr.FW)
        assert lab[0, i] == t and lab[0, j] == -1, 'only the claim shows which of the two won'
    best = iou.max(dim=1).values
    thr = dr.match_thresholds(anchors, targets)
    for v in thr.values():
        assert dr.f32(v) == v and 0 < v < 1 and int((best == v).sum()) >= 1
    if Na >= 255:
        tg = dr.fast_targets(targets)[:, 2:]
        claimed = set(iou.argmax(dim=0).tolist())
        up = float(np.nextafter(np.float32(thr['floor']), np.float32(1)))
        a = [i for i in torch.nonzero(best == thr['pos']).flatten().tolist() if i not in claimed]
        assert a, 'an unclaimed anchor sits on the threshold'
        assert (R.rpn_match(anchors, targets, 1, dr.FH, dr.FW, thr['pos'], thr['pos'] / 2)[0, a] == -2).all()   # == pos_thr: not positive
        assert (R.fast_match(anchors, tg, thr['pos'], thr['pos'] / 2, 0.0)[a] >= 0).all()                       # == pos_thr: positive
        a = [i for i in torch.nonzero(best == thr['neg']).flatten().tolist() if i not in claimed]
        assert a and (R.rpn_match(anchors, targets, 1, dr.FH, dr.FW, 0.999, thr['neg'])[0, a] == -2).all()      # == neg_thr: not negative
        assert (R.fast_match(anchors, tg, 0.999, thr['neg'], 0.0)[a] == -2).all()
        a = torch.nonzero(best == thr['floor']).flatten()
        assert (R.fast_match(anchors, tg, 0.999, 0.998, thr['floor'])[a] == -1).all()                           # == neg_floor: negative
        assert (R.fast_match(anchors, tg, 0.999, 0.998, up)[a] == -2).all()
