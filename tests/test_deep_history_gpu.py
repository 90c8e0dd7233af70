"""hb_belief_history_step, hb_belief_splice_alive / hb_belief_splice and hb_belief_score (csrc/belief.hip) on the deep games of
tests/deep_history.py and the deep rows of tests/deep_rows.py, all twelve variants, everything bit for bit. The history kernel is
held to the identity model (plain lists of card serials; PartnerHistory("cpu") is not consulted): the pushed move is the move the
driver made, the masks say which cards are still held. The splice runs on the histories those runs leave: the true rows give the
stored rows back, determinized candidates land where the rule says, from the rows alone and against the restatement. The score
runs on the nine variants it had never seen. tests/test_deep_history_cpu.py holds the model, the corpus and the restatements."""
import functools

import numpy as np
import pytest

import deep_history as DH
import deep_rows as DR
from search_util import _u32

pytestmark = pytest.mark.gpu

N = 48
FILL = {1: 0x5A, 4: 0x5A5A5A5A}


def _seats(players):
    return tuple(range(players)) if players <= 3 else (0, 1, players - 1)


@functools.lru_cache(maxsize=None)
def _rows_dev(game, players):
    """The corpus' rows [T + 1, 48, SW] as int32 on the device."""
    import torch

    return torch.from_numpy(np.array(DH.play(game, players).rows).view(np.int32)).cuda()


def _run(game, players, seat, depth, guard=0, snap=()):
    """One observer's history on the device through PartnerHistory.advance, all 48 games in one launch per call, compared with
    the model after every call. guard > 0: the four tensors sit `guard` elements into sentinel-filled buffers (3: hist_rows 12
    bytes off a 16-byte boundary, the word-by-word form). -> {ply: (hist_rows, alive) clones} for the plies in `snap`."""
    import torch

    import hanabi_hip
    from hanabi_hip import PartnerHistory

    cfg = hanabi_hip.make_config(game, players)
    rows_dev = _rows_dev(game, players)
    model = DH.Model(game, players, seat, depth)
    h = PartnerHistory(cfg, N, depth, "cuda")
    bufs = {}
    for name in ("prev_rows", "moves", "alive", "valid") if guard else ():
        t = getattr(h, name)
        buf = torch.full((t.numel() + 2 * guard,), FILL[t.dtype.itemsize], dtype=t.dtype, device="cuda")
        view = buf[guard:guard + t.numel()].view(t.shape)
        view.zero_()
        bufs[name] = buf
        setattr(h, name, view)
    if guard:
        assert h.prev_rows.data_ptr() % 16 == (4 * guard) % 16
    snaps, pushes = {}, 0
    for call in model.calls():
        t = call["t"]
        if call["own"] is not None:
            h.advance(own_moves=torch.from_numpy(call["own"]).cuda())
        else:
            h.advance(cur_rows=rows_dev[t + 1], prev_rows=rows_dev[t], seat=seat, draw=t)
            pushes += 1
            assert h.draws[0] == t
        where = (game, players, "seat", seat, "depth", depth, "guard", guard, "ply", t)
        assert np.array_equal(_u32(h.prev_rows), model.rows), ("rows",) + where
        assert np.array_equal(h.moves.cpu().numpy(), model.moves), ("moves",) + where
        assert np.array_equal(h.alive.cpu().numpy(), model.alive), ("alive",) + where
        assert np.array_equal(h.valid.cpu().numpy(), model.valid), ("valid",) + where
        assert h.filled == min(pushes, depth)
        if t in snap:
            snaps[t] = (h.prev_rows.clone(), h.alive.clone())
    for name, buf in bufs.items():   # the sentinels on both sides
        fill = FILL[buf.dtype.itemsize]
        assert bool((buf[:guard] == fill).all()) and bool((buf[-guard:] == fill).all()), (name, game, players)
    return snaps


@functools.lru_cache(maxsize=None)
def _deep_histories(game, players):
    """The depth-8 runs of the tested seats: {seat: {ply: (hist_rows [8, 48, SW] int32, alive [8, 48] uint8)}} at splice_plies."""
    plies = DH.splice_plies(game, players)
    return {seat: _run(game, players, seat, 8, snap=plies) for seat in _seats(players)}


@pytest.mark.parametrize("game,players", DH.VARIANTS)
def test_history_step_equals_the_identity_model(game, players):
    """Depth 1 and 8, every observer seat for P <= 3, seats 0, 1 and P - 1 for P >= 4, from zeros, all four tensors after every
    call; the last seat once more at depth 8 with every tensor 3 elements into a sentinel-filled buffer."""
    assert _rows_dev(game, players).shape[2] == (48 if players >= 4 else 32)
    _deep_histories(game, players)
    for seat in _seats(players):
        _run(game, players, seat, 1)
    _run(game, players, players - 1, 8, guard=3)


def _fields(hand):
    """[..., 5]: the five 5-bit fields of hand words."""
    return np.stack([(np.asarray(hand).astype(np.int64) >> (5 * s)) & 31 for s in range(5)], axis=-1)


def _check_spliced(out, stored, alive, det, seat, K):
    """What hb_belief_splice_alive promises, from the rows alone: out [K, m, SW], stored [m, SW], alive [m], det [m * K, SW]."""
    m, SW = stored.shape
    w = 10 + seat
    other = np.arange(SW) != w
    assert np.array_equal(out[:, :, other], np.broadcast_to(stored[:, other], (K, m, SW - 1))), "a word other than the hand's changed"
    got, old = _fields(out[:, :, w]), _fields(stored[:, w])[None]                    # [K, m, 5], [1, m, 5]
    cand = _fields(det[:, w].reshape(m, K).T)                                         # [K, m, 5]
    takes = (old != 31) & (((alive.astype(np.int64)[None, :, None] >> np.arange(5)) & 1) == 1)   # [1, m, 5]
    assert np.array_equal((out[:, :, w] >> 25), np.broadcast_to(stored[:, w] >> 25, (K, m))), "bits 25 .. 31 of the hand word changed"
    keep = np.broadcast_to(~takes, got.shape)
    assert np.array_equal(got[keep], np.broadcast_to(old, got.shape)[keep]), "a dead or empty slot does not hold the stored card"
    j = np.broadcast_to(np.cumsum(takes, axis=-1) - takes, got.shape)                # the alive slots before each slot
    want = np.take_along_axis(cand, j, axis=-1)
    take = np.broadcast_to(takes, got.shape)
    assert (want[take] != 31).all(), "more cards alive than the candidate holds"
    assert np.array_equal(got[take], want[take]), "the alive slots do not hold the candidate's hand prefix in order"


@pytest.mark.parametrize("game,players", DH.VARIANTS)
def test_splice_alive_on_the_histories_deep_play_leaves(game, players):
    """At the ply of the first push on an empty deck, the ply with the most short hands and a mid-game ply, for every tested
    seat and every stored entry d: (a) the true current rows, K = 1, give hist_rows[d] back word for word; (b) candidates from
    hb_belief_determinize at the explicit seat (K = 3 and 65) land as the restatement has them and as the
    rule says from the rows alone; (c) where the ply was another seat's (the observer holds now what it held in the newest
    entry), alive = NULL on the newest entry is hb_belief_splice's restatement: the candidate's whole hand word."""
    import torch
    from test_search_belief_cpu import splice_ref
    from test_search_depth_cpu import splice_alive_ref

    import hanabi_hip
    from hanabi_hip import Determinizer, belief_splice, belief_splice_alive

    cfg = hanabi_hip.make_config(game, players)
    rows_dev = _rows_dev(game, players)
    det_of = Determinizer(config=cfg)
    seen = dict(entries=0, dead=0, short_stored=0, short_now=0, finished=0, null=0)
    for seat, snaps in _deep_histories(game, players).items():
        for ply, (hist, alive) in snaps.items():
            now = rows_dev[ply + 1].contiguous()
            now_n = _u32(now)
            filled = sum(1 for t in range(ply + 1) if t % players != seat)
            cands = {}
            for K in (3, 65):
                det, w = det_of.sample(now, seat=seat, replicas=K, seed=21, draw=ply, first_row_id=1000 * seat)
                cands[K] = (det, _u32(det))
                assert bool((w.view(N, K) > 0).any(1).cpu().numpy()[DH.running(now_n)].all())
            for d in range(min(8, filled)):
                stored, mask = hist[d].contiguous(), alive[d].contiguous()
                stored_n, mask_n = _u32(stored), mask.cpu().numpy()
                back = belief_splice_alive(cfg, stored, mask, now, seat, 1)
                assert np.array_equal(_u32(back)[0], stored_n), ("the true rows do not give the stored rows back", seat, ply, d)
                for K, (det, det_n) in cands.items():
                    out = _u32(belief_splice_alive(cfg, stored, mask, det, seat, K))
                    assert np.array_equal(out.reshape(K * N, -1), splice_alive_ref(stored_n, mask_n, det_n, seat, K)), (seat, ply, d, K)
                    _check_spliced(out, stored_n, mask_n, det_n, seat, K)
                occ = (_fields(stored_n[:, 10 + seat]) != 31).sum(1)
                seen["entries"] += N
                seen["dead"] += int((np.array([bin(int(a) & 31).count("1") for a in mask_n]) < occ).sum())
                seen["short_stored"] += int((DH.running(stored_n) & (occ < cfg.hand_size)).sum())
                seen["short_now"] += int((DH.running(now_n) & (DH.hand_n(now_n, seat) < cfg.hand_size)).sum())
                seen["finished"] += int((~DH.running(now_n)).sum())
            if filled and ply % players != seat:
                stored = hist[0].contiguous()
                for K, (det, det_n) in cands.items():
                    want = splice_ref(_u32(stored), det_n, seat, K)
                    assert np.array_equal(_u32(belief_splice_alive(cfg, stored, None, det, seat, K)).reshape(K * N, -1), want), (seat, ply, K)
                    assert np.array_equal(_u32(belief_splice(cfg, stored, det, seat, K)).reshape(K * N, -1), want), (seat, ply, K)
                    seen["null"] += 1
    torch.cuda.synchronize()
    print(game, players, seen)
    assert seen["entries"] > 0 and seen["dead"] > 0 and seen["null"] > 0
    if players > 2:
        assert seen["short_stored"] > 0 and seen["short_now"] > 0


SCORE_VARIANTS = [v for v in DR.VARIANTS if v not in (("Hanabi-Full", 2), ("Hanabi-Small", 2), ("Hanabi-Full", 5))]


@pytest.mark.parametrize("game,players", SCORE_VARIANTS)
def test_score_on_the_deep_rows_of_the_variants_it_never_saw(game, players):
    """deep_rows.pick: seat -1 and every seat that is some row's short seat, R in {1, 65}, replicas from the determinizer with a
    third of the weights zeroed, counts given and NULL: bit-equal to belief_score_ref, and from the outputs alone: wsum is the sum
    of the weights; truth is the true hand below the hand size and -1 above it; every slot below the hand size has its counts sum
    to wsum (a determinizer replica holds only real cards); hit is counts at the truth; the prior is 0 wherever the slot's
    knowledge rules the card out."""
    import torch

    import hanabi_hip
    from hanabi_hip import Determinizer, belief_score, belief_score_ref

    cfg, ocfg = hanabi_hip.make_config(game, players), DH.config(game, players)
    p = DR.pick(game, players)
    cats = set(p.category)
    assert {"short", "finished", "deck0"} <= cats and (p.short_seat >= 0).any()
    true = np.array(p.rows)
    m, SW = true.shape
    assert SW == (48 if players >= 4 else 32) and (cfg.hand_size, cfg.colors * cfg.ranks) in ((5, 25), (4, 25), (2, 10), (2, 5))
    H, NC = cfg.hand_size, cfg.colors * cfg.ranks
    rows_dev = torch.from_numpy(true.view(np.int32)).cuda()
    det_of = Determinizer(config=cfg)
    seen = dict(short=0, finished=0, dead=0)
    for seat in [-1] + sorted(set(int(s) for s in p.short_seat if s >= 0)):
        live, st, hand, n_hand, know, _, _ = DR._view(ocfg, true, seat)
        n_hand = np.where(live, n_hand, 0)
        below = np.arange(H)[None, :] < n_hand[:, None]
        seen["short"] += int((live & (n_hand < H)).sum())
        seen["finished"] += int((~live).sum())
        for R in (1, 65):
            rng = np.random.default_rng(1000 * R + seat + 1)
            det, w = det_of.sample(rows_dev, seat=seat, replicas=R, seed=3, draw=R, out=(
                torch.empty((m * R, SW), dtype=torch.int32, device="cuda"), torch.empty(m * R, dtype=torch.int32, device="cuda")))
            w_n = _u32(w).copy()
            w_n[rng.random(m * R) < 1 / 3] = 0
            w_dev = torch.from_numpy(w_n.view(np.int32)).cuda()
            want = belief_score_ref(cfg, true, _u32(det), w_n, seat, R)
            for counts in (True, False):
                got = belief_score(cfg, rows_dev, det, w_dev, seat, R, counts=counts)
                for name in ("truth", "hit", "joint", "wsum", "n_live", "prior") + (("counts",) if counts else ()):
                    g = getattr(got, name).cpu().numpy()
                    assert g.dtype == want[name].dtype and np.array_equal(g, want[name]), (name, seat, R, counts)
                assert counts or got.counts is None
                truth, hit, wsum = got.truth.cpu().numpy(), got.hit.cpu().numpy(), got.wsum.cpu().numpy()
                wl = np.where(live[:, None], w_n.reshape(m, R).astype(np.int64), 0)
                assert np.array_equal(wsum, wl.sum(1)) and np.array_equal(got.n_live.cpu().numpy(), (wl != 0).sum(1))
                assert np.array_equal(truth, np.where(below, hand, -1))
                prior = got.prior.cpu().numpy()
                card = np.broadcast_to(np.arange(NC)[None, None, :], prior.shape)
                ruled_out = ~(DR._plausible(ocfg, np.broadcast_to(know[:, :, None], prior.shape), card) & below[:, :, None])
                assert not prior[ruled_out].any() and (prior[~ruled_out] >= 0).all()
                at_truth = np.take_along_axis(prior, np.clip(truth, 0, NC - 1)[:, :, None].astype(np.int64), 2)[:, :, 0]
                assert (at_truth[below] >= 1).all(), "the true card is not in the seat's own pool"
                if counts:
                    cnt = got.counts.cpu().numpy()
                    assert np.array_equal(cnt.sum(2), np.where(below, wsum[:, None], 0))
                    assert np.array_equal(hit, np.where(below, np.take_along_axis(cnt, np.clip(truth, 0, NC - 1)[:, :, None].astype(np.int64), 2)[:, :, 0], 0))
            seen["dead"] += int(((want["n_live"] < R) & live).sum())
    print(game, players, "rows", m, seen)
    assert seen["short"] and seen["finished"] and seen["dead"]
