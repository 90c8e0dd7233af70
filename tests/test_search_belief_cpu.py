"""The search belief conditioned on the partner's last move, the parts that need no GPU: a numpy restatement of
hb_belief_splice and hb_belief_select (include/hanabi_hip.h), hand-worked cases of the selection, its exactness by enumeration
against the CPU rule oracle, last_move_uid against scripted moves, and argument validation. tests/test_search_belief_gpu.py
holds the kernels to this restatement byte for byte."""
import ctypes as C
import math

import numpy as np
import pytest

from test_search_cpu import SMALL_SCRIPTS, _oracle, deck_size_of, determinize_ref, enumerate_hands, hand_types, seat_view


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def splice_ref(prev_rows, det_rows, seat, K):
    """hb_belief_splice: prev_rows [m, SW], det_rows [m * K, SW] -> [K * m, SW]; row k * m + i = prev row i with word 10 + seat
    taken from candidate (i, k) = det row i * K + k."""
    prev_rows, det_rows = np.asarray(prev_rows).astype(np.uint32), np.asarray(det_rows).astype(np.uint32)
    m = prev_rows.shape[0]
    out = np.empty((K * m, prev_rows.shape[1]), np.uint32)
    for k in range(K):
        for i in range(m):
            out[k * m + i] = prev_rows[i]
            out[k * m + i, 10 + seat] = det_rows[i * K + k, 10 + seat]
    return out


def select_ref(src_rows, det_rows, weights, hyp_moves, actual, valid, K, R):
    """hb_belief_select -> (rows uint32 [m * R, SW], weights uint32 [m * R], n_surv int32 [m], fallback uint8 [m])."""
    src_rows, det_rows = np.asarray(src_rows).astype(np.uint32), np.asarray(det_rows).astype(np.uint32)
    weights, hyp = np.asarray(weights).astype(np.uint32), np.asarray(hyp_moves).reshape(K, -1)
    m = src_rows.shape[0]
    rows, w = np.empty((m * R, src_rows.shape[1]), np.uint32), np.empty(m * R, np.uint32)
    n_surv, fallback = np.zeros(m, np.int32), np.zeros(m, np.uint8)
    for i in range(m):
        usable = (int(src_rows[i, 0]) >> 19) & 3 == 0 and (valid is None or valid[i] != 0)
        surv = [k for k in range(K) if weights[i * K + k] != 0 and hyp[k, i] == actual[i]] if usable else []
        n_surv[i] = len(surv)
        fallback[i] = 2 if not usable else 1 if not surv else 0
        picks = surv[:R] if surv else list(range(R))
        for j in range(R):
            if j < len(picks):
                rows[i * R + j], w[i * R + j] = det_rows[i * K + picks[j]], weights[i * K + picks[j]]
            else:
                rows[i * R + j], w[i * R + j] = src_rows[i], 0
    return rows, w, n_surv, fallback


# ---- hand-worked cases ------------------------------------------------------------------------------------------------------------
def _labelled(m, K, SW=32):
    """Source rows (running) and candidate rows that carry their own (root, candidate) in every word past word 0."""
    src = np.zeros((m, SW), np.uint32)
    src[:, 1:] = 0xAAAA0000 + np.arange(m, dtype=np.uint32)[:, None]
    det = np.zeros((m * K, SW), np.uint32)
    det[:, 1:] = np.arange(m * K, dtype=np.uint32)[:, None] + 1
    return src, det


@pytest.mark.parametrize("name,weights,hyp,actual,valid,picks,want_w,n_surv,fallback", [
    ("all candidates survive", [3, 3, 3, 3, 3], [7, 7, 7, 7, 7], 7, 1, [0, 1, 2], [3, 3, 3], 5, 0),
    ("survivors interleaved with non-survivors", [3, 3, 3, 3, 3], [1, 7, 2, 7, 7], 7, 1, [1, 3, 4], [3, 3, 3], 3, 0),
    ("fewer survivors than replicas", [3, 4, 5, 6, 7], [1, 2, 7, 4, 7], 7, 1, [2, 4, None], [5, 7, 0], 2, 0),
    ("no survivor: the unconditioned belief", [3, 4, 0, 6, 7], [1, 2, 3, 4, 5], 7, 1, [0, 1, 2], [3, 4, 0], 0, 1),
    ("no usable previous state", [3, 4, 5, 6, 7], [7, 7, 7, 7, 7], 7, 0, [0, 1, 2], [3, 4, 5], 0, 2),
    ("a weight-0 candidate whose move matches is no survivor", [0, 3, 0, 3, 3], [7, 1, 7, 7, 7], 7, 1, [3, 4, None], [3, 3, 0], 2, 0),
])
def test_hand_worked_selection(name, weights, hyp, actual, valid, picks, want_w, n_surv, fallback):
    m, K, R = 2, 5, 3
    src, det = _labelled(m, K)
    # root 1 is the case; root 0 is a root where candidates 4 and 2 alone survive, to show that roots do not leak into each other
    w = np.array([0, 0, 9, 0, 9] + weights, np.uint32)
    hyp_moves = np.stack([np.array([5, 5, 5, 5, 5]), np.array(hyp)], 1)   # [K, m]
    rows, ow, ns, fb = select_ref(src, det, w, hyp_moves, np.array([5, actual]), np.array([1, valid], np.uint8), K, R)
    assert [int(x) for x in ns] == [2, n_surv] and [int(x) for x in fb] == [0, fallback], name
    assert np.array_equal(rows[0], det[2]) and np.array_equal(rows[1], det[4]) and np.array_equal(rows[2], src[0])
    assert [int(x) for x in ow[:3]] == [9, 9, 0]
    for j, k in enumerate(picks):
        assert np.array_equal(rows[R + j], src[1] if k is None else det[K + k]), name
    assert [int(x) for x in ow[R:]] == want_w, name
    # valid = None means every root is valid
    if valid:
        again = select_ref(src, det, w, hyp_moves, np.array([5, actual]), None, K, R)
        assert all(np.array_equal(a, b) for a, b in zip(again, (rows, ow, ns, fb)))


def test_a_finished_root_is_never_filtered():
    m, K, R = 2, 5, 3
    src, det = _labelled(m, K)
    src[1, 0] = 2 << 19   # fireworks complete
    rows, ow, ns, fb = select_ref(src, det, np.zeros(m * K, np.uint32), np.full((K, m), 7), np.array([7, 7]), None, K, R)
    assert [int(x) for x in fb] == [1, 2] and [int(x) for x in ns] == [0, 0]   # (root 0: every candidate dead, so no survivor)
    assert np.array_equal(rows[R:], det[K:K + R]) and not ow.any()


def test_splice_changes_the_hand_word_only():
    rng = np.random.default_rng(3)
    m, K, SW, seat = 3, 4, 48, 3
    prev = rng.integers(0, 2 ** 32, (m, SW), dtype=np.uint64).astype(np.uint32)
    det = rng.integers(0, 2 ** 32, (m * K, SW), dtype=np.uint64).astype(np.uint32)
    out = splice_ref(prev, det, seat, K).reshape(K, m, SW)
    for k in range(K):
        for i in range(m):
            same = np.ones(SW, bool)
            same[10 + seat] = False
            assert np.array_equal(out[k, i][same], prev[i][same]) and out[k, i, 10 + seat] == det[i * K + k, 10 + seat]


# ---- exactness by enumeration -------------------------------------------------------------------------------------------------------
def _rules():
    from hanabi_hip import _capi as K

    return [(K.RULE_PLAY_SAFE_CARD, 0, 0.0), (K.RULE_TELL_PLAYABLE_CARD, 0, 0.0), (K.RULE_DISCARD_OLDEST_FIRST, 0, 0.0)]


def _replay(cfg, deck, moves):
    O = _oracle()
    env = O.OracleEnv(cfg, 1, seed=1, decks=np.asarray(deck, np.uint8)[None])
    for u in moves:
        env.step(np.asarray([u], np.int32))
    assert env.illegal_count() == 0
    return env


def _hand_positions(cfg, moves):
    """Deck positions of every seat's hand slots (oldest first) after `moves`, and the first undealt position."""
    P, H = cfg.players, cfg.hand_size
    D = deck_size_of(cfg)
    hands = [list(range(p * H, (p + 1) * H)) for p in range(P)]
    pos, cur = P * H, 0
    for u in moves:
        if u < 2 * H:
            hands[cur].pop(u % H)
            if pos < D:
                hands[cur].append(pos)
                pos += 1
        cur = (cur + 1) % P
    return hands, pos


class Scene:
    """A Small 2-player game: `moves` played on `deck`, then the partner's rule-list move a_prev from S_prev to S; the observer
    is the seat to act in S. move_under(hand): what the partner's rule list plays in S_prev had the observer held `hand` —
    the same script replayed on a deck with the observer's cards swapped (a hand in the V0 support has, by definition, answered
    every hint given so far as the real one did, so the replay is legal and ends in S_prev with only that hand changed)."""

    def __init__(self, deck, moves):
        O = _oracle()
        self.cfg = O.make_config("Hanabi-Small", 2, 0)
        self.deck, self.moves = list(deck), list(moves)
        env = _replay(self.cfg, deck, moves)
        self.prev_row = env.export_state()[0]
        self.partner = (int(self.prev_row[0]) >> 13) & 7
        self.a_prev = int(env.rule_act(_rules(), 1, 1)[0][0])
        env.step(np.asarray([self.a_prev], np.int32))
        assert env.illegal_count() == 0
        self.row = env.export_state()[0]
        self.running = (int(self.row[0]) >> 19) & 3 == 0
        self.seat = (int(self.row[0]) >> 13) & 7
        hands, pos = _hand_positions(self.cfg, self.moves + [self.a_prev])
        self.my_pos, self.undealt = hands[self.seat], list(range(pos, len(deck)))
        self._cache = {}

    def move_under(self, hand):
        if hand not in self._cache:
            pool = [self.deck[q] for q in self.my_pos + self.undealt]
            deck = list(self.deck)
            for q, c in zip(self.my_pos, hand):
                pool.remove(c)
                deck[q] = c
            for q, c in zip(self.undealt, pool):
                deck[q] = c
            env = _replay(self.cfg, deck, self.moves)
            got = env.export_state()[0]
            same = np.ones(len(got), bool)
            same[10 + self.seat] = False
            same[10 + 3 * self.cfg.players:] = False
            assert np.array_equal(got[same], self.prev_row[same]), "the replay did not end in S_prev"
            self._cache[hand] = int(env.rule_act(_rules(), 1, 1)[0][0])
        return self._cache[hand]


# (script of tests/test_search_cpu.SMALL_SCRIPTS, moves of it played before the partner's rule-list move): found by a search
# over all prefixes for states where the hands under which the partner plays a_prev are a proper, non-empty part of the V0 support
SCENES = [(1, 14), (2, 12), (2, 19)]
R_EX, OVERSAMPLE_EX, CALLS_EX = 4, 4, 300


def _posterior(scene):
    exact = enumerate_hands(scene.cfg, scene.row, scene.seat)
    keep = {h: t for h, (t, _, _) in exact.items() if scene.move_under(h) == scene.a_prev}
    total, total_keep = sum(t for t, _, _ in exact.values()), sum(keep.values())
    return ({h: t / total for h, (t, _, _) in exact.items()}, {h: keep.get(h, 0) / total_keep for h in exact} if total_keep else None)


def _violations(freq, n, p):
    return [(h, p[h], freq.get(h, 0) / n) for h in p if abs(freq.get(h, 0) / n - p[h]) > 6 * math.sqrt(p[h] * (1 - p[h]) / n) + 1e-12]


@pytest.mark.parametrize("script,n_moves", SCENES)
def test_survivors_are_the_exact_posterior_by_enumeration(script, n_moves):
    """The restated pipeline (determinize, splice, the partner's move by the CPU rule oracle, select) against the exact
    posterior — uniform over the physical assignments in the V0 support under which the partner's rule list plays the move it
    played — within 6 sigma of the binomial deviation per hand (the bound of tests/test_search_cpu.py; the survivors of iid
    uniform candidates under a deterministic predicate are iid from the posterior). The unconditioned candidates miss it."""
    deck, moves = SMALL_SCRIPTS[script]
    sc = Scene(deck, moves[:n_moves])
    assert sc.running and sc.seat != sc.partner
    prior, post = _posterior(sc)
    assert post is not None and post[hand_types(sc.cfg, sc.row, sc.seat)] > 0   # the true hand is consistent with the move
    n_keep = sum(1 for v in post.values() if v > 0)
    assert 0 < n_keep < len(post), "the move tells the observer nothing about its hand: not a test of the filter"
    K = R_EX * OVERSAMPLE_EX
    cond, plain, n_cond, n_plain, n_fallback = {}, {}, 0, 0, 0
    for call in range(CALLS_EX):
        det, w = determinize_ref(sc.cfg, sc.row[None], sc.seat, K, 11, 3, first_row_id=call * K)
        hyp_rows = splice_ref(sc.prev_row[None], det, sc.seat, K)
        hyp = np.empty((K, 1), np.int64)
        for k in range(K):
            # what the spliced row shows the partner is the candidate's hand in S_prev
            assert hand_types(sc.cfg, hyp_rows[k], sc.seat) == hand_types(sc.cfg, det[k], sc.seat)
            hyp[k, 0] = sc.move_under(hand_types(sc.cfg, det[k], sc.seat))
        rows, ow, ns, fb = select_ref(sc.row[None], det, w, hyp, np.array([sc.a_prev]), None, K, R_EX)
        n_fallback += int(fb[0] != 0)
        if fb[0] == 0:
            for j in range(R_EX):
                if ow[j]:
                    h = hand_types(sc.cfg, rows[j], sc.seat)
                    cond[h] = cond.get(h, 0) + 1
                    n_cond += 1
        for k in range(R_EX):
            h = hand_types(sc.cfg, det[k], sc.seat)
            plain[h] = plain.get(h, 0) + 1
            n_plain += 1
    assert n_cond > 500 and set(cond) <= {h for h, v in post.items() if v > 0}
    assert min(v for v in post.values() if v > 0) * n_cond >= 20   # every kept hand is drawn often enough for the bound to bite
    assert not _violations(cond, n_cond, post), _violations(cond, n_cond, post)
    assert not _violations(plain, n_plain, prior)                  # (the candidates are the V0 belief)
    assert _violations(plain, n_plain, post), "the unconditioned belief passes: the test cannot see the filter"


# ---- last_move_uid ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("game,players", [("Hanabi-Full", 2), ("Hanabi-Full", 3), ("Hanabi-Small", 2)])
def test_last_move_uid_on_scripted_moves(game, players):
    import torch

    from hanabi_hip import last_move_uid

    O = _oracle()
    cfg = O.make_config(game, players, 0)
    # Small (one life) follows a script of careful play; Full walks through the legal uids so that every kind and, at three
    # players, both target offsets come up
    script = SMALL_SCRIPTS[0] if game == "Hanabi-Small" else None
    env = O.OracleEnv(cfg, 1, seed=5, decks=None if script is None else np.asarray(script[0], np.uint8)[None])
    assert int(last_move_uid(cfg, torch.as_tensor(env.export_state().astype(np.int64)))[0]) == -1   # no move yet: valid = 0
    H, kinds = cfg.hand_size, set()
    legal = env.observe()["legal"][0]
    for t in range(40 if script is None else len(script[1])):
        uids = np.flatnonzero(legal)
        uid = int(uids[(7 * t + 3) % len(uids)]) if script is None else script[1][t]
        mover = (int(env.export_state()[0, 0]) >> 13) & 7
        legal = env.step(np.asarray([uid], np.int32))["legal"][0]
        row = env.export_state()
        if (int(row[0, 0]) >> 19) & 3:
            break
        assert int(last_move_uid(cfg, torch.as_tensor(row.astype(np.int64)))[0]) == uid
        assert int(last_move_uid(cfg, torch.as_tensor(row.view(np.int32)))[0]) == uid    # (the int32 bits of an exported row)
        assert (int(row[0, 2]) >> 1) & 7 == mover
        kinds.add(0 if uid < H else 1 if uid < 2 * H else 2 if uid < 2 * H + (players - 1) * cfg.colors else 3)
        if players == 3 and uid >= 2 * H:
            kinds.add(4 + ((uid - 2 * H) // cfg.colors if uid < 2 * H + 2 * cfg.colors else (uid - 2 * H - 2 * cfg.colors) // cfg.ranks))
    assert {0, 1, 2, 3} <= kinds and (players != 3 or {4, 5} <= kinds)


# ---- declarations and argument validation ---------------------------------------------------------------------------------------------
def test_new_names_are_exported_and_declared():
    import hanabi_hip
    from hanabi_hip import _capi

    for name in ("ConditionedDeterminizer", "belief_splice", "belief_select", "last_move_uid"):
        assert hasattr(hanabi_hip, name) and name in hanabi_hip.__all__
    assert "hb_belief_splice" in _capi.SIGNATURES and "hb_belief_select" in _capi.SIGNATURES
    L = hanabi_hip.lib()
    assert L.hb_belief_splice and L.hb_belief_select


def test_argument_validation_needs_no_gpu():
    import hanabi_hip

    L = hanabi_hip.lib()
    cfg = hanabi_hip.make_config()
    ref, one = C.byref(cfg), C.c_void_p(16)
    err = lambda: L.hb_last_error()
    assert L.hb_belief_splice(None, one, one, 4, 0, 8, one, None) < 0 and b"null" in err()
    for bad in range(3):
        p = [one] * 3
        p[bad] = None
        assert L.hb_belief_splice(ref, p[0], p[1], 4, 0, 8, p[2], None) < 0 and b"null" in err()
    assert L.hb_belief_splice(ref, one, one, 4, -1, 8, one, None) < 0 and b"seat" in err()
    assert L.hb_belief_splice(ref, one, one, 4, 2, 8, one, None) < 0 and b"seat" in err()
    assert L.hb_belief_splice(ref, one, one, 4, 0, 0, one, None) < 0 and b"n_cand" in err()
    assert L.hb_belief_splice(ref, one, one, -1, 0, 8, one, None) < 0
    assert L.hb_belief_splice(ref, one, one, 1 << 20, 0, 64, one, None) < 0 and b"2^31" in err()   # 2^20 * 64 * 32 words
    assert L.hb_belief_splice(ref, one, one, 0, 0, 8, one, None) == 0                               # empty: no-op
    bad_cfg = hanabi_hip.HbConfig(6, 5, 5, 5, 8, 3, 0)
    assert L.hb_belief_splice(C.byref(bad_cfg), one, one, 4, 0, 8, one, None) < 0 and b"players" in err()

    def select(ptrs, m=4, k=8, r=3, cfg_ref=ref):
        p = list(ptrs)
        return L.hb_belief_select(cfg_ref, p[0], p[1], p[2], p[3], p[4], p[5], m, k, r, p[6], p[7], p[8], p[9], None)

    assert select([one] * 10, cfg_ref=None) < 0 and b"null" in err()
    for bad in range(10):
        p = [one] * 10
        p[bad] = None
        if bad == 5:   # valid may be NULL: the call gets as far as asking for a device, or launches
            continue
        assert select(p) < 0 and b"null" in err()
    assert select([one] * 10, r=0) < 0 and b"replicas" in err()
    assert select([one] * 10, k=2, r=3) < 0 and b"n_cand" in err()
    assert select([one] * 10, m=-1) < 0
    assert select([one] * 10, m=1 << 20, k=64, r=3) < 0 and b"2^31" in err()
    assert select([one] * 10, m=0) == 0
    assert select([one] * 5 + [None] + [one] * 4, m=0) == 0
    assert select([one] * 10, cfg_ref=C.byref(bad_cfg)) < 0 and b"players" in err()


class _Agent:
    def eval_moves(self, *a, **k):
        raise AssertionError("not called")


def test_history_and_condition_are_checked():
    import torch

    from hanabi_hip import RolloutSearch, SearchPlayer
    from hanabi_hip.search import _history

    rows = torch.zeros((4, 32), dtype=torch.int32)
    prev, seed, draw, gid, valid = _history((rows, 7, 3, 100), 4, 32, "cpu")
    assert prev.shape == (4, 32) and (seed, draw, gid, valid) == (7, 3, 100, None)
    assert _history((rows, 7, 3, 100, [1, 0, 1, 1]), 4, 32, "cpu")[4].tolist() == [1, 0, 1, 1]
    for bad in (rows, (rows, 7, 3), (rows, 7, 3, 100, None, None)):
        with pytest.raises(ValueError, match="history is"):
            _history(bad, 4, 32, "cpu")
    for bad_rows in (rows[:3], rows[:, :31], rows[0]):
        with pytest.raises(ValueError, match="previous rows"):
            _history((bad_rows, 7, 3, 100), 4, 32, "cpu")
    with pytest.raises(ValueError, match="valid mask"):
        _history((rows, 7, 3, 100, [1, 0, 1]), 4, 32, "cpu")
    with pytest.raises(ValueError, match="oversample"):
        RolloutSearch(oversample=0)
    with pytest.raises(ValueError, match="oversample"):
        SearchPlayer([_Agent(), _Agent()], 0, condition=True, oversample=0)
    with pytest.raises(ValueError, match="2 players"):
        SearchPlayer([_Agent(), _Agent(), _Agent()], 0, condition=True)
    sp = SearchPlayer([_Agent(), _Agent()], 1, condition=True)
    assert sp.condition and sp.oversample == 8
    assert (sp.conditioned, sp.unconditioned, sp.survivors, sp.candidates, sp.fallbacks) == (0, 0, 0, 0, 0)
    plain = SearchPlayer([_Agent(), _Agent(), _Agent()], 0)
    assert not plain.condition
