"""Scoring a belief against the true hand, the parts that need no GPU (hanabi_hip.search, include/hanabi_hip.h): the numpy
restatement `belief_score_ref` against a brute-force tally, its card-counting prior against an independent count of the cards a
seat cannot see, its marginals against the exact enumeration of tests/test_search_cpu.py, `BeliefScore`'s arithmetic on hand-made
numbers, and the argument checks. tests/test_belief_score_gpu.py holds hb_belief_score to the restatement bit for bit."""
import ctypes as C
import math

import numpy as np
import pytest
from test_search_cpu import (FULL_SCRIPT, SMALL_SCRIPTS, _check_state_is_a_real_test, deck_size_of, determinize_ref, enumerate_hands,
                             plausible, played_states, random_play_rows, scripted_state, seat_view)


def _seat(cfg, row, seat):
    w0 = int(row[0])
    st = seat if seat >= 0 else (w0 >> 13) & 7
    return None if (w0 >> 19) & 3 or st >= cfg.players else st


def brute_force(cfg, rows, det, w, seat, R):
    """The tally with whole-array numpy operations per root (belief_score_ref walks replica by replica)."""
    rows, det, w = np.asarray(rows, np.uint32), np.asarray(det, np.uint32), np.asarray(w, np.uint32).astype(np.int64)
    m, H, NC = rows.shape[0], cfg.hand_size, cfg.colors * cfg.ranks
    truth, counts = np.full((m, H), -1, np.int64), np.zeros((m, H, NC), np.int64)
    hit, joint, wsum, n_live = np.zeros((m, H), np.int64), np.zeros(m, np.int64), np.zeros(m, np.int64), np.zeros(m, np.int64)
    for i in range(m):
        st = _seat(cfg, rows[i], seat)
        if st is None:
            continue
        n = min((int(rows[i, 1]) >> (15 + 3 * st)) & 7, H)
        shifts = 5 * np.arange(n, dtype=np.uint32)
        true = (rows[i, 10 + st] >> shifts) & 31
        field = (det[i * R:(i + 1) * R, 10 + st, None] >> shifts[None]) & 31   # [R, n]
        wi = w[i * R:(i + 1) * R]
        truth[i, :n] = true
        counts[i, :n] = np.einsum("r,rsc->sc", wi, field[:, :, None] == np.arange(NC)[None, None])
        same = (field == true[None]) & (field < NC)
        hit[i, :n] = wi @ same
        joint[i] = wi @ same.all(1)
        wsum[i], n_live[i] = wi.sum(), np.count_nonzero(wi)
    return dict(truth=truth, hit=hit, joint=joint, wsum=wsum, n_live=n_live, counts=counts)


def _same(got, want):
    for k, v in want.items():
        assert np.array_equal(got[k].astype(np.int64), v), k


def _scripted():
    return [scripted_state("Hanabi-Small", 2, deck, moves) for deck, moves in SMALL_SCRIPTS] + [scripted_state("Hanabi-Full", 2, *FULL_SCRIPT)]


# ---- 1. the restatement against a brute-force tally -------------------------------------------------------------------------------
def test_restatement_equals_a_brute_force_tally():
    from hanabi_hip import belief_score_ref

    R = 24
    for n_state, (cfg, row) in enumerate(_scripted()):
        st, H, NC = (int(row[0]) >> 13) & 7, cfg.hand_size, cfg.colors * cfg.ranks
        rows = np.stack([row, row, row, row]).astype(np.uint32)
        det, w = determinize_ref(cfg, rows, -1, R, seed=5, draw=n_state, first_row_id=100)
        assert (w != 0).all()
        rng = np.random.default_rng(n_state)
        # root 0: some weights zeroed; a weight-0 copy of the true hand among them
        w[:R][rng.random(R) < 0.4] = 0
        det[3], w[3] = row, 0
        # root 1: every replica holds the true hand
        det[R:2 * R, 10 + st] = row[10 + st]
        # root 2: slots holding 31, and ids >= NC
        for r in range(0, R, 3):
            s = r % H
            bad = 31 if r % 2 else min(NC + r % 4, 31)
            det[2 * R + r, 10 + st] = (int(det[2 * R + r, 10 + st]) & ~(31 << (5 * s))) | (bad << (5 * s))
        # root 3: every replica dead
        w[3 * R:] = 0
        for seat in (-1, st, 1 - st):
            got = belief_score_ref(cfg, rows.view(np.int32), det.view(np.int32), w.view(np.int32), seat, R)
            _same(got, brute_force(cfg, rows, det, w, seat, R))
            assert got["truth"].dtype == np.int8 and got["hit"].dtype == np.int64 and got["n_live"].dtype == np.int32
            assert got["prior"].dtype == np.int8 and got["prior"].shape == (4, H, NC)
        got = belief_score_ref(cfg, rows, det, w, -1, R)
        wl = w.reshape(4, R).astype(np.int64)
        assert got["wsum"][0] == wl[0].sum() and 0 < got["n_live"][0] < R
        # the dead copy of the true hand counts nothing: the tally is that of the live replicas alone
        live = wl[0] != 0
        alone = belief_score_ref(cfg, rows[:1], det[:R][live], wl[0][live], -1, int(live.sum()))
        for k in ("hit", "joint", "wsum", "n_live", "counts"):
            assert np.array_equal(alone[k][0], got[k][0]), k
        # all true hands: hit == joint == wsum
        assert (got["hit"][1] == got["wsum"][1]).all() and got["joint"][1] == got["wsum"][1] == wl[1].sum()
        # 31 and ids >= NC match nothing: the per-card tallies of a slot add up to less than wsum exactly by those replicas
        assert (got["counts"][2].sum(1) < got["wsum"][2]).any() and (got["counts"][2].sum(1) <= got["wsum"][2]).all()
        assert got["joint"][2] <= got["hit"][2].min()
        assert got["wsum"][3] == 0 and got["n_live"][3] == 0 and not got["hit"][3].any() and (got["truth"][3] >= 0).all()


# ---- 2. the prior against an independent count ------------------------------------------------------------------------------------
def _pool_count(cfg, row, st):
    """Copies of every card that seat `st` cannot see: all copies, minus the discard pile (the thermometers of words 8-9), minus
    the fireworks, minus every other seat's hand."""
    P, Cn, Rn = cfg.players, cfg.colors, cfg.ranks
    copies = [3 if r == 0 else 1 if r == Rn - 1 else 2 for r in range(Rn)]
    disc = int(row[8]) | int(row[9]) << 32
    left = np.zeros(Cn * Rn, np.int64)
    for col in range(Cn):
        fire = (int(row[1]) >> (3 * col)) & 7
        for r in range(Rn):
            pos = col * sum(copies) + sum(copies[:r])
            gone = bin((disc >> pos) & ((1 << copies[r]) - 1)).count("1")
            left[col * Rn + r] = copies[r] - gone - (1 if r < fire else 0)
    for p in range(P):
        if p != st:
            for s in range((int(row[1]) >> (15 + 3 * p)) & 7):
                left[(int(row[10 + p]) >> (5 * s)) & 31] -= 1
    return left


def _check_prior(cfg, rows, seen):
    """belief_score_ref's truth and prior on `rows` (scored against themselves: the replica IS the true row), for the seat to
    act and for the last seat, against _pool_count and the slots' knowledge bits."""
    from hanabi_hip import belief_score_ref

    rows = np.asarray(rows).astype(np.uint32)
    players, H, NC = cfg.players, cfg.hand_size, cfg.colors * cfg.ranks
    for seat in (-1, players - 1):
        got = belief_score_ref(cfg, rows, rows, np.ones(len(rows), np.uint32), seat, 1)
        for i, row in enumerate(rows):
            st = _seat(cfg, row, seat)
            if st is None:
                seen["finished"] += 1
                assert (got["truth"][i] == -1).all() and not got["prior"][i].any() and not got["hit"][i].any()
                assert got["wsum"][i] == 0 and got["joint"][i] == 0 and got["n_live"][i] == 0 and not got["counts"][i].any()
                continue
            seen["live"] += 1
            n = (int(row[1]) >> (15 + 3 * st)) & 7
            deck_size = int(row[0]) & 63
            know = int(row[10 + players + 2 * st]) | int(row[10 + players + 2 * st + 1]) << 32
            left = _pool_count(cfg, row, st)
            assert (left >= 0).all() and left.sum() == n + deck_size
            seen["short"] += n < H
            seen["empty_deck"] += deck_size == 0
            for s in range(H):
                if s >= n:
                    assert got["truth"][i, s] == -1 and not got["prior"][i, s].any() and got["hit"][i, s] == 0
                    continue
                t = (int(row[10 + st]) >> (5 * s)) & 31
                ok = np.array([plausible(cfg, know, s, c) for c in range(NC)])
                seen["hinted"] += not ok.all()
                assert got["truth"][i, s] == t and np.array_equal(got["prior"][i, s], np.where(ok, left, 0))
                assert got["prior"][i, s, t] >= 1   # reached by play: the true card is in the pool and plausible
            # the replica IS the true row: everything hits
            assert (got["hit"][i, :n] == 1).all() and got["joint"][i] == 1


GAMES = [("Hanabi-Full", 2), ("Hanabi-Full", 5), ("Hanabi-Small", 2)]


@pytest.mark.parametrize("game,players", GAMES)
def test_prior_is_the_count_of_unseen_cards_under_the_hints(game, players):
    seen = dict.fromkeys(("finished", "short", "empty_deck", "hinted", "live"), 0)
    for turns in (0, 20, 60):
        cfg, rows = random_play_rows(game, players, 24, seed=17 + turns, turns=turns)
        _check_prior(cfg, rows, seen)
    # (Small has one life: every randomly played game is over by turn 20, and at turn 0 nobody has been told anything)
    assert seen["live"] and seen["finished"] and (seen["hinted"] or game == "Hanabi-Small")


@pytest.mark.parametrize("game,players", GAMES)
def test_prior_with_an_empty_deck_and_a_short_hand(game, players):
    """Uniform random play loses its lives long before the deck runs out (tests/deep_play.py), so the rows above hold neither
    an empty deck nor a short hand: the open-handed driver of the deep-play tests reaches both."""
    from deep_play import open_hand_moves
    from oracle import oracle_py as O

    cfg = O.make_config(game, players, 0)
    env = O.OracleEnv(cfg, 16, seed=9)
    legal, rng = env.observe()["legal"], np.random.default_rng(4)
    seen = dict.fromkeys(("finished", "short", "empty_deck", "hinted", "live"), 0)
    for t in range(76):
        if t >= 10 and (t % 5 == 0 or (env.export_state()[:, 0] & 63).min() == 0):   # every turn once a deck has run out
            _check_prior(cfg, env.export_state(), seen)
        legal = env.step(open_hand_moves(cfg, env.export_state(), legal, rng, 0.05))["legal"]
    assert seen["short"] and seen["empty_deck"] and seen["hinted"] and seen["finished"]


# ---- 3. the marginals against the exact enumeration -------------------------------------------------------------------------------
R_LIVE, R_DEAD = 2000, 1000


def _marginal_violations(cfg, exact, sc, n):
    """(slot, card) marginals and the joint of the true hand further than 6 binomial standard errors from the exact value."""
    total = sum(t for t, _, _ in exact.values())
    H, NC = cfg.hand_size, cfg.colors * cfg.ranks
    p = np.zeros((H, NC))
    for hand, (t, _, _) in exact.items():
        for s, c in enumerate(hand):
            p[s, c] += t / total
    est = sc["counts"][0] / sc["wsum"][0]
    bad = [(s, c, est[s, c], p[s, c]) for s in range(H) for c in range(NC)
           if abs(est[s, c] - p[s, c]) > 6 * math.sqrt(max(p[s, c] * (1 - p[s, c]), 0.0) / n) + 1e-12]
    true = tuple(int(x) for x in sc["truth"][0])
    pj = exact[true][0] / total
    if abs(sc["joint"][0] / sc["wsum"][0] - pj) > 6 * math.sqrt(max(pj * (1 - pj), 0.0) / n) + 1e-12:
        bad.append(("joint", sc["joint"][0] / sc["wsum"][0], pj))
    return bad


def test_marginals_agree_with_the_exact_enumeration():
    """On states reached by play the weights are constant, so R_LIVE replicas are R_LIVE uniform draws from the V0 belief and a
    marginal's standard error is the binomial one. R_DEAD dead replicas follow them, unchanged copies of the true row with
    weight 0 (what the filters hand out when they run short of survivors): the scorer must not count them. One that does, with
    the weight the live ones carry, puts a third more mass on the true hand and must miss the bound."""
    from hanabi_hip import belief_score_ref

    wrong_misses = 0
    for n_state, (cfg, row) in enumerate(played_states()):
        exact = enumerate_hands(cfg, row, -1)
        _check_state_is_a_real_test(cfg, row, exact)
        assert min(p for _, _, p in exact.values()) * R_LIVE >= 5
        det, w = determinize_ref(cfg, row[None], -1, R_LIVE, seed=21, draw=n_state)
        assert len(set(w.tolist())) == 1 and w[0] != 0
        det = np.concatenate([det, np.repeat(np.asarray(row, np.uint32)[None], R_DEAD, 0)])
        w_all = np.concatenate([w, np.zeros(R_DEAD, np.uint32)])
        sc = belief_score_ref(cfg, row[None], det, w_all, -1, R_LIVE + R_DEAD)
        assert sc["n_live"][0] == R_LIVE and sc["wsum"][0] == R_LIVE * int(w[0])
        assert not _marginal_violations(cfg, exact, sc, R_LIVE)
        wrong = belief_score_ref(cfg, row[None], det, np.full(R_LIVE + R_DEAD, w[0], np.uint32), -1, R_LIVE + R_DEAD)
        wrong_misses += bool(_marginal_violations(cfg, exact, wrong, R_LIVE + R_DEAD))
    assert wrong_misses >= 1, "a scorer that counts the dead replicas passes on every state: the bound does not bite"


# ---- 4. BeliefScore's arithmetic ----------------------------------------------------------------------------------------------------
def _hand_made():
    """Three roots, H = 2, NC = 4. Root 0: wsum 8 over 3 live replicas, slot 0 hit by 6, slot 1 by none. Root 1: one slot only.
    Root 2: running, no live replica (unscored)."""
    truth = np.array([[1, 2], [3, -1], [0, 1]], np.int8)
    hit = np.array([[6, 0], [5, 0], [0, 0]], np.int64)
    joint, wsum, n_live = np.array([0, 5, 0], np.int64), np.array([8, 10, 0], np.int64), np.array([3, 1, 0], np.int32)
    prior = np.zeros((3, 2, 4), np.int8)
    prior[0, 0], prior[0, 1], prior[1, 0], prior[2, 0], prior[2, 1] = [1, 1, 0, 2], [0, 3, 1, 0], [2, 2, 2, 2], [1, 0, 0, 0], [0, 1, 0, 0]
    return dict(truth=truth, hit=hit, joint=joint, wsum=wsum, n_live=n_live, prior=prior)


def test_belief_score_arithmetic_on_hand_made_numbers():
    from hanabi_hip import BeliefScore, belief_figures

    b = BeliefScore(**_hand_made())
    assert b.scored.tolist() == [True, True, False]
    q = [6 / 8, 0.0, 5 / 10]           # hit / wsum of the three scored cards
    pr = [1 / 4, 1 / 4, 2 / 8]         # prior[truth] / sum prior
    lam = [1 / 4, 1 / 4, 1 / 2]        # 1 / (n_live + 1)
    assert b.hit_rate() == pytest.approx(sum(q) / 3) and b.prior_rate() == pytest.approx(sum(pr) / 3)
    assert b.joint_rate() == pytest.approx((0 / 8 + 5 / 10) / 2)
    want = -sum(math.log((1 - l) * x + l * p) for x, p, l in zip(q, pr, lam)) / 3
    assert b.cross_entropy() == pytest.approx(want, rel=1e-12) and math.isfinite(want)   # the card with hit = 0 stays finite
    want = -sum(math.log(0.9 * x + 0.1 * p) for x, p in zip(q, pr)) / 3
    assert b.cross_entropy(0.1) == pytest.approx(want, rel=1e-12)
    assert b.cross_entropy(0.0) == math.inf                                               # ... and only because of the mixture
    assert b.prior_cross_entropy() == pytest.approx(-sum(math.log(p) for p in pr) / 3, rel=1e-12)
    assert b.cross_entropy(1.0) == pytest.approx(b.prior_cross_entropy(), rel=1e-12)
    f = b.figures()
    assert f["cards"] == 3 and f["roots"] == 2
    s = f["by_slot"]
    assert s["cards"] == [2, 1] and sum(s["cards"]) == f["cards"]
    assert s["hit_rate"] == pytest.approx([(q[0] + q[2]) / 2, q[1]])
    for k in ("hit_rate", "prior_rate", "cross_entropy", "prior_cross_entropy"):   # the slots add back up to the total
        assert sum(v * n for v, n in zip(s[k], s["cards"])) / f["cards"] == pytest.approx(f[k], rel=1e-12)
    # the unscored root changes nothing, whatever it holds
    d = _hand_made()
    d["hit"][2], d["joint"][2] = [99, 99], 99
    assert BeliefScore(**d).figures() == f
    # a mask, and sums that add up
    import torch

    one, other = b.sums(where=torch.tensor([True, False, False])), b.sums(where=torch.tensor([False, True, True]))
    assert one.shape == (len(BeliefScore.SUMS), 2) and one.dtype == torch.float64
    assert torch.allclose(one + other, b.sums(), rtol=1e-12, atol=0)
    assert belief_figures(one)["cards"] == 2 and belief_figures(other)["roots"] == 1
    # an edited row whose hints exclude the true card: nothing to mix in, inf
    d = _hand_made()
    d["prior"][0, 1, 2] = 0
    assert BeliefScore(**d).cross_entropy() == math.inf
    zeros = belief_figures(None)
    assert zeros["cards"] == 0 and zeros["roots"] == 0 and zeros["hit_rate"] == 0.0 and zeros["cross_entropy"] == 0.0
    assert zeros["by_slot"]["cards"] == []


def test_figures_of_the_restatement_on_true_hand_replicas():
    from hanabi_hip import BeliefScore, belief_score_ref

    cfg, rows = random_play_rows("Hanabi-Full", 2, 8, seed=3, turns=20)
    rows = np.asarray(rows).astype(np.uint32)
    b = BeliefScore(**belief_score_ref(cfg, rows, np.repeat(rows, 2, 0), np.full(16, 7, np.uint32), -1, 2))
    assert b.hit_rate() == 1.0 and b.joint_rate() == 1.0 and 0.0 < b.prior_rate() < 1.0
    assert 0.0 < b.cross_entropy() < b.prior_cross_entropy() < math.log(45)   # (a pool holds at most 45 cards)


# ---- 5. argument checks -------------------------------------------------------------------------------------------------------------
def test_the_symbol_is_declared_exported_and_bound():
    import hanabi_hip
    from hanabi_hip import _capi

    assert "hb_belief_score" in _capi.SIGNATURES and len(_capi.SIGNATURES["hb_belief_score"][1]) == 15
    assert hasattr(hanabi_hip.lib(), "hb_belief_score")
    for name in ("belief_score", "belief_score_ref", "belief_figures", "BeliefScore"):
        assert hasattr(hanabi_hip, name) and name in hanabi_hip.__all__


def test_argument_validation_needs_no_gpu():
    import hanabi_hip

    L = hanabi_hip.lib()
    cfg = hanabi_hip.make_config()
    ref, one = C.byref(cfg), C.c_void_p(16)
    err = lambda: L.hb_last_error()
    good = [ref, one, one, one, 4, -1, 8, one, one, one, one, one, one, one, None]

    def call(**change):
        a = list(good)
        for k, v in change.items():
            a[int(k[1:])] = v
        return L.hb_belief_score(*a)

    assert call(a0=None) < 0 and b"null config" in err()
    for j in (1, 2, 3, 7, 8, 9, 10, 11, 13):
        assert call(**{f"a{j}": None}) < 0 and b"null argument" in err(), j
    assert call(a6=0) < 0 and b"replicas 0 out of range 1..2^20" in err()
    assert call(a6=(1 << 20) + 1) < 0 and b"replicas 1048577 out of range" in err()
    assert call(a5=2) < 0 and b"seat 2 out of range" in err()
    assert call(a5=-2) < 0 and b"seat -2 out of range" in err()
    assert call(a4=-1) < 0 and b"m must be >= 0" in err()
    assert call(a4=1 << 31) < 0 and b"2^31" in err()
    bad = hanabi_hip.HbConfig(6, 5, 5, 5, 8, 3, 0)
    assert call(a0=C.byref(bad)) < 0 and b"players" in err()
    assert call(a4=0) == 0                 # empty: a no-op
    assert call(a4=0, a12=None) == 0       # (counts may be null)
    # with everything in order the only thing missing here is a device (or, with one, the call would touch the fake pointers)
    import torch

    if not torch.cuda.is_available():
        assert call(a12=None) < 0 and b"device" in err()


class _Agent:
    def eval_moves(self, *a, **k):
        raise AssertionError("not called")

    def requires_vectorized_observation(self):
        return False


def test_python_arguments_are_checked():
    import torch

    import hanabi_hip
    from hanabi_hip import OffBeliefSession, RolloutSearch, SearchPlayer, belief_score

    team = [_Agent(), _Agent()]
    for bad in (1, "yes", None):
        with pytest.raises(TypeError, match="score_belief"):
            RolloutSearch(score_belief=bad)
        with pytest.raises(TypeError, match="score_belief"):
            SearchPlayer(team, 0, score_belief=bad)
    assert RolloutSearch().score_belief is False and RolloutSearch(score_belief=True).score_belief is True
    off, on = SearchPlayer(team, 0), SearchPlayer(team, 1, score_belief=True, condition=True)
    assert off.score_belief is False and on.score_belief is True and off._belief is None and on._belief is None
    for p in (off, on):
        st = p.belief_stats()
        assert st["cards"] == 0 and st["roots"] == 0 and st["by_slot"]["cards"] == []
        for k in ("hit_rate", "prior_rate", "joint_rate", "cross_entropy", "prior_cross_entropy"):
            assert st[k] == 0.0
    assert "conditioned" not in off.belief_stats()
    assert on.belief_stats()["conditioned"]["cards"] == 0 and on.belief_stats()["unconditioned"]["roots"] == 0
    on.reset_stats()
    assert on._belief is None

    class _Env:   # what OffBeliefSession looks at before it reaches the switch
        players, color_shuffled = 2, False

    with pytest.raises(TypeError, match="score_belief"):
        OffBeliefSession(_Env(), team, score_belief=1)
    assert OffBeliefSession.BELIEF_COUNTERS == ("belief_cards", "belief_hit_sum", "belief_prior_sum", "belief_joint_sum", "belief_roots")
    # the wrapper is GPU only, with the soft filter's wording
    cfg = hanabi_hip.make_config()
    rows = torch.zeros((2, 32), dtype=torch.int32)
    with pytest.raises(hanabi_hip.HbError, match="tensors of one GPU"):
        belief_score(cfg, rows, rows.repeat(3, 1), torch.ones(6, dtype=torch.int32), -1, 3)
    with pytest.raises(AssertionError):
        belief_score(cfg, rows, rows, torch.ones(6, dtype=torch.int32), -1, 3)
