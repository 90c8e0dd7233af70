"""Screen-then-confirm search, the parts that need no GPU: a restatement of hb_search_compare's rule (include/hanabi_hip.h) in
Python integers and math.fsum, hand-worked cases of it, the argument validation of hb_search_layout and hb_search_compare, and
SearchPlayer's new arguments. tests/test_search_confirm_gpu.py holds the kernels to this restatement."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest


def compare_ref(scores, weights, cand, base_slot):
    """hb_search_compare: scores [m, C, R] int, weights [m, R] unsigned, cand [m, C] int, base_slot [m] int ->
    (diff [m, C] f64, se [m, C] f64, n_pair [m] int32). The integer sums in Python ints, the second pass with math.fsum."""
    scores, weights, cand, base_slot = (np.asarray(x) for x in (scores, weights, cand, base_slot))
    m, Cn, R = scores.shape
    diff = np.full((m, Cn), np.nan)
    se = np.full((m, Cn), np.nan)
    n_pair = np.zeros(m, np.int32)
    for i in range(m):
        w = [int(x) for x in weights[i]]
        sw, n = sum(w), sum(1 for x in w if x > 0)
        n_pair[i] = n
        base = int(base_slot[i])
        if not 0 <= base < Cn or sw == 0 or cand[i, base] < 0:
            continue
        sb = [int(x) for x in scores[i, base]]
        for c in range(Cn):
            if cand[i, c] < 0:
                continue
            if c == base:
                diff[i, c] = se[i, c] = 0.0
                continue
            d = [int(x) - y for x, y in zip(scores[i, c], sb)]
            mu = float(sum(wr * dr for wr, dr in zip(w, d))) / float(sw)
            diff[i, c] = mu
            if n < 2:
                se[i, c] = math.inf
                continue
            terms = [float(wr) * (float(dr) - mu) for wr, dr in zip(w, d) if wr > 0]
            se[i, c] = math.sqrt(math.fsum(t * t for t in terms)) / float(sw) * math.sqrt(float(n) / float(n - 1))
    return diff, se, n_pair


def test_constant_weights_give_the_textbook_standard_error():
    rng = np.random.default_rng(1)
    for R, wt in ((2, 1), (7, 6), (33, 3125), (130, 55 ** 5)):
        scores = rng.integers(0, 26, (3, 4, R))
        weights = np.full((3, R), wt, np.uint64)
        cand = np.array([[3, 7, 1, 0]] * 3)
        base = np.array([0, 2, 3])
        diff, se, n_pair = compare_ref(scores, weights, cand, base)
        assert list(n_pair) == [R] * 3
        for i in range(3):
            for c in range(4):
                d = (scores[i, c] - scores[i, base[i]]).astype(np.float64)
                if c == base[i]:
                    assert diff[i, c] == 0.0 and se[i, c] == 0.0
                else:
                    assert diff[i, c] == pytest.approx(d.mean(), rel=1e-13, abs=1e-13)
                    assert se[i, c] == pytest.approx(np.std(d, ddof=1) / math.sqrt(R), rel=1e-12, abs=1e-13)


def test_hand_worked_cases():
    # two candidates, three live replicas of weight 2 and a dead one: d = (3, -1, 1) -> mean 1, s^2 = 4, se = 2 / sqrt(3)
    scores = np.array([[[10, 12, 9, 25], [13, 11, 10, 0]]])
    weights = np.array([[2, 2, 2, 0]])
    diff, se, n_pair = compare_ref(scores, weights, [[4, 9]], [0])
    assert n_pair[0] == 3 and diff[0, 0] == 0.0 and se[0, 0] == 0.0
    assert diff[0, 1] == 1.0 and se[0, 1] == pytest.approx(2 / math.sqrt(3), rel=1e-15)
    # the other way round: the sign flips, the error does not
    diff2, se2, _ = compare_ref(scores, weights, [[4, 9]], [1])
    assert diff2[0, 0] == -1.0 and se2[0, 0] == se[0, 1] and diff2[0, 1] == 0.0 and se2[0, 1] == 0.0
    # one live replica: the difference is that replica's, its error is unknown
    diff, se, n_pair = compare_ref(scores, [[0, 0, 7, 0]], [[4, 9]], [0])
    assert n_pair[0] == 1 and diff[0, 1] == 1.0 and se[0, 1] == math.inf and (diff[0, 0], se[0, 0]) == (0.0, 0.0)
    # a slot without a candidate, a root without a baseline, a baseline slot without a candidate, a root without a live replica
    diff, se, _ = compare_ref(scores, weights, [[4, -1]], [0])
    assert math.isnan(diff[0, 1]) and math.isnan(se[0, 1]) and diff[0, 0] == 0.0
    for cand, base, w in (([[4, 9]], [-1], weights), ([[-1, 9]], [0], weights), ([[4, 9]], [0], [[0, 0, 0, 0]]), ([[4, 9]], [2], weights)):
        diff, se, _ = compare_ref(scores, w, cand, base)
        assert np.isnan(diff).all() and np.isnan(se).all()


def test_weights_that_differ():
    """The crossed-knowledge states of test_search_cpu (no play reaches them): replicas of one root carry different weights.
    Against exact rational arithmetic."""
    from test_search_cpu import crossed_states, determinize_ref

    states = crossed_states()
    cfg = states[0][0]
    rows = np.stack([r for _, r in states]).astype(np.uint32)
    R = 24
    _, w = determinize_ref(cfg, rows, -1, R, 3, 9)
    w = w.reshape(len(states), R)
    assert all(len(set(int(x) for x in w[i] if x > 0)) >= 2 for i in range(len(states)))
    rng = np.random.default_rng(4)
    scores = rng.integers(0, 11, (len(states), 2, R))
    diff, se, n_pair = compare_ref(scores, w, [[0, 1]] * len(states), [0] * len(states))
    for i in range(len(states)):
        wi = [int(x) for x in w[i]]
        d = [int(scores[i, 1, r]) - int(scores[i, 0, r]) for r in range(R)]
        sw, n = sum(wi), sum(1 for x in wi if x > 0)
        mu = Fraction(sum(a * b for a, b in zip(wi, d)), sw)
        ss = sum((a * (b - mu)) ** 2 for a, b in zip(wi, d))
        assert n_pair[i] == n and diff[i, 1] == pytest.approx(float(mu), rel=1e-15, abs=1e-300)
        assert se[i, 1] == pytest.approx(math.sqrt(ss * n / (n - 1)) / sw, rel=1e-12)
        # not the unweighted formula: the weights matter
        live = [b for a, b in zip(wi, d) if a > 0]
        assert abs(diff[i, 1] - sum(live) / n) > 1e-9 or abs(se[i, 1] - np.std(live, ddof=1) / math.sqrt(n)) > 1e-9


def test_new_entry_points_are_declared():
    from hanabi_hip import _capi

    assert "hb_search_layout" in _capi.SIGNATURES and "hb_search_compare" in _capi.SIGNATURES
    from hanabi_hip.search import RolloutSearch, SearchResult

    for name in ("run_candidates", "confirm"):
        assert callable(getattr(RolloutSearch, name))
    res = SearchResult(None, None, None, None, 0, 0)
    assert res.diff is None and res.se is None and res.n_pair is None and res.cand is None


def test_argument_validation_needs_no_gpu():
    import hanabi_hip

    L = hanabi_hip.lib()
    cfg = hanabi_hip.make_config()
    ref = C.byref(cfg)
    one = C.c_void_p(16)
    err = lambda: L.hb_last_error()

    def layout(cfg_ref=ref, m=4, c=2, r=8, **null):
        p = [None if null.get(k) else one for k in ("det", "w", "cand", "filler", "rows", "forced", "done", "n_played")]
        return L.hb_search_layout(cfg_ref, p[0], p[1], p[2], p[3], m, c, r, p[4], p[5], p[6], p[7], None)

    def compare(m=4, c=2, r=8, **null):
        p = [None if null.get(k) else one for k in ("score", "w", "cand", "base", "diff", "se", "n_pair")]
        return L.hb_search_compare(p[0], p[1], p[2], p[3], m, c, r, p[4], p[5], p[6], None)

    assert layout(cfg_ref=None) < 0 and b"null" in err()
    bad = hanabi_hip.HbConfig(6, 5, 5, 5, 8, 3, 0)
    assert layout(cfg_ref=C.byref(bad)) < 0 and b"players" in err()
    for k in ("det", "w", "cand", "filler", "rows", "forced", "done", "n_played"):
        assert layout(**{k: True}) < 0 and b"null" in err()
    for k in ("score", "w", "cand", "base", "diff", "se", "n_pair"):
        assert compare(**{k: True}) < 0 and b"null" in err()
    for fn in (layout, compare):
        assert fn(m=-1) < 0 and len(err()) > 0
        assert fn(c=0) < 0 and b"n_cand" in err()
        assert fn(c=65) < 0 and b"n_cand" in err()
        assert fn(r=0) < 0 and b"replicas" in err()
        assert fn(m=1 << 25, c=64, r=1) < 0 and b"2^31" in err()         # m * C * R = 2^31
        assert fn(m=(1 << 31) // 48 + 1, c=2, r=24) < 0 and b"2^31" in err()
        assert fn(m=0) == 0                                               # empty: a no-op
    assert layout(m=0, c=64, r=1 << 30) == 0
    assert compare(r=(1 << 20) + 1) < 0 and b"replicas" in err()


class _Agent:
    def eval_moves(self, *a, **k):
        raise AssertionError("not called")

    def requires_vectorized_observation(self):
        return False


def test_search_player_checks_its_new_arguments():
    from hanabi_hip import SearchPlayer

    team = [_Agent(), _Agent()]
    for z in (-1, -1e-9, float("nan")):
        with pytest.raises(ValueError, match="z must be"):
            SearchPlayer(team, 0, z=z)
    with pytest.raises(ValueError, match="confirm_replicas"):
        SearchPlayer(team, 0, confirm_replicas=-1)
    sp = SearchPlayer(team, 1, z=0, confirm_replicas=256)
    assert sp.z == 0.0 and sp.confirm_replicas == 256
    assert (sp.confirmed, sp.rejected, sp.rollouts, sp.moves, sp.deviations) == (0, 0, 0, 0, 0)
    sp = SearchPlayer(team, 1)
    assert sp.z is None and sp.confirm_replicas == 0
    assert SearchPlayer(team, 0, z=math.inf).z == math.inf
