"""Partner-response (convention) statistics, the parts that need no GPU: the numpy restatement `response_counts` on hand-written
logs, EvalResult.response_matrix (normalisation, pooling, the collapse to move kinds), convention_distance on synthetic counts,
and the argument checks of hb_eval_response_bins / hb_eval_response_tally / hb_eval_response_tally_grouped."""
import ctypes as C

import numpy as np
import pytest


def _sparse(shape, entries):
    out = np.zeros(shape, np.int64)
    for idx, v in entries.items():
        out[idx] = v
    return out


# 2 players, Hanabi-Small: H = 2, C = 2, R = 5 -> A = 11. uids 0-1 discard, 2-3 play, 4-5 reveal colour, 6-10 reveal rank.
# Three games of lengths 1, 4 and 0; turn t is seat t % 2.
HAND_LOG = np.array([[3, 5, 7],     # t0, seat 0: game 0's only move; game 1's first; game 2 never starts
                     [9, 2, 1],     # t1, seat 1: game 0 is over
                     [0, 5, 4],     # t2, seat 0
                     [0, 10, 4]],   # t3, seat 1
                    np.int32)
HAND_LENGTHS = np.array([1, 4, 0])
HAND_WANT = _sparse((2, 12, 11), {(0, 0, 3): 1, (0, 0, 5): 1,      # first moves: row 0
                                  (1, 5 + 1, 2): 1,                 # game 1, t1: 2 after 5
                                  (0, 2 + 1, 5): 1,                 # game 1, t2: 5 after 2
                                  (1, 5 + 1, 10): 1})               # game 1, t3: 10 after 5


def test_response_counts_hand_written_log():
    from hanabi_hip.evaluate import response_counts

    got = response_counts(HAND_LOG, HAND_LENGTHS, 2, 11)
    assert got.dtype == np.int64 and got.shape == (2, 12, 11)
    assert np.array_equal(got, HAND_WANT)
    assert got.sum() == HAND_LENGTHS.sum()
    assert got[:, 0].sum() == 2                                  # one first move per game that starts; the length-0 game adds nothing
    only_empty = response_counts(HAND_LOG[:, 2:], HAND_LENGTHS[2:], 2, 11)
    assert not only_empty.any()
    with pytest.raises(ValueError):
        response_counts(HAND_LOG, HAND_LENGTHS[:2], 2, 11)


def test_response_counts_three_players_first_seat():
    """Hanabi-Small, 3 players: A = 2 * 2 + 2 * 7 = 18; first_seat = 1, so turns 0, 1, 2 are seats 1, 2, 0. Game 2 holds uids
    outside 0 .. 17: they are not counted and do not become the previous move."""
    from hanabi_hip.evaluate import response_counts

    log = np.array([[4, 17, -1],
                    [0, 6, 2],
                    [12, 3, 18]], np.int32)
    lengths = np.array([3, 2, 3])
    want = _sparse((3, 19, 18), {(1, 0, 4): 1, (1, 0, 17): 1,
                                 (2, 4 + 1, 0): 1, (2, 17 + 1, 6): 1, (2, 0, 2): 1,   # game 2: still its first move
                                 (0, 0 + 1, 12): 1})
    assert np.array_equal(response_counts(log, lengths, 3, 18, first_seat=1), want)
    assert not np.array_equal(response_counts(log, lengths, 3, 18), want)


def _result(responses, kinds=None):
    from hanabi_hip import EvalResult

    return EvalResult([1], [1], 10, responses=responses, kinds=kinds)


def test_response_matrix_rows_sum_to_one_and_empty_rows_are_nan():
    rng = np.random.default_rng(0)
    c = rng.integers(0, 9, (2, 12, 11))
    c[0, 4] = 0
    c[1, 7] = 0
    c[:, 9] = 0
    r = _result(c)
    assert r.responses.dtype == np.int64 and np.array_equal(r.responses, c)
    for seat in (0, 1, None):
        m = r.response_matrix(seat=seat)
        assert m.dtype == np.float64 and m.shape == (12, 11)
        n = (c.sum(0) if seat is None else c[seat]).sum(-1)
        assert np.array_equal(np.isnan(m).all(-1), n == 0) and np.array_equal(np.isnan(m).any(-1), n == 0)
        assert np.allclose(m[n > 0].sum(-1), 1.0, rtol=0, atol=1e-12)
        assert np.array_equal(m[n > 0], (c.sum(0) if seat is None else c[seat])[n > 0] / n[n > 0, None])
    assert np.isnan(r.response_matrix(0)[4]).all() and not np.isnan(r.response_matrix(1)[4]).any()
    assert np.isnan(r.response_matrix()[9]).all()
    with pytest.raises(ValueError):
        _result(None).response_matrix()
    assert _result(None).responses is None


def test_response_matrix_pools_counts_not_probabilities():
    c = np.zeros((2, 12, 11), np.int64)
    c[0, 3, :2] = (1, 0)     # seat 0 answers move 2 once, with uid 0
    c[1, 3, :2] = (1, 3)     # seat 1 four times: once uid 0, three times uid 1
    m = _result(c).response_matrix()
    assert np.allclose(m[3, :2], (2 / 5, 3 / 5), rtol=0, atol=1e-15)     # (the mean of the two seats' rows would be 5/8, 3/8)
    assert np.allclose(_result(c).response_matrix(seat=1)[3, :2], (1 / 4, 3 / 4), rtol=0, atol=1e-15)


def test_response_matrix_kinds_against_hand_collapse():
    from hanabi_hip.evaluate import MOVE_KINDS, uid_kinds

    kinds = uid_kinds(2, 2, 2, 11)
    assert kinds.tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 3, 3, 3] and len(MOVE_KINDS) == 4
    assert uid_kinds(5, 5, 4, 48).tolist() == [0] * 4 + [1] * 4 + [2] * 20 + [3] * 20
    r = _result(HAND_WANT, kinds)
    nan = float("nan")
    # HAND_WANT by kinds: seat 0: none -> play (uid 3), none -> colour (uid 5), play (uid 2) -> colour (uid 5);
    #                     seat 1: colour (uid 5) -> play (uid 2), colour (uid 5) -> rank (uid 10)
    pooled = np.array([[0, .5, .5, 0],        # none
                       [nan] * 4,             # after a discard: never
                       [0, 0, 1, 0],          # after a play
                       [0, .5, 0, .5],        # after a colour reveal
                       [nan] * 4])            # after a rank reveal: never
    assert np.array_equal(r.response_matrix(kinds=True), pooled, equal_nan=True)
    seat0 = np.array([[0, .5, .5, 0], [nan] * 4, [0, 0, 1, 0], [nan] * 4, [nan] * 4])
    assert np.array_equal(r.response_matrix(seat=0, kinds=True), seat0, equal_nan=True)
    # a dense case: the collapse is a sum over the uids of each kind, on both axes
    c = np.random.default_rng(1).integers(0, 5, (2, 12, 11))
    rows = np.concatenate(([0], 1 + kinds))
    want = np.zeros((2, 5, 4), np.int64)
    for p in range(2):
        for i in range(12):
            for a in range(11):
                want[p, rows[i], kinds[a]] += c[p, i, a]
    got = _result(c, kinds).response_matrix(seat=1, kinds=True)
    assert np.array_equal(got, want[1] / want[1].sum(-1, keepdims=True))
    with pytest.raises(ValueError):
        _result(c).response_matrix(kinds=True)     # no uid kinds given


def test_as_dict_gains_responses_only_when_on():
    import json

    off, on = _result(None).as_dict(), _result(HAND_WANT).as_dict()
    assert "responses" not in off
    assert on["responses"] == HAND_WANT.tolist()
    assert {k: v for k, v in on.items() if k != "responses"} == off
    json.dumps(on)


def test_convention_distance_synthetic():
    from hanabi_hip import CrossPlayResult, EvalResult
    from hanabi_hip.crossplay import convention_distance

    P, A = 2, 3
    x = _sparse((P, A + 1, A), {(0, 1, 0): 4, (1, 2, 1): 2, (1, 2, 2): 2})
    y = _sparse((P, A + 1, A), {(0, 1, 1): 7, (1, 2, 0): 1, (0, 3, 0): 5})     # same rows as x (and one more), disjoint answers
    z = _sparse((P, A + 1, A), {(1, 0, 2): 3})                                  # no row in common with x or y
    d = convention_distance([x, x.copy(), y, z])
    assert d.dtype == np.float64 and d.shape == (4, 4)
    assert np.array_equal(d, d.T, equal_nan=True)
    assert np.array_equal(np.diag(d), np.zeros(4))
    assert d[0, 1] == 0.0                       # identical teams
    assert d[0, 2] == 1.0 and d[1, 2] == 1.0    # disjoint support on every shared row
    assert np.isnan(d[0, 3]) and np.isnan(d[2, 3])
    # weights: two shared rows, TV 1/2 on a row of 4 + 4 counts and TV 0 on a row of 1 + 3
    u = _sparse((P, A + 1, A), {(0, 0, 0): 4, (1, 1, 2): 1})
    v = _sparse((P, A + 1, A), {(0, 0, 0): 2, (0, 0, 1): 2, (1, 1, 2): 3, (1, 3, 1): 9})
    want = (8 * 0.5 + 4 * 0.0) / 12
    assert convention_distance([u, v])[0, 1] == pytest.approx(want, abs=1e-15)
    # scale: doubling a team's counts changes the weights, not its rows
    assert convention_distance([x, 2 * x])[0, 1] == 0.0
    with pytest.raises(ValueError):
        convention_distance(np.zeros((2, 3, 3)))
    # through the result object, in team order
    res = CrossPlayResult([(0, 0), (0, 1), (1, 0), (1, 1)], [EvalResult([1], [1], 10, responses=c) for c in (x, x, y, z)], 2, 2, True)
    assert res.responses.shape == (4, P, A + 1, A) and np.array_equal(res.responses[2], y)
    assert np.array_equal(res.convention_distance(), d, equal_nan=True)
    off = CrossPlayResult([(0, 0)], [EvalResult([1], [1], 10)], 1, 2, True)
    assert off.responses is None
    with pytest.raises(ValueError):
        off.convention_distance()


def test_switch_is_off_by_default_and_needs_no_device():
    from hanabi_hip import CrossPlay, Evaluator

    assert Evaluator(n_games=8).responses is False and CrossPlay(n_games=8).responses is False
    ev = Evaluator("Hanabi-Small", 2, n_games=8, responses=True)
    assert ev.responses is True and ev.env is None      # nothing touches the device before run()
    assert CrossPlay("Hanabi-Small", 2, n_games=8, responses=True).responses is True


def test_response_entry_points_check_their_arguments():
    import torch

    import hanabi_hip
    from hanabi_hip import _capi

    L = hanabi_hip.lib()
    err = L.hb_last_error
    for name in ("hb_eval_response_bins", "hb_eval_response_tally", "hb_eval_response_tally_grouped"):
        assert name in _capi.SIGNATURES and getattr(L, name)
    for game, players, a in (("Hanabi-Small", 2, 11), ("Hanabi-Full", 2, 20), ("Hanabi-Full", 5, 48), ("Hanabi-Small", 3, 18)):
        cfg = hanabi_hip.make_config(game, players)
        assert L.hb_num_actions(C.byref(cfg)) == a and L.hb_eval_response_bins(C.byref(cfg)) == (a + 1) * a
    assert L.hb_eval_response_bins(None) < 0 and b"null" in err()
    bad = hanabi_hip.HbConfig(6, 5, 5, 5, 8, 3, 0)
    assert L.hb_eval_response_bins(C.byref(bad)) < 0 and b"players" in err()

    cfg = hanabi_hip.make_config()
    ref = C.byref(cfg)
    one = C.c_void_p(16)      # a non-null fake pointer: validation must reject the call before using it
    # hb_eval_response_tally(cfg, n_games, seat, actions, done, prev, resp, stream)
    assert L.hb_eval_response_tally(None, 4, 0, one, one, one, one, None) < 0 and b"null" in err()
    for k in range(4):
        p = [one] * 4
        p[k] = None
        assert L.hb_eval_response_tally(ref, 4, 0, *p, None) == -1 and b"null" in err()
        assert L.hb_eval_response_tally_grouped(ref, 2, 4, 0, *p, None) == -1 and b"null" in err()
    assert L.hb_eval_response_tally(ref, 4, -1, one, one, one, one, None) == -1 and b"seat" in err()
    assert L.hb_eval_response_tally(ref, 4, 2, one, one, one, one, None) == -1 and b"seat" in err()
    assert L.hb_eval_response_tally(ref, -1, 0, one, one, one, one, None) == -1 and b"n_games" in err()
    assert L.hb_eval_response_tally(ref, 0, 0, one, one, one, one, None) == 0                       # empty: no-op
    assert L.hb_eval_response_tally(C.byref(bad), 4, 0, one, one, one, one, None) < 0 and b"players" in err()
    # hb_eval_response_tally_grouped(cfg, n_blocks, block_games, seat, actions, done, prev, resp, stream)
    assert L.hb_eval_response_tally_grouped(None, 2, 4, 0, one, one, one, one, None) < 0 and b"null" in err()
    assert L.hb_eval_response_tally_grouped(ref, 2, 4, 2, one, one, one, one, None) == -1 and b"seat" in err()
    assert L.hb_eval_response_tally_grouped(ref, 2, -1, 0, one, one, one, one, None) == -1
    assert L.hb_eval_response_tally_grouped(ref, -1, 4, 0, one, one, one, one, None) == -1 and b"n_blocks" in err()
    assert L.hb_eval_response_tally_grouped(ref, 65536, 4, 0, one, one, one, one, None) == -1 and b"n_blocks" in err()
    assert L.hb_eval_response_tally_grouped(ref, 1 << 15, 1 << 16, 0, one, one, one, one, None) == -1 and b"2^31" in err()
    assert L.hb_eval_response_tally_grouped(ref, 1, 1 << 31, 0, one, one, one, one, None) == -1 and b"2^31" in err()
    assert L.hb_eval_response_tally_grouped(ref, 0, 4, 0, one, one, one, one, None) == 0            # empty: no-ops
    assert L.hb_eval_response_tally_grouped(ref, 2, 0, 0, one, one, one, one, None) == 0
    assert L.hb_eval_response_tally_grouped(C.byref(bad), 2, 4, 0, one, one, one, one, None) < 0
    if not torch.cuda.is_available():      # valid arguments, no device: refused, nothing computed
        assert L.hb_eval_response_tally(ref, 4, 0, one, one, one, one, None) == -2
        assert L.hb_eval_response_tally_grouped(ref, 2, 4, 0, one, one, one, one, None) == -2
