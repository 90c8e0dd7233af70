"""The per-game tally models and the crafted steps of tests/tally_cases.py, without a GPU: hand-worked counters, a played oracle
game, the generator's coverage as conditions on the models' output, the teeth (five wrong models, each told from the right one by
the crafted steps; the first of them NOT told by 300 steps of uniform-random play, which is all hb_train_tally's counters had been
compared on), and PartnerStats against numpy."""
import collections
import functools
import math

import numpy as np
import pytest

import deep_play as D
import tally_cases as T
from oracle import oracle_py as O

HAND = T.Dims(P=2, H=2, C=2, R=3, A=9, max_life=2, B=7, max_info=3, deck=12)   # uids: 0-1 discard, 2-3 play, 4-5 colour, 6-8 rank
TURNS = 6
N_TRAIN = 384                       # three tiles, one per member: two waves each
TILE_MEMBER = np.array([0, 1, 2], np.int32)


def _cfg(game, players, flags=0):
    return O.make_config(game, players, flags)


def _step(actions, reward, terminal, score):
    return dict(actions=np.array(actions, np.int32), reward=np.array(reward, np.float32), terminal=np.array(terminal, np.int8),
                score=np.array(score, np.int8))


def test_dims_are_the_oracles():
    for game, players in T.VARIANTS + [("Hanabi-Small", 2)]:
        cfg = _cfg(game, players)
        d = T.dims_of(cfg)
        L = O.lib()
        assert d.A == L.orc_num_actions(cfg) and d.deck == L.orc_deck_size(cfg) and d.B == cfg.colors * cfg.ranks + 1
    assert [T.dims_of(_cfg(g, p)).B for g, p in T.VARIANTS] == [26, 26, 11, 6]
    assert [T.move_kind(HAND, u) for u in range(-1, 10)] == [None, 0, 0, 1, 1, 2, 2, 3, 3, 3, None]


# ---- hand-worked -----------------------------------------------------------------------------------------------------------------

def test_eval_model_by_hand():
    """Four games, three turns (seats 0, 1, 0), 2 lives. Game 3 was finished before (status 0x81) and is given a terminal, a score
    and a move every turn: none counts. Counter row: [0] live, [1..8) scores 0..6, [8] bomb-outs, [9 + 4 p + k] moves, [17 + p]
    misplays."""
    d = HAND
    cr = T.Crafted([
        # g0 plays and scores; g1 misplays (reward 0) and goes on; g2's uid 9 is no move
        _step([2, 3, 9, 0], [1, 0, 0, 0], [0, 0, 0, 1], [1, 0, 0, 5]),
        # g0 ends on a rank hint with lives left at score 7 (no such bin: the top one, 6); g1's second misplay (reward -3) ends it
        _step([6, 2, 4, 2], [0, -3, 0, 0], [1, 1, 0, 1], [7, 0, 0, 5]),
        # g2 ends on a uid that is no move (-1) at score 3; g0 and g1 are finished: their plays with reward 0 are no misplays
        _step([2, 2, -1, 2], [0, 0, 0, 0], [1, 1, 1, 1], [2, 2, 3, 5]),
    ], np.array([0, 0, 0, 0x81], np.uint8), None, None, None)
    want = [
        ([0, 1, 0, 0x81], [-1, -1, -1, -1], [-1, -1, -1, -1], {0: 3, 9 + 1: 2, 17: 1}),
        ([0x80, 0x82, 0, 0x81], [7, 0, -1, -1], [2, 2, -1, -1], {0: 1, 1 + 6: 1, 1 + 0: 1, 8: 1, 9 + 1: 2, 17: 1,
                                                                 13 + 3: 1, 13 + 1: 1, 13 + 2: 1, 18: 1}),
        ([0x80, 0x82, 0x80, 0x81], [7, 0, 3, -1], [2, 2, 3, -1], {0: 0, 1 + 6: 1, 1 + 0: 1, 1 + 3: 1, 8: 1, 9 + 1: 2, 17: 1,
                                                                  13 + 3: 1, 13 + 1: 1, 13 + 2: 1, 18: 1}),
    ]
    for (t, done, final, length, c), (wd, wf, wl, wc) in zip(T.eval_run(d, cr), want):
        assert done.tolist() == wd and final.tolist() == wf and length.tolist() == wl, t
        assert c == [wc.get(i, 0) for i in range(T.eval_counters(d))], t


def test_train_model_by_hand():
    """Four games of one tile, three steps (seats 0, 1, 0), 2 lives. Game 1's deal was not seen (0x80): its first ending counts as
    an episode and a score but in neither bomb-outs nor lengths, and it is tracked from the next deal on: its second ending, two
    moves later, counts in both. Counter row: [0] episodes, [1] score sum, [2] squared sum, [3..10) scores 0..6, [10] bomb-outs,
    [11] length sum, [12] tracked, [13 + 4 p + k] moves, [21 + p] misplays."""
    d = HAND
    cr = T.Crafted([
        # g0 misplays (life 1 of 2); g1 (unseen deal) plays, scores and ends at 4; g2 discards; g3 hints
        _step([3, 2, 0, 5], [0, 1, 0, 0], [0, 1, 0, 0], [0, 4, 0, 0]),
        # g0's second misplay (reward -2) ends it after 2 moves: a bomb-out, score 0; g1 hints; g2 ends at 6 after 4 + 2 moves with
        # a life left; g3's uid 11 is no move, but a step
        _step([2, 7, 2, 11], [-2, 0, 1, 0], [1, 0, 1, 0], [0, 0, 6, 0]),
        # g1 ends after 2 moves at score 9: counted as 6 everywhere; g3 ends after 10 + 3 moves at 2
        _step([1, 3, 4, 0], [0, 1, 0, 0], [0, 1, 0, 1], [0, 9, 0, 2]),
    ], None, np.array([0, 0x80, 1, 0], np.uint8), np.array([0, 0, 4, 10], np.int16), None)
    want = [
        ([1, 0, 1, 0], [1, 0, 5, 11], {0: 1, 1: 4, 2: 16, 3 + 4: 1, 13 + 0: 1, 13 + 1: 2, 13 + 2: 1, 21: 1}),
        ([0, 0, 0, 0], [0, 1, 0, 12], {0: 3, 1: 10, 2: 52, 3 + 4: 1, 3 + 0: 1, 3 + 6: 1, 10: 1, 11: 2 + 6, 12: 2,
                                       13 + 0: 1, 13 + 1: 2, 13 + 2: 1, 21: 1, 17 + 1: 2, 17 + 3: 1, 22: 1}),
        ([0, 0, 0, 0], [1, 0, 1, 0], {0: 5, 1: 18, 2: 92, 3 + 4: 1, 3 + 0: 1, 3 + 6: 2, 3 + 2: 1, 10: 1, 11: 8 + 2 + 13, 12: 4,
                                      13 + 0: 3, 13 + 1: 3, 13 + 2: 2, 21: 1, 17 + 1: 2, 17 + 3: 1, 22: 1}),
    ]
    for (t, lost, length, c), (wl, wn, wc) in zip(T.train_run(d, cr, np.array([0], np.int32), 1), want):
        assert lost.tolist() == wl and length.tolist() == wn, t
        assert c == [[wc.get(i, 0) for i in range(T.train_counters(d))]], t
    # a tile of nobody's (-1) or of a member that is not there (1 of 1): nothing is counted, nothing is written
    for owner in (-1, 1):
        *_, (t, lost, length, c) = T.train_run(d, cr, np.array([owner], np.int32), 1)
        assert lost.tolist() == cr.lost0.tolist() and length.tolist() == cr.length0.tolist() and not any(c[0])


def test_train_init_model_by_hand():
    d = T.dims_of(_cfg("Hanabi-Small", 3))          # deck 20, 3 hands of 2: 14 cards to draw; 3 tokens
    fresh = np.zeros(16, np.uint32)
    fresh[0] = 14 | 3 << 6 | 1 << 10 | 2 << 13      # (life and seat do not matter)
    rows = np.stack([fresh] * 6)
    rows[1, 0] = 13 | 3 << 6                        # a card drawn
    rows[2, 0] = 14 | 2 << 6                        # a token spent
    rows[3, 1] = 1 << 3                             # a firework
    rows[4, 9] = 1 << 4                             # a discard
    rows[5, 1] = 2 << 15                            # (hand sizes are not fireworks)
    lost, length = T.train_tally_init_model(d, rows)
    assert lost.tolist() == [0, 0x80, 0x80, 0x80, 0x80, 0] and not length.any()


# ---- a played game ----------------------------------------------------------------------------------------------------------------

def test_eval_model_on_a_played_oracle_game():
    """Hanabi-Small, 2 players, 48 games to the end under the open-handed driver (auto-reset off): the model fed with the oracle's
    outputs gives np.bincount of the final scores, the lengths, and the per-seat move counts of the recorded moves."""
    cfg, n = _cfg("Hanabi-Small", 2), 48
    d = T.dims_of(cfg)
    orc = O.OracleEnv(cfg, n, seed=D.SEED, first_game_id=D.FIRST_GAME_ID)
    rng = np.random.default_rng(D.SEED)
    out = orc.observe()
    done, final, length = np.zeros(n, np.uint8), np.full(n, -1, np.int8), np.full(n, -1, np.int16)
    c = [n] + [0] * (T.eval_counters(d) - 1)
    over, scores, lengths, moves = np.zeros(n, bool), np.zeros(n, np.int64), np.zeros(n, np.int64), []
    t = 0
    while not over.all():
        assert t < 200
        act = D.open_hand_moves(cfg, orc.export_state(), out["legal"], rng, D.P_RAND)
        out = orc.step(act)
        done, final, length, c = T.eval_tally_model(d, t % 2, t, act, out["reward"], out["terminal"], out["score"], done, final, length, c)
        ended = (out["terminal"] != 0) & ~over
        scores[ended], lengths[ended] = out["score"][ended], t + 1
        moves.append(np.where(over, -1, act))
        over |= ended
        t += 1
        assert c[0] == int((~over).sum())
    B = d.B
    assert scores.max() >= 5 and (scores > 0).sum() >= 24, "the driver no longer scores"
    assert c[1:1 + B] == np.bincount(scores, minlength=B).tolist() and c[0] == 0
    assert np.array_equal(final, scores) and np.array_equal(length, lengths) and (done & 0x80).all()
    moves = np.stack(moves)                         # [turn, game]; Small 2: uids 0-1 discard, 2-3 play, 4-5 colour, 6-10 rank
    for seat in range(2):
        m = moves[seat::2]
        want = [int(((m >= lo) & (m < hi)).sum()) for lo, hi in ((0, 2), (2, 4), (4, 6), (6, 11))]
        assert c[2 + B + 4 * seat:2 + B + 4 * seat + 4] == want and sum(want) > 0
    assert c[1 + B] == int((done & 0x7F >= cfg.max_life).sum()) and sum(c[2 + B + 8:]) == int((done & 0x7F).sum())


# ---- the generator's coverage ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _train_case(game, players, wrong=None):
    d = T.dims_of(_cfg(game, players))
    cr = T.crafted_steps(d, N_TRAIN, TURNS, seed=100 + players, p_end=0.3)
    log = collections.Counter()
    *_, last = T.train_run(d, cr, TILE_MEMBER, 3, wrong=wrong, log=log)
    return d, cr, last, log


@functools.lru_cache(maxsize=None)
def _eval_case(game, players, wrong=None):
    d = T.dims_of(_cfg(game, players))
    cr = T.crafted_steps(d, 300, TURNS, seed=200 + players)
    *_, last = T.eval_run(d, cr, wrong=wrong)
    return d, cr, last


def _distinct_scores_per_wave(cr, live0=None):
    """The largest number of distinct scores that games ending on one turn in one wave hold (live0: the games that count at all)."""
    best = 0
    live = np.ones(len(cr.steps[0]["terminal"]), bool) if live0 is None else live0.copy()
    for s in cr.steps:
        ended = (s["terminal"] != 0) & live
        for w in range(0, len(ended), 64):
            best = max(best, len(set(s["score"][w:w + 64][ended[w:w + 64]].tolist())))
        if live0 is not None:
            live &= ~ended
    return best


@pytest.mark.parametrize("game,players", T.VARIANTS)
def test_generator_coverage(game, players):
    d, cr, (_, lost, length, c), log = _train_case(game, players)
    B, P = d.B, d.P
    c = np.array(c, dtype=object)
    bomb, tracked, episodes = int(c[:, 3 + B].sum()), int(c[:, 5 + B].sum()), int(c[:, 0].sum())
    moves = c[:, 6 + B:6 + B + 4 * P]
    outside = N_TRAIN * TURNS - int(moves.sum())
    print(f"{game} {players}: episodes {episodes}, bomb-outs {bomb} ({log['end_exact']} on the misplay that took the last life), "
          f"lives left {tracked - bomb}, unarmed {episodes - tracked}, misplays that end nothing {log['misplay_live']}, uids outside "
          f"{outside}, smallest bin {int(c[:, 3:3 + B].min())}, smallest (seat, kind) {int(moves.sum(0).min())}, "
          f"scores in a wave {_distinct_scores_per_wave(cr)}, longest {log['longest']}")
    assert (c[:, 3:3 + B] > 0).all(), "a bin of a member is empty"
    assert bomb >= 10 and tracked - bomb >= 10 and episodes - tracked >= 10
    assert (bomb, tracked - bomb, episodes - tracked) == (log["end_bomb"], log["end_lives_left"], log["end_unarmed"])
    assert log["end_exact"] >= 10 and log["misplay_live"] >= 10
    assert outside >= 10 and outside == log["out_of_range"]
    assert (moves.sum(0) > 0).all() and (c[:, 6 + B + 4 * P:].sum(0) > 0).all()
    assert _distinct_scores_per_wave(cr) == B
    assert log["longest"] == 32767
    assert set(cr.lost0.tolist()) == {0, 1, 2, 0x80, 0x81} and cr.length0.max() <= 32766
    for s in cr.steps:
        assert s["score"].min() >= 0 and s["score"].max() <= B - 1
    acts = np.concatenate([s["actions"] for s in cr.steps])
    assert set(range(-2, d.A + 2)) == set(acts.tolist())
    # the same generator for the evaluation tally: 300 games, the last wave ragged, games finished beforehand with low bits
    d, cr, (_, done, final, length, ce) = _eval_case(game, players)
    fin0 = cr.done0 & 0x80 != 0
    assert fin0.sum() >= 10 and (cr.done0[fin0] & 0x7F != 0).any()
    assert all(x > 0 for x in ce[1:1 + B]) and ce[1 + B] >= 10 and sum(ce[1:1 + B]) - ce[1 + B] >= 10
    assert all(x > 0 for x in ce[2 + B:]), "a (seat, kind) or a seat's misplays never counted"
    assert ce[0] == int((done & 0x80 == 0).sum()) and (final[fin0] == -1).all() and (length[fin0] == -1).all()
    assert _distinct_scores_per_wave(cr, ~fin0) == B
    ragged = (cr.steps[0]["terminal"][256:] != 0) & ~fin0[256:]
    assert ragged.any(), "no game ends in the ragged last wave"


def test_wave_patterns_are_what_they_say():
    """On 300 games (waves 0..4): which lanes end, per pattern, in the eval model's own bookkeeping."""
    d, cr, _ = _eval_case("Hanabi-Full", 2)
    assert cr.schedule == {(0, 0): "all_misplay", (1, 0): "lane0", (2, 0): "lane63", (0, 1): "distinct", (3, 2): "same", (4, 2): "finished"}
    seen = {}
    prev = cr.done0
    for t, done, final, length, c in T.eval_run(d, cr):
        for (tt, w), what in cr.schedule.items():
            if tt == t:
                sl = slice(64 * w, 64 * w + 64)
                ended = (done[sl] & 0x80 != 0) & (prev[sl] & 0x80 == 0)
                seen[what] = (ended, final[sl].copy(), (done[sl] & 0x7F) - (prev[sl] & 0x7F), prev[sl] & 0x80 != 0)
        prev = done
    assert not seen["all_misplay"][0].any() and (seen["all_misplay"][2][~seen["all_misplay"][3]] == 1).all()
    assert np.flatnonzero(seen["lane0"][0]).tolist() == [0] and np.flatnonzero(seen["lane63"][0]).tolist() == [63]
    assert seen["distinct"][0].all() and seen["distinct"][1].tolist() == [l % d.B for l in range(64)]
    assert seen["same"][0].all() and len(set(seen["same"][1].tolist())) == 1
    assert seen["finished"][3].all()
    assert T.wave_schedule(64) == {(0, 0): "all_misplay", (1, 0): "lane0", (2, 0): "lane63", (3, 0): "distinct", (4, 0): "finished"}
    assert T.wave_schedule(128)[(0, 1)] == "distinct" and T.wave_schedule(128)[(3, 0)] == "same"


def test_generator_is_deterministic():
    d = T.dims_of(_cfg("Hanabi-Small", 3))
    a, b, other = T.crafted_steps(d, 130, 3, 5), T.crafted_steps(d, 130, 3, 5), T.crafted_steps(d, 130, 3, 6)
    for x, y in zip(a.steps, b.steps):
        assert all(np.array_equal(x[k], y[k]) and x[k].dtype == y[k].dtype for k in x)
    assert np.array_equal(a.done0, b.done0) and np.array_equal(a.lost0, b.lost0) and np.array_equal(a.length0, b.length0)
    assert not np.array_equal(a.steps[0]["actions"], other.steps[0]["actions"])


# ---- teeth ------------------------------------------------------------------------------------------------------------------------

def _shows(wrong, game, players):
    """Where a mistake can show at all: the hint boundary only where colours != ranks."""
    cfg = _cfg(game, players)
    return wrong != "rank_boundary_by_ranks" or cfg.colors != cfg.ranks


@pytest.mark.parametrize("wrong", T.WRONG)
def test_wrong_models_differ_on_the_crafted_steps(wrong):
    shown = 0
    for game, players in T.VARIANTS:
        right, bad = _train_case(game, players)[2][3], _train_case(game, players, wrong)[2][3]
        if _shows(wrong, game, players):
            assert right != bad, (wrong, game, players)
            shown += 1
        else:
            assert right == bad
        if wrong != "sq_is_sum":                    # (the evaluation tally keeps no squared sum)
            right, bad = _eval_case(game, players)[2][4], _eval_case(game, players, wrong)[2][4]
            assert (right != bad) == _shows(wrong, game, players), (wrong, game, players)
    assert shown >= 2


def test_random_play_cannot_tell_the_squared_sum_from_the_sum():
    """The gap: 300 uniform-random legal steps of Hanabi-Full, 2 players (the old kernel-level comparison's input; 256 games): every
    episode ends at score 0, so the model that adds b where it should add b * b gives the same counters. The models that count
    misplays wrongly do differ there: that part of the old test had teeth."""
    cfg = _cfg("Hanabi-Full", 2, D.FLAGS)
    d, n = T.dims_of(cfg), 256
    orc = O.OracleEnv(cfg, n, seed=2)
    legal = orc.observe()["legal"]
    steps = []
    for t in range(300):
        act = O.random_legal_actions(legal, 4, t + 1)
        out = orc.step(act)
        legal = out["legal"]
        steps.append(dict(actions=act, reward=out["reward"], terminal=out["terminal"], score=out["score"]))
    cr = T.Crafted(steps, None, np.zeros(n, np.uint8), np.zeros(n, np.int16), None)
    tm = np.array([0, 1], np.int32)
    run = lambda wrong: list(T.train_run(d, cr, tm, 2, wrong=wrong))[-1][3]
    right = run(None)
    episodes, top = sum(r[0] for r in right), max(b for r in right for b in range(d.B) if r[3 + b])
    print(f"episodes {episodes}, highest score {top}")
    assert episodes > 3000 and top == 0
    assert run("sq_is_sum") == right
    assert run("bomb_gt") != right and run("seat_stride_5") != right


# ---- PartnerStats -----------------------------------------------------------------------------------------------------------------

def test_partner_stats_equal_numpy():
    from hanabi_hip.partner_pool import PartnerStats

    d = T.dims_of(_cfg("Hanabi-Full", 2))
    rng = np.random.default_rng(9)
    scores = rng.integers(0, 26, 777).tolist() + [25] * 5
    lengths = rng.integers(20, 90, 500).tolist()                       # 500 of the 782 episodes were tracked from their deal
    s = PartnerStats(T.score_counter_row(d, scores, lengths, bombouts=120), 2, d.B)
    assert s.episodes == 782 and s.tracked == 500 and s.histogram.tolist() == np.bincount(scores, minlength=26).tolist()
    assert s.mean == pytest.approx(np.mean(scores), abs=1e-12)
    assert s.stderr == pytest.approx(np.std(scores, ddof=1) / np.sqrt(len(scores)), abs=1e-12)
    assert s.bombout_rate == 120 / 500 and s.mean_length == pytest.approx(np.mean(lengths), abs=1e-12)
    assert s.as_dict()["mean"] == s.mean and s.as_dict()["bombout_rate"] == s.bombout_rate
    # a row the model made: the same numbers as its own score list
    _, cr, (_, _, _, c), _ = _train_case("Hanabi-Full", 2)
    ended = [int(x) for st in cr.steps for x in st["score"][:128][st["terminal"][:128] != 0]]
    s = PartnerStats(c[0], 2, d.B)
    assert s.episodes == len(ended) and s.mean == pytest.approx(np.mean(ended), abs=1e-12)
    assert s.stderr == pytest.approx(np.std(ended, ddof=1) / np.sqrt(len(ended)), abs=1e-12)
    # no episode: NaN / NaN; one: stderr 0; every score the same: stderr 0, not the square root of a rounding error
    s = PartnerStats(T.score_counter_row(d, []), 2, d.B)
    assert math.isnan(s.mean) and math.isnan(s.stderr) and math.isnan(s.bombout_rate) and math.isnan(s.mean_length)
    s = PartnerStats(T.score_counter_row(d, [17], [60]), 2, d.B)
    assert s.mean == 17 and s.stderr == 0.0 and s.mean_length == 60 and s.bombout_rate == 0
    s = PartnerStats(T.score_counter_row(d, [3] * 7), 2, d.B)
    assert s.mean == 3 and s.stderr == 0.0 and math.isnan(s.mean_length)
