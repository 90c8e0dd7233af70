"""Greedy evaluation (hanabi_hip.evaluate, csrc/eval.hip), the parts that need no GPU: the turn bound against the CPU oracle,
EvalResult's statistics, argument checks, and the tally entry point's refusal to run without a device."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle_py as O

VARIANTS = [(g, p) for g in ("Hanabi-Full", "Hanabi-Small", "Hanabi-Very-Small") for p in (2, 3, 4, 5)]


def _longest_game(game, players, policy, n=256, seed=11):
    """Plays n oracle games (auto-reset off) to the end; returns the longest length."""
    cfg = O.make_config(game, players, 0)
    env = O.OracleEnv(cfg, n, seed=seed)
    hand = cfg.hand_size
    rng = np.random.default_rng(seed)
    legal = env.observe()["legal"]
    done = np.zeros(n, bool)
    length = np.zeros(n, np.int64)
    t = 0
    while not done.all():
        assert t < 1000, "a game did not end"
        if policy == "random":
            act = O.random_legal_actions(legal, seed, t + 1)
        else:
            # hint-heavy: a random legal hint whenever one is legal, else a discard, else a play (plays last: they end games)
            act = np.zeros(n, np.int32)
            for g in range(n):
                lg = np.flatnonzero(legal[g])
                if lg.size == 0:
                    continue
                for group in (lg[lg >= 2 * hand], lg[lg < hand], lg):
                    if group.size:
                        act[g] = rng.choice(group)
                        break
        out = env.step(act)
        ended = (out["terminal"] != 0) & ~done
        length[ended] = t + 1
        done |= ended
        legal = out["legal"]
        t += 1
    return int(length.max())


@pytest.mark.parametrize("game,players", VARIANTS)
def test_max_turns_bounds_every_oracle_game(game, players):
    import hanabi_hip
    from hanabi_hip.evaluate import max_turns

    bound = max_turns(hanabi_hip.make_config(game, players))
    longest = max(_longest_game(game, players, "hints"), _longest_game(game, players, "random"))
    assert longest <= bound, (longest, bound)
    if (game, players) == ("Hanabi-Full", 2):
        assert bound == 95


def test_eval_result_statistics_equal_numpy():
    from hanabi_hip import EvalResult

    rng = np.random.default_rng(3)
    scores = rng.integers(0, 26, 1001)
    scores[:7] = 25
    lengths = rng.integers(30, 96, 1001)
    r = EvalResult(scores, lengths, 25, bombouts=13)
    assert r.mean == pytest.approx(np.mean(scores), abs=1e-12)
    assert r.stderr == pytest.approx(np.std(scores, ddof=1) / np.sqrt(scores.size), abs=1e-12)
    assert r.perfect_rate == pytest.approx(np.mean(scores == 25), abs=1e-12)
    assert r.bombout_rate == pytest.approx(13 / 1001)
    assert r.histogram.tolist() == np.bincount(scores, minlength=26).tolist()
    d = r.as_dict()
    import json

    json.dumps(d)
    assert d["n_games"] == 1001 and d["max_length"] == int(lengths.max())
    one = EvalResult([4], [50], 25)
    assert one.stderr == 0.0 and one.mean == 4.0


def test_evaluator_argument_checks():
    from hanabi_hip import Evaluator

    with pytest.raises(ValueError):
        Evaluator(n_games=0)
    with pytest.raises(ValueError):
        Evaluator(n_games=-5)
    ev = Evaluator("Hanabi-Full", players=3, n_games=8)
    assert ev.max_turns > 0 and ev.env is None   # nothing touches the device before run()

    class Dummy:
        def eval_moves(self, *a, **k):
            raise AssertionError("must not be called")

        def requires_vectorized_observation(self):
            return True

    with pytest.raises(ValueError, match="one agent per seat"):
        ev.run([Dummy(), Dummy()])
    with pytest.raises(TypeError):
        ev.run([Dummy(), Dummy(), object()])


def test_eval_tally_arguments_and_counter_layout():
    import hanabi_hip

    L = hanabi_hip.lib()
    one = C.c_void_p(16)
    for game in ("Hanabi-Full", "Hanabi-Small"):
        for p in (2, 5):
            cfg = hanabi_hip.make_config(game, p)
            assert L.hb_eval_counters(C.byref(cfg)) == 2 + cfg.colors * cfg.ranks + 1 + 5 * p
    cfg = hanabi_hip.make_config()
    args = lambda n, seat, turn, ptr=one: (C.byref(cfg), n, seat, turn, ptr, one, one, one, one, one, one, one, None)
    assert L.hb_eval_tally(*args(4, 2, 0)) == -1 and b"seat" in L.hb_last_error()
    assert L.hb_eval_tally(*args(4, 0, -1)) == -1 and b"turn" in L.hb_last_error()
    assert L.hb_eval_tally(*args(4, 0, 40000)) == -1
    assert L.hb_eval_tally(*args(-1, 0, 0)) == -1
    assert L.hb_eval_tally(*args(4, 0, 0, None)) == -1 and b"null" in L.hb_last_error()
    assert L.hb_eval_tally(*args(0, 0, 0)) == 0       # empty: no-op
    bad = hanabi_hip.HbConfig(6, 5, 5, 5, 8, 3, 0)
    assert L.hb_eval_tally(C.byref(bad), 4, 0, 0, one, one, one, one, one, one, one, one, None) < 0


def test_eval_tally_without_device():
    import torch

    import hanabi_hip

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    cfg = hanabi_hip.make_config()
    one = C.c_void_p(16)
    assert hanabi_hip.lib().hb_eval_tally(C.byref(cfg), 4, 0, 0, one, one, one, one, one, one, one, one, None) == -2
