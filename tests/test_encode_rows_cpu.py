"""hb_encode_rows and its numpy reference, without a GPU ("The stateless encoder").

* the entry point is declared in the header, exported by the library, bound in the ctypes table and exported by the package;
* every argument check of hb_encode_rows answers by return code before any device call;
* `encode_rows_ref` equals the C oracle's observation and legal mask at every state of the deep-play corpus (tests/deep_play.py),
  all twelve variants, every game, every step;
* an explicit observer: the observation is the one of the same row with the seat field rewritten, the legal mask is zero exactly
  where the observer is not to act, and one 3-player row is worked out by hand.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import deep_play as D
import encode_rows_util as U
import hanabi_hip
from oracle import oracle_py as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_declared_exported_bound():
    text = open(os.path.join(ROOT, "include", "hanabi_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+hb_encode_rows\s*\(\s*const\s+hb_config\s*\*", text), "hb_encode_rows is not declared in the header"
    from hanabi_hip import _capi

    assert "hb_encode_rows" in _capi.SIGNATURES
    L = hanabi_hip.lib()
    assert hasattr(L, "hb_encode_rows") and L.hb_encode_rows.argtypes is not None and len(L.hb_encode_rows.argtypes) == 8
    assert L.hb_abi_version() == 1
    assert callable(hanabi_hip.encode_rows) and callable(hanabi_hip.encode_rows_ref)
    assert "encode_rows" in hanabi_hip.__all__ and "encode_rows_ref" in hanabi_hip.__all__
    assert "encode_rows.hip" in open(os.path.join(ROOT, "hanabi-agents_amd", "csrc", "Makefile")).read()


def test_argument_validation_needs_no_gpu():
    L = hanabi_hip.lib()
    cfg = hanabi_hip.make_config("Hanabi-Full", 3)
    c = C.byref(cfg)
    one, odd = C.c_void_p(4096), C.c_void_p(4096 + 8)    # fake pointers: every call below must be refused before they are used
    INVALID, ALIGN = -1, -4
    assert L.hb_encode_rows(None, one, 4, -1, one, None, one, None) == INVALID and b"config" in L.hb_last_error()
    assert L.hb_encode_rows(c, None, 4, -1, one, None, one, None) == INVALID and b"rows_dev" in L.hb_last_error()
    assert L.hb_encode_rows(c, one, -1, -1, one, None, one, None) == INVALID
    # a valid configuration nobody compiled a kernel for (6 information tokens), and one out of range
    other = hanabi_hip.HbConfig(2, 5, 5, 5, 6, 3, 0)
    assert L.hb_config_validate(C.byref(other)) == 0
    assert L.hb_encode_rows(C.byref(other), one, 4, -1, one, None, one, None) == INVALID and b"no compiled kernel" in L.hb_last_error()
    bad = hanabi_hip.HbConfig(6, 5, 5, 5, 8, 3, 0)
    assert L.hb_encode_rows(C.byref(bad), one, 4, -1, one, None, one, None) == INVALID and b"players" in L.hb_last_error()
    for seat in (-2, 3, 7):
        assert L.hb_encode_rows(c, one, 4, seat, one, None, one, None) == INVALID and b"seat" in L.hb_last_error()
    assert L.hb_encode_rows(c, one, 4, -1, None, None, one, None) == INVALID and b"obs" in L.hb_last_error()
    assert L.hb_encode_rows(c, one, 4, -1, odd, None, one, None) == ALIGN
    assert L.hb_encode_rows(c, one, 4, -1, one, odd, one, None) == ALIGN
    assert L.hb_encode_rows(c, one, 4, -1, None, odd, one, None) == ALIGN
    assert L.hb_encode_rows(c, one, 4, -1, one, None, odd, None) == ALIGN
    assert L.hb_encode_rows(c, odd, 4, -1, one, None, one, None) == ALIGN and b"rows_dev" in L.hb_last_error()
    # nothing to do: OK, whatever the machine
    for seat in (-1, 0, 2):
        assert L.hb_encode_rows(c, one, 0, seat, one, None, one, None) == 0
        assert L.hb_encode_rows(c, one, 0, seat, None, one, None, None) == 0


def test_no_cpu_fallback():
    import torch

    if torch.cuda.is_available():
        return      # (the GPU tests cover the machine with a device)
    L = hanabi_hip.lib()
    cfg = hanabi_hip.make_config()
    one = C.c_void_p(4096)
    assert L.hb_encode_rows(C.byref(cfg), one, 4, -1, one, None, one, None) == -2      # HB_ERR_NO_DEVICE: nothing is computed
    with pytest.raises(hanabi_hip.HbError):
        hanabi_hip.encode_rows(cfg, torch.zeros((4, 32), dtype=torch.int32))


def test_python_argument_checks():
    cfg = hanabi_hip.make_config()
    rows = np.zeros((2, 32), np.uint32)
    for seat in (-2, 2, 5):
        with pytest.raises(ValueError):
            hanabi_hip.encode_rows_ref(cfg, rows, seat=seat)
        with pytest.raises(ValueError):
            hanabi_hip.encode_rows(cfg, None, seat=seat)


@pytest.mark.parametrize("game,players", D.VARIANTS)
def test_ref_equals_the_oracle_on_deep_play(game, players):
    cfg = hanabi_hip.make_config(game, players, D.FLAGS)
    tally = D.Tally(O.make_config(game, players, D.FLAGS))
    seen = 0
    for t, rows, out in U.deep_run(game, players, tally):
        obs, legal = hanabi_hip.encode_rows_ref(cfg, rows)
        assert obs.dtype == np.int8 and legal.dtype == np.int8 and obs.shape == out["obs"].shape
        bad = np.flatnonzero((obs != out["obs"]).any(1) | (legal != out["legal"]).any(1))
        assert bad.size == 0, f"step {t}: games {bad[:8]} differ from the oracle"
        seen += 1
    assert seen == U.steps(game, players) + 1
    print(game, players, tally.as_dict())
    # the states an encoder goes wrong at were there
    assert tally.deck0_states > 0 and tally.info0_states > 0 and tally.short_hand_states > 0
    if (game, players) == ("Hanabi-Full", 2):
        assert tally.episodes > 0


@pytest.mark.parametrize("players", [3, 5])
def test_explicit_observer_is_the_row_with_the_seat_rewritten(players):
    cfg = hanabi_hip.make_config("Hanabi-Full", players, D.FLAGS)
    snaps = U.deep_rows("Hanabi-Full", players)
    rows = np.concatenate([snaps[k] for k in U.SNAPSHOTS])
    cur = (rows[:, 0] >> 13) & 7
    own_obs, own_legal = hanabi_hip.encode_rows_ref(cfg, rows)
    assert own_legal.any(1).all()
    for o in range(players):
        obs, legal = hanabi_hip.encode_rows_ref(cfg, rows, seat=o)
        want, _ = hanabi_hip.encode_rows_ref(cfg, U.with_seat(rows, o))
        assert np.array_equal(obs, want)
        mine = cur == o
        assert mine.any() and (~mine).any()
        assert not legal[~mine].any()
        assert np.array_equal(legal[mine], own_legal[mine]) and np.array_equal(obs[mine], own_obs[mine])


def _ones(v):
    return [int(i) for i in np.flatnonzero(v)]


def test_hand_worked_three_player_rank_hint():
    """Full, 3 players (25 identities, hands of 5, 32-word rows). Seat 0 holds R1 R2 R3 R4 R5 (cards 0-4), seat 1 Y1-Y5 (5-9),
    seat 2 G1 G1 G2 B3 W5 (10 10 11 17 24). Two hints were given (6 tokens left); the second, by seat 1, told seat 2 (one seat on:
    target offset 1) its rank-1 cards, slots 0 and 1. Seat 2 is to act.
    Layout: hands [0, 250) | short-hand flags [250, 253) | deck [253, 288) | fireworks [288, 313) | tokens [313, 321) |
    lives [321, 324) | discards [324, 374) | last move: actor [374, 377) type [377, 381) target [381, 384) colour [384, 389)
    rank [389, 394) touched [394, 399) position [399, 404) card [404, 429) scored 429 token 430 | knowledge 431 + 35 * slot."""
    cfg = hanabi_hip.make_config("Hanabi-Full", 3)
    hands = [[0, 1, 2, 3, 4], [5, 6, 7, 8, 9], [10, 10, 11, 17, 24]]
    row = np.zeros((1, 32), np.uint32)
    row[0, 0] = 35 | (6 << 6) | (3 << 10) | (2 << 13) | (3 << 16) | (2 << 21)
    row[0, 1] = (5 << 15) | (5 << 18) | (5 << 21)
    row[0, 2] = 1 | (1 << 1) | (3 << 4) | (1 << 9) | (0 << 15) | (0b00011 << 20)      # seat 1, reveal rank, offset 1, rank 1
    everything = 31 | (31 << 5)
    told = 31 | (1 << 5) | (1 << 11)              # any colour, rank 1, rank revealed
    not_one = 31 | (0b11110 << 5)                 # any colour, not rank 1
    know = [[everything] * 5, [everything] * 5, [told, told, not_one, not_one, not_one]]
    for p in range(3):
        row[0, 10 + p] = sum(c << (5 * i) for i, c in enumerate(hands[p])) | (31 << 25)
        k = sum(v << (12 * i) for i, v in enumerate(know[p]))
        row[0, 13 + 2 * p], row[0, 14 + 2 * p] = k & 0xFFFFFFFF, k >> 32
    all_25, ranks_2_to_5 = list(range(25)), [c * 5 + r for c in range(5) for r in range(1, 5)]
    # observer -> (last-move actor offset, target offset, the two other hands in the order it sees them)
    expect = {0: (1, 2, (1, 2)), 1: (0, 1, (2, 0)), 2: (2, 0, (0, 1))}
    for o, (actor, target, others) in expect.items():
        obs, legal = hanabi_hip.encode_rows_ref(cfg, row, seat=o)
        v = obs[0]
        assert v.shape == (956,)
        for j, p in enumerate(others):
            for i in range(5):
                assert _ones(v[(5 * j + i) * 25:(5 * j + i + 1) * 25]) == [hands[p][i]], (o, p, i)
        assert _ones(v[250:253]) == []
        assert _ones(v[253:288]) == list(range(35)) and _ones(v[288:313]) == []
        assert _ones(v[313:321]) == list(range(6)) and _ones(v[321:324]) == [0, 1, 2] and _ones(v[324:374]) == []
        assert _ones(v[374:431]) == [actor, 3 + 3, 7 + target, 15 + 0, 20 + 0, 20 + 1], o
        for rel in range(3):
            p = (o + rel) % 3
            for i in range(5):
                slot = v[431 + 35 * (5 * rel + i):431 + 35 * (5 * rel + i + 1)]
                if p != 2:
                    assert _ones(slot) == all_25, (o, p, i)
                elif i < 2:
                    assert _ones(slot) == [0, 5, 10, 15, 20, 30], (o, p, i)      # a rank-1 card of any colour; rank 1 revealed
                else:
                    assert _ones(slot) == ranks_2_to_5, (o, p, i)
        if o == 2:
            # discards 0-4 (6 < 8 tokens), plays 5-9; the next seat (0) holds red only, ranks 1-5; the one after (1) yellow, ranks 1-5
            assert _ones(legal[0]) == list(range(10)) + [10 + 0, 10 + 5 + 1] + list(range(20, 25)) + list(range(25, 30))
        else:
            assert not legal.any()
    # seat=None is the seat to act
    assert all(np.array_equal(a, b) for a, b in zip(hanabi_hip.encode_rows_ref(cfg, row), hanabi_hip.encode_rows_ref(cfg, row, seat=2)))
