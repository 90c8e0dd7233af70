"""Off-belief learning levels 2+ without a GPU (hanabi_hip.obl, PartnerHistory.advance, hb_belief_history_step): the symbol is
declared, exported and bound; the entry point checks its arguments before any launch; `PartnerHistory.advance` on CPU tensors —
the reference the kernel is compared against in tests/test_obl_level_gpu.py — equals the method sequence (own_move, reset, push)
and the values worked out by hand; and its Python-side argument checks."""
import ctypes as C
import os

import numpy as np
import pytest

from test_search_depth_cpu import occupied_mask, own_move_ref

SW = 32   # state words, 2 players


def _hand(*cards):
    cards = list(cards) + [31] * (5 - len(cards))
    return sum(c << (5 * s) for s, c in enumerate(cards))


def _row(cp=0, status=0, mover=None, kind=0, idx=0, off=1, col=0, rank=0, hands=(_hand(1, 2, 3, 4, 5), _hand(6, 7, 8, 9, 10)), tag=0):
    """A state row with the words the history reads: word 0 current player and status, word 2 the last move,
    words 10 + seat the hands; `tag` marks word 5 so that rows can be told apart."""
    r = np.zeros(SW, np.int64)
    r[0] = (cp << 13) | (status << 19)
    if mover is not None:
        r[2] = 1 | (mover << 1) | (kind << 4) | (idx << 6) | (off << 9) | (col << 12) | (rank << 15)
    r[5] = tag
    r[10], r[11] = hands
    return r


def _rows(*rows):
    import torch

    return torch.as_tensor(np.stack(rows).astype(np.uint32).view(np.int32))


def _history(depth, m, alive, valid, moves=None):
    import torch

    import hanabi_hip
    from hanabi_hip import PartnerHistory

    h = PartnerHistory(hanabi_hip.make_config("Hanabi-Full", 2, 0), m, depth, "cpu")
    h.alive.copy_(torch.tensor(alive, dtype=torch.uint8))
    h.valid.copy_(torch.tensor(valid, dtype=torch.uint8))
    h.moves.copy_(torch.arange(depth * m, dtype=torch.int32).view(depth, m) + 100 if moves is None else torch.tensor(moves, dtype=torch.int32))
    h.prev_rows.copy_(torch.arange(depth * m * SW, dtype=torch.int32).view(depth, m, SW))
    h.draws, h.filled = list(range(50, 50 - 2 * depth, -2)), depth
    return h


def _clone(h):
    from hanabi_hip import PartnerHistory

    c = PartnerHistory(h.cfg, h.m, h.depth, "cpu")
    for name in ("prev_rows", "moves", "alive", "valid"):
        getattr(c, name).copy_(getattr(h, name))
    c.draws, c.filled = list(h.draws), h.filled
    return c


def _same(a, b):
    import torch

    return all(torch.equal(getattr(a, n), getattr(b, n)) for n in ("prev_rows", "moves", "alive", "valid")) and \
        (a.draws, a.filled) == (b.draws, b.filled)


# ---- declarations and argument validation ---------------------------------------------------------------------------------------------
def test_the_symbol_is_declared_exported_and_bound():
    import hanabi_hip
    from hanabi_hip import _capi, obl

    assert "hb_belief_history_step" in _capi.SIGNATURES and len(_capi.SIGNATURES["hb_belief_history_step"][1]) == 13
    L = hanabi_hip.lib()
    assert L.hb_belief_history_step and L.hb_abi_version() == 1
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "hanabi_hip.h")).read()
    assert "int hb_belief_history_step(const hb_config* cfg, int64_t m, int32_t depth, int32_t seat" in header
    assert hasattr(hanabi_hip.PartnerHistory, "advance") and callable(obl.frozen_copy)
    assert obl.OffBeliefSession.LEVEL_COUNTERS == ("conditioned_rows", "fallback_rows", "unconditioned_rows", "survivors", "depth_used_sum")


def test_argument_validation_needs_no_gpu():
    import hanabi_hip

    L = hanabi_hip.lib()
    cfg = hanabi_hip.make_config()
    ref, one = C.byref(cfg), C.c_void_p(16)
    err = lambda: L.hb_last_error()

    def step(m=4, depth=2, seat=0, own=one, reset=one, cur=one, prev=one, hist=(one,) * 4, cfg_ref=ref):
        return L.hb_belief_history_step(cfg_ref, m, depth, seat, own, reset, cur, prev, *hist, None)

    assert step(cfg_ref=None) < 0 and b"null" in err()
    assert step(cfg_ref=C.byref(hanabi_hip.HbConfig(6, 5, 5, 5, 8, 3, 0))) < 0 and b"players" in err()
    assert step(m=-1) < 0
    for depth in (0, 9, -1):
        assert step(depth=depth) < 0 and b"depth" in err()
    for seat in (-1, 2):
        assert step(seat=seat) < 0 and b"seat" in err()
    assert step(cur=None) < 0 and b"together" in err()
    assert step(prev=None) < 0 and b"together" in err()
    for bad in range(4):
        hist = [one] * 4
        hist[bad] = None
        assert step(hist=hist) < 0 and b"null" in err()
    assert step(m=1 << 24, depth=8) < 0 and b"2^31" in err()
    # no-ops: no game, or no part asked for (every optional pointer NULL)
    assert step(m=0) == 0 and step(m=0, depth=8, own=None, reset=None) == 0
    assert step(own=None, reset=None, cur=None, prev=None) == 0
    import torch

    if not torch.cuda.is_available():   # a real call without a device: refused, nothing computed on the CPU
        assert step() == -2


# ---- advance on CPU tensors: the method sequence and the hand-worked values -----------------------------------------------------------
def _by_methods(h, own, reset, cur, prev, seat, draw, valid):
    """The same turn with the methods a SearchPlayer uses, the push's valid flags given by the caller."""
    import torch

    from hanabi_hip import last_move_uid

    if own is not None:
        h.own_move(own)
    if reset is not None:
        for g in np.flatnonzero(np.asarray(reset)):
            h.valid[:, g] = 0
            h.alive[:, g] = 0
    if cur is not None:
        h.push(prev, last_move_uid(h.cfg, cur), draw, torch.tensor(valid), seat=seat)


def test_a_play_of_a_slot_alive_in_some_entries_and_gone_in_others_and_a_hint():
    import torch

    H = 5
    alive = [[0b11111, 0b11111, 0b11111], [0b10111, 0b10111, 0b01010], [0b00001, 0b00001, 0b00000]]
    valid = [[1, 1, 1], [1, 0, 1], [1, 1, 0]]
    # game 0: plays slot 3; game 1: hints (uid 2H + 1); game 2: discards slot 1 (uid H + 1)
    own = torch.tensor([3, 2 * H + 1, H + 1], dtype=torch.int32)
    h = _history(3, 3, alive, valid)
    want = _clone(h)
    h.advance(own_moves=own)
    _by_methods(want, own, None, None, None, None, None, None)
    assert _same(h, want)
    # by hand: the 4th set bit leaves entries 0 (bit 3) and 1 (bit 4) of game 0, entry 2 holds one card only; a hint changes
    # nothing, whatever the valid flag; the 2nd set bit leaves entry 0 (bit 1) and entry 1 (bit 3) of game 2
    assert h.alive.tolist() == [[0b10111, 0b11111, 0b11101], [0b00111, 0b10111, 0b00010], [0b00001, 0b00001, 0b00000]]
    for d in range(3):
        for g in range(3):
            assert int(h.alive[d, g]) == own_move_ref(alive[d][g], int(own[g]), H)
    assert h.valid.tolist() == valid and (h.draws, h.filled) == ([50, 48, 46], 3)   # nothing else moved


def test_reset_then_push_cut_chain_and_a_full_turn():
    """Four games, observer seat 1, depth 3, one call with all three parts.
    game 0: the ordinary turn — I played slot 0 two plies ago, the partner (seat 0) answered with a rank hint;
    game 1: reset, and the new deal has no move yet (word 2 = 0): every entry invalid, the new one too;
    game 2: the chain is cut — prev is a finished game; the older entries stay valid behind the invalid new one;
    game 3: the last mover recorded is me (seat 1): invalid too."""
    import torch

    mine = _hand(11, 12, 13, 14)     # four cards: slot 4 empty
    prev = _rows(_row(cp=0, tag=70, hands=(_hand(1, 2, 3, 4, 5), mine)), _row(cp=0, tag=71), _row(cp=0, status=1, tag=72),
                 _row(cp=1, tag=73))
    cur = _rows(_row(cp=1, mover=0, kind=3, off=1, rank=4), _row(cp=0), _row(cp=1, mover=0, kind=1, idx=2),
                _row(cp=0, mover=1, kind=0, idx=4))
    alive = [[0b11111] * 4, [0b01111] * 4, [0b00011] * 4]
    valid = [[1] * 4, [1] * 4, [1] * 4]
    own = torch.tensor([0, 0, 25, -1], dtype=torch.int32)   # (25: not a move of this game; -1: none)
    reset = torch.tensor([0, 1, 0, 0], dtype=torch.int8)
    h = _history(3, 4, alive, valid)
    before = _clone(h)
    want = _clone(h)
    h.advance(own_moves=own, reset=reset, cur_rows=cur, prev_rows=prev, seat=1, draw=52)
    _by_methods(want, own, reset, cur, prev, 1, 52, [1, 0, 0, 0])
    assert _same(h, want)
    # rows and moves: shifted by one whatever happened to the flags, the oldest dropped
    assert torch.equal(h.prev_rows[0], prev) and torch.equal(h.prev_rows[1:], before.prev_rows[:2])
    assert torch.equal(h.moves[1:], before.moves[:2])
    # rank hint to the next seat: 2H + (P - 1) C + 0 * R + 4 = 19; no move yet: -1; play of slot 2: 2; discard of slot 4: H + 4
    assert h.moves[0].tolist() == [19, -1, 2, 9]
    assert h.valid.tolist() == [[1, 0, 0, 0], [1, 0, 1, 1], [1, 0, 1, 1]]
    occ = [occupied_mask(int(prev[g, 11]) & 0xFFFFFFFF) for g in range(4)]
    assert occ == [0b01111, 0b11111, 0b11111, 0b11111]
    # the own move came first (slot 0 left the old entries of games 0 and 1), then game 1 was reset, then the push
    assert h.alive.tolist() == [occ, [0b11110, 0, 0b11111, 0b11111], [0b01110, 0, 0b01111, 0b01111]]
    assert (h.draws, h.filled) == ([52, 50, 48], 3)


def test_depth_1_and_parts_alone():
    import torch

    prev, cur = _rows(_row(cp=1, tag=9)), _rows(_row(cp=0, mover=1, kind=2, off=1, col=3))
    h = _history(1, 1, [[0b00111]], [[1]])
    h.advance(reset=torch.tensor([True]))
    assert h.alive.tolist() == [[0]] and h.valid.tolist() == [[0]] and h.moves.tolist() == [[100]] and h.filled == 1
    h.advance(cur_rows=cur, prev_rows=prev, seat=0, draw=7)
    want = _history(1, 1, [[0]], [[0]])
    _by_methods(want, None, None, cur, prev, 0, 7, [1])
    assert _same(h, want)
    assert h.moves.tolist() == [[2 * 5 + 3]] and h.valid.tolist() == [[1]] and h.alive.tolist() == [[0b11111]] and h.draws == [7]
    assert torch.equal(h.prev_rows[0], prev)
    h.advance()   # nothing asked for: nothing happens
    assert _same(h, want)


def test_filled_and_draws_move_as_in_push():
    prev, cur = _rows(_row(cp=1)), _rows(_row(cp=0, mover=1, kind=1, idx=0))
    from hanabi_hip import PartnerHistory, make_config

    h = PartnerHistory(make_config("Hanabi-Full", 2, 0), 1, 3, "cpu")
    for k, draw in enumerate((3, 5, 7, 9)):
        h.advance(cur_rows=cur, prev_rows=prev, seat=0, draw=draw)
        assert h.filled == min(k + 1, 3)
    assert h.draws == [9, 7, 5] and h.valid.tolist() == [[1]] * 3


def test_python_arguments_are_checked():
    import torch

    h = _history(2, 4, [[0] * 4] * 2, [[0] * 4] * 2)
    rows = torch.zeros((4, SW), dtype=torch.int32)
    with pytest.raises(ValueError, match="together"):
        h.advance(cur_rows=rows, seat=0, draw=1)
    with pytest.raises(ValueError, match="together"):
        h.advance(prev_rows=rows, seat=0, draw=1)
    with pytest.raises(ValueError, match="seat and the draw"):
        h.advance(cur_rows=rows, prev_rows=rows, draw=1)
    with pytest.raises(ValueError, match="seat and the draw"):
        h.advance(cur_rows=rows, prev_rows=rows, seat=0)
    for seat in (-1, 2):
        with pytest.raises(ValueError, match="out of range"):
            h.advance(cur_rows=rows, prev_rows=rows, seat=seat, draw=1)
    with pytest.raises(ValueError, match="cur_rows has shape"):
        h.advance(cur_rows=rows[:3], prev_rows=rows, seat=0, draw=1)
    with pytest.raises(ValueError, match="prev_rows has shape"):
        h.advance(cur_rows=rows, prev_rows=rows[:, :31], seat=0, draw=1)
    with pytest.raises(ValueError, match="own_moves has shape"):
        h.advance(own_moves=[0] * 3)
    with pytest.raises(ValueError, match="reset has shape"):
        h.advance(reset=[0] * 5)
    before = _clone(h)
    h.advance(own_moves=[0] * 4, reset=[0] * 4)   # lists are taken, as own_move() takes them
    assert _same(h, before)
