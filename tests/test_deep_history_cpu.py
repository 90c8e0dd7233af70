"""The partner history and the splice on deep play of all twelve variants, the parts that need no GPU: the
corpus of tests/deep_history.py held to floors, `PartnerHistory("cpu").advance` against the identity model after every call, the
true current rows spliced back into every stored state under the tracked mask, and teeth: a plain restatement of
include/hanabi_hip.h's text for hb_belief_history_step agrees with the model, and each of five wrong versions of it (or of the
splice's walk) differs from the model in every variant where that mistake can show, and in no other.
tests/test_deep_history_gpu.py holds the kernels to the same model."""
import numpy as np
import pytest

import deep_history as DH
from test_search_depth_cpu import splice_alive_ref

# what deep_history.counts measured (games of seed 9, default_rng(4), 20 % random moves), in VARIANTS' order; the floors below
# are half of these, rounded down. With two players no hint goes past the next seat and no running game shows the seat that
# observes a short hand: those three are 0 by the rules.
MEASURED = dict(
    rank=(77, 122, 156, 166, 21, 44, 51, 60, 16, 25, 22, 17),
    rank_far=(0, 49, 91, 117, 0, 20, 25, 40, 0, 13, 13, 12),
    colour_far=(0, 69, 107, 130, 0, 15, 31, 39, 0, 6, 4, 3),
    short_observer=(0, 8, 56, 164, 0, 5, 32, 130, 0, 25, 78, 136),
    deck0=(9, 36, 84, 170, 6, 18, 61, 140, 16, 72, 134, 192),
    dead=(25678, 35007, 45954, 48141, 7400, 10469, 13266, 15771, 5124, 5605, 4822, 2749),
    short_stored=(0, 96, 577, 1640, 0, 60, 331, 1300, 0, 300, 805, 1360),
    finished_push=(48,) * 12)
BY_TWO = ("rank_far", "colour_far", "short_observer", "short_stored")


@pytest.mark.parametrize("game,players", DH.VARIANTS)
def test_the_corpus_reaches_what_the_tests_need(game, players):
    got = DH.counts(game, players)
    print(game, players, got)
    k = DH.VARIANTS.index((game, players))
    for name, measured in MEASURED.items():
        if players == 2 and name in BY_TWO:
            assert got[name] == 0, name
        else:
            assert measured[k] >= 2 and got[name] >= measured[k] // 2, (name, got[name], measured[k])
    assert got["finished_push"] == 48   # every game ends within STEPS plies, on a ply some observer is pushed
    plies = DH.splice_plies(game, players)
    assert 2 <= len(plies) <= 3 and plies[-1] < DH.play(game, players).moves.shape[0]


def _i32(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy())


@pytest.mark.parametrize("game,players", DH.VARIANTS)
def test_advance_on_the_cpu_equals_the_identity_model(game, players):
    """Every observer seat, depth 1 and 8, a history that starts from zeros; all four tensors after every call."""
    import torch

    import hanabi_hip
    from hanabi_hip import PartnerHistory

    cfg = hanabi_hip.make_config(game, players)
    for depth in DH.DEPTHS:
        for seat in range(players):
            model = DH.Model(game, players, seat, depth)
            h = PartnerHistory(cfg, 48, depth, "cpu")
            for call in model.calls():
                if call["own"] is not None:
                    h.advance(own_moves=torch.from_numpy(call["own"]))
                else:
                    h.advance(cur_rows=_i32(call["cur"]), prev_rows=_i32(call["prev"]), seat=seat, draw=call["t"])
                where = (game, players, depth, seat, call["t"])
                assert np.array_equal(h.prev_rows.numpy().view(np.uint32), model.rows), where
                assert np.array_equal(h.moves.numpy(), model.moves), where
                assert np.array_equal(h.alive.numpy(), model.alive), where
                assert np.array_equal(h.valid.numpy(), model.valid), where


# ---- the splice -------------------------------------------------------------------------------------------------------------------
def _junk(hand, alive, t):
    """The hand word with every occupied alive slot overwritten by another card id."""
    hand = int(hand)
    for s in range(5):
        c = (hand >> (5 * s)) & 31
        if (alive >> s) & 1 and c != 31:
            hand = (hand & ~(31 << (5 * s))) | (((c + 1 + (7 * s + t) % 29) % 30) << (5 * s))
    return hand


def _splice_by_size(prev_hand, alive, cand_hand, n_now):
    """WRONG on purpose: the splice's walk with a slot taken as occupied when it lies below the hand size of the CURRENT row."""
    out, j = int(prev_hand), 0
    for s in range(5):
        if s >= n_now:
            continue
        c = (int(cand_hand) >> (5 * j)) & 31 if j < 5 else 31
        if (alive >> s) & 1 and c != 31:
            out = (out & ~(31 << (5 * s))) | (c << (5 * s))
            j += 1
    return out


@pytest.mark.parametrize("game,players", DH.VARIANTS)
def test_the_true_rows_spliced_back_give_every_stored_state(game, players):
    """Every observer, depth 8, after every call, every stored entry of every game that was running before the ply (an entry of a
    game that is over no longer changes): the true current row spliced into the stored row under the model's mask (the
    restatement of tests/test_search_depth_cpu.py, K = 1) is the stored row word for word, and still is after the alive slots of
    the stored hand were overwritten with other card ids. The walk that reads occupancy from the current row's hand size instead
    of the stored hand's fields gives another hand exactly where the model says it must: a stored slot at or above the current
    hand size that is alive (it keeps the overwritten card) — in every variant, two players included (the observer's own last
    move leaves it a short hand next to stored full ones)."""
    checked = wrong = must = 0
    for seat in range(players):
        model = DH.Model(game, players, seat, 8)
        w = 10 + seat
        for call in model.calls():
            t = call["t"]
            live = np.flatnonzero(DH.running(model.play.rows[t]))
            now = model.now[live]
            n_now = DH.hand_n(now, seat)
            for d in range(min(8, t + 1)):
                stored, alive = model.rows[d][live], model.alive[d][live]
                if not stored.any():
                    continue
                assert np.array_equal(splice_alive_ref(stored, alive, now, seat, 1), stored), (seat, t, d)
                junk = stored.copy()
                junk[:, w] = [_junk(hw, int(a), t) for hw, a in zip(stored[:, w], alive)]
                assert np.array_equal(splice_alive_ref(junk, alive, now, seat, 1), stored), (seat, t, d, "junk")
                checked += len(live)
                for i in range(len(live)):
                    bad = _splice_by_size(junk[i, w], int(alive[i]), now[i, w], int(n_now[i])) != int(stored[i, w])
                    need = (int(alive[i]) >> int(n_now[i])) != 0
                    assert bad == need, (seat, t, d, i)
                    wrong, must = wrong + bad, must + need
    print(game, players, "entries checked", checked, "the walk by the current hand size differs in", wrong)
    assert checked > 1000 and wrong == must > 0


# ---- teeth: the header's text in plain Python, and wrong versions of it ---------------------------------------------------------------
def decode(cfg, w2, mutant=None):
    """The move recorded in word 2, by include/hanabi_hip.h's text for hb_belief_history_step."""
    H, P, C, R = cfg.hand_size, cfg.players, cfg.colors, cfg.ranks
    w2 = int(w2)
    if not w2 & 1:
        return -1
    kind, idx, off, col, rank = (w2 >> 4) & 3, (w2 >> 6) & 7, ((w2 >> 9) & 7) - 1, (w2 >> 12) & 7, (w2 >> 15) & 7
    if kind == 1:
        return idx
    if kind == 0:
        return H + idx
    if kind == 2:
        return 2 * H + off * C + col
    base = (P - 1) * (R if mutant == "rank_base_ranks" else C)
    return 2 * H + base + off * (C if mutant == "offset_times_colors" else R) + rank


def own_kill(alive, uid, H, mutant=None):
    if not 0 <= uid < 2 * H:
        return alive
    s = uid % (5 if mutant == "slot_mod_5" else H)
    if mutant == "bit_s":
        return alive & ~(1 << s)
    seen = 0
    for b in range(5):
        if (alive >> b) & 1:
            if seen == s:
                return alive & ~(1 << b)
            seen += 1
    return alive


def differs(game, players, seat, depth, mutant):
    """(calls after which the restated rule's moves differ from the model's, calls after which its alive masks do)."""
    model = DH.Model(game, players, seat, depth)
    cfg, N = model.cfg, 48
    alive, moves = np.zeros((depth, N), np.uint8), np.zeros((depth, N), np.int32)
    bad_moves = bad_alive = 0
    for call in model.calls():
        if call["own"] is not None:
            for g in range(N):
                for d in range(depth):
                    alive[d, g] = own_kill(int(alive[d, g]), int(call["own"][g]), cfg.hand_size, mutant)
        else:
            alive[1:], moves[1:] = alive[:-1].copy(), moves[:-1].copy()
            for g in range(N):
                hand = int(call["prev"][g, 10 + seat])
                alive[0, g] = sum(1 << s for s in range(5) if (hand >> (5 * s)) & 31 != 31)
                moves[0, g] = decode(cfg, call["cur"][g, 2], mutant)
        bad_moves += not np.array_equal(moves, model.moves)
        bad_alive += not np.array_equal(alive, model.alive)
    return bad_moves, bad_alive


@pytest.mark.parametrize("game,players", DH.VARIANTS)
def test_each_wrong_rule_differs_from_the_model_where_it_can(game, players):
    """The header's rule, restated, agrees with the model at every call. Then, one at a time:
      * the offset multiplied by `colors` in the rank-hint branch: shows exactly where colors != ranks and a hint can go past the
        next seat, Small and Very-Small with 3 players or more; elsewhere the two formulas are the same number for every word 2
        the game can write (colors == ranks, or offset - 1 == 0), and the run shows no difference;
      * (P - 1) * ranks as the rank hints' base: shows where colors != ranks, at the first rank hint;
      * uid % 5 for the slot of a play or discard: shows where the hand size is not 5 (a play of slot s is uid H + s);
      * the own move clears bit s instead of the s-th set bit: shows at depth 8 (an older entry has a dead slot below) in every
        variant but Very-Small with 5 players, whose ten cards are all dealt: the last round is the first, nobody moves twice, no
        mask loses a second bit; at depth 1 the one entry is never older than the observer's last move, and the two are the
        same."""
    cfg = DH.config(game, players)
    seats = range(players)
    for depth in DH.DEPTHS:
        assert all(differs(game, players, seat, depth, None) == (0, 0) for seat in seats), depth
    C, R, H, P = cfg.colors, cfg.ranks, cfg.hand_size, cfg.players
    far = sum(differs(game, players, seat, 1, "offset_times_colors")[0] for seat in seats)
    base = sum(differs(game, players, seat, 1, "rank_base_ranks")[0] for seat in seats)
    mod5 = sum(differs(game, players, seat, 8, "slot_mod_5")[1] for seat in seats)
    bit8 = sum(differs(game, players, seat, 8, "bit_s")[1] for seat in seats)
    bit1 = sum(differs(game, players, seat, 1, "bit_s")[1] for seat in seats)
    print(game, players, "calls that differ:", dict(offset_times_colors=far, rank_base_ranks=base, slot_mod_5=mod5, bit_s=bit8))
    assert (far > 0) == (C != R and P >= 3)
    if C == R or P == 2:   # it cannot show: the same number for every offset the game has
        for off in range(1, P):
            w2 = 1 | (3 << 4) | (off << 9) | (2 << 15)
            assert C == R or off == 1
            assert decode(cfg, w2, "offset_times_colors") == decode(cfg, w2)
    assert (base > 0) == (C != R)
    assert (mod5 > 0) == (H != 5)
    once = not DH.running(DH.play(game, players).rows[P]).any()   # every game is over after one round of the table
    assert once == ((game, players) == ("Hanabi-Very-Small", 5))
    assert (bit8 > 0) == (not once) and bit1 == 0
