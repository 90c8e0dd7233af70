"""hb_belief_carry and the tracked belief, the parts that need no GPU: hand-worked cases of the numpy restatement
`belief_carry_ref` (one per branch of the rule in include/hanabi_hip.h), its exactness against the enumerated posterior on scripted
Hanabi-Small transitions (and the failure of the variant without the draw weight g), its invariants on random play, the argument
validation of the wrapper and of SearchPlayer(track=...), and the exported symbol. tests/test_belief_carry_gpu.py holds the kernel
to this restatement byte for byte."""
import math
import os

import numpy as np
import pytest
import torch
from test_search_cpu import _oracle, determinize_row, enumerate_hands, hand_types

M32 = 0xFFFFFFFF


# ---- hand-made rows: only what the rule reads ------------------------------------------------------------------------------------
# Hanabi-Small, 2 players: 2 colours x 5 ranks (card id = colour * 5 + rank), hands of 2, a deck of 20. The observer is seat 0.
ALL = 0x3E3   # a slot that was told nothing: both colours, all five ranks


def small_cfg():
    return _oracle().make_config("Hanabi-Small", 2, 0)


def state_words(cfg):
    import ctypes as C

    import hanabi_hip

    return hanabi_hip.lib().hb_state_words(C.byref(hanabi_hip.make_config("Hanabi-Small", cfg.players, 0)))


def synth_row(cfg, hand, deck, know=None, cur=0, status=0, seat=0):
    """A state row that holds only what hb_belief_carry reads: the deck size, seat to act and status (word 0), `seat`'s hand size
    (word 1), its hand word and knowledge words, and the undealt deck bytes (the last len(deck) positions)."""
    P, D = cfg.players, 20
    row = np.zeros(state_words(cfg), np.uint32)
    row[0] = len(deck) | (cur << 13) | (status << 19)
    row[1] = len(hand) << (15 + 3 * seat)
    word = 0x1FFFFFF
    for s, c in enumerate(hand):
        word = (word & ~(31 << (5 * s))) | (c << (5 * s))
    row[10 + seat] = word
    kn = 0
    for s, k in enumerate(know if know is not None else [ALL] * len(hand)):
        kn |= k << (12 * s)
    row[10 + P + 2 * seat], row[10 + P + 2 * seat + 1] = kn & M32, kn >> 32
    row[10 + 3 * P:].view(np.uint8)[D - len(deck):D] = deck
    return row


def old_row(cfg, hand, seat=0):
    """A particle of the previous turn: only its hand word is read."""
    return synth_row(cfg, hand, [], seat=seat)


def cards(cfg, row, seat=0):
    n = (int(row[1]) >> (15 + 3 * seat)) & 7
    return [(int(row[10 + seat]) >> (5 * s)) & 31 for s in range(n)]


def deck_of(cfg, row):
    size = int(row[0]) & 63
    return sorted(int(c) for c in row[10 + 3 * cfg.players:].view(np.uint8)[20 - size:20])


def carry_one(cfg, cur, old_hand, slot, rev, drew, K=1, weight=1, **kw):
    from hanabi_hip import belief_carry_ref

    old = np.stack([old_row(cfg, old_hand)] * K)
    return belief_carry_ref(cfg, cur[None], old, np.full(K, weight, np.uint32), [slot], [rev], [drew], 0, K, 3, 1, details=True, **kw)


def test_a_hint_keeps_every_card_and_weighs_by_the_partners_draw():
    cfg = small_cfg()
    cur = synth_row(cfg, [7, 3], [3, 8, 8])   # (the true hand holds the same cards in another order: matching is by card)
    rows, w, info = carry_one(cfg, cur, [3, 7], -1, -1, 8)
    # kept = [3, 7] take pool elements 1 and 0; the free pool is then {3, 8, 8}: g = 1 + 2; no new slot
    assert info[0] == dict(dead=0, kept=[3, 7], g=3, ns=[]) and w[0] == 3
    assert cards(cfg, rows[0]) == [3, 7] and deck_of(cfg, rows[0]) == [3, 8, 8]
    other = np.ones(len(cur), bool)
    other[[10, 16, 17, 18, 19, 20]] = False   # only the hand word and the deck words may differ
    assert np.array_equal(rows[0][other], cur[other])
    rows, w, info = carry_one(cfg, cur, [3, 7], -1, -1, -1)
    assert w[0] == 1 and info[0]["g"] == 1   # no visible draw: no factor


def test_a_play_whose_card_matches_removes_it_and_draws_the_new_slot():
    cfg = small_cfg()
    cur = synth_row(cfg, [7, 1], [2, 2, 8])
    rows, w, info = carry_one(cfg, cur, [3, 7], 0, 3, 2, K=64)
    # kept = [7] takes pool element 0; free pool {1, 2, 2, 8}: g = 1 + 2 = 3; the new slot has n = 4 candidates: weight 12
    seen = set()
    for k in range(64):
        assert info[k] == dict(dead=0, kept=[7], g=3, ns=[4]) and w[k] == 12
        hand = cards(cfg, rows[k])
        assert hand[0] == 7 and hand[1] in (1, 2, 8)
        assert sorted(deck_of(cfg, rows[k]) + [hand[1]]) == [1, 2, 2, 8]
        seen.add(hand[1])
    assert seen == {1, 2, 8}   # 64 particles with their own row ids draw every kind


def test_a_play_whose_card_does_not_match_is_dead():
    cfg = small_cfg()
    cur = synth_row(cfg, [7, 1], [2, 2, 8])
    for slot, rev in ((0, 4), (0, -1), (1, 3), (2, 3)):   # another card; none seen; the other slot's card; no such slot
        rows, w, info = carry_one(cfg, cur, [3, 7], slot, rev, 2)
        assert info[0]["dead"] == 2 and w[0] == 0 and np.array_equal(rows[0], cur)


def test_a_kept_card_ruled_out_by_a_hint_received_since_is_dead():
    cfg = small_cfg()
    not_rank3 = ALL & ~(1 << (5 + 3))
    cur = synth_row(cfg, [7, 3], [3, 8, 8], know=[not_rank3, ALL])   # slot 0 was told "not a 4" (rank index 3): card 3 is out
    rows, w, info = carry_one(cfg, cur, [3, 7], -1, -1, 8)
    assert info[0]["dead"] == 4 and w[0] == 0 and np.array_equal(rows[0], cur)
    not_colour1 = ALL & ~2
    cur = synth_row(cfg, [7, 3], [3, 8, 8], know=[ALL, not_colour1])   # slot 1 was told "not colour 1": card 7 is out
    assert carry_one(cfg, cur, [3, 7], -1, -1, 8)[2][0]["dead"] == 4
    cur = synth_row(cfg, [7, 3], [3, 8, 8], know=[ALL, ALL & ~1])      # "not colour 0" leaves 7 in
    assert carry_one(cfg, cur, [3, 7], -1, -1, 8)[1][0] == 3


def test_a_kept_card_without_a_copy_left_is_dead():
    cfg = small_cfg()
    cur = synth_row(cfg, [7, 9], [8, 8])   # the partner's new card took the last 3: none in my hand or the deck
    rows, w, info = carry_one(cfg, cur, [3, 7], -1, -1, 3)
    assert info[0]["dead"] == 4 and w[0] == 0 and np.array_equal(rows[0], cur)
    cur = synth_row(cfg, [7, 3], [8, 8])   # one 3 in the pool, two in the old hand: the second finds none
    assert carry_one(cfg, cur, [3, 3], -1, -1, -1)[2][0]["dead"] == 4
    cur = synth_row(cfg, [3, 3], [8, 8])
    assert carry_one(cfg, cur, [3, 3], -1, -1, -1)[1][0] == 1


def test_a_draw_of_the_new_cards_kind_gives_k_times_k_plus_one():
    cfg = small_cfg()
    cur = synth_row(cfg, [7, 2], [2, 8])
    rows, w, info = carry_one(cfg, cur, [3, 7], 0, 3, 2, K=64)
    # after the kept 7 the free pool is {2, 2, 8}: k = 2 copies of the card the partner drew, g = k + 1 = 3, n = 3, weight 9 each.
    # The k particles-in-expectation whose new card is a 2 weigh k (k + 1) of the total together, the one with the 8 weighs k + 1
    # (the ordered pairs of distinct physical cards (mine, the partner's) out of a deck that held k + 1 copies)
    assert all(x == 9 for x in w) and all(n == dict(dead=0, kept=[7], g=3, ns=[3]) for n in info)
    new = [cards(cfg, r)[1] for r in rows]
    assert set(new) == {2, 8}
    p2 = new.count(2) / 64   # 2 of the 3 candidates: 64 draws lie within 6 sigma of 2 / 3
    assert abs(p2 - 2 / 3) < 6 * math.sqrt(2 / 9 / 64)
    assert carry_one(cfg, cur, [3, 7], 0, 3, 2, draw_weight=False)[1][0] == 3   # the wrong variant drops g


def test_an_empty_deck_with_a_short_hand_has_no_new_slot():
    cfg = small_cfg()
    cur = synth_row(cfg, [3], [])
    rows, w, info = carry_one(cfg, cur, [3, 7], 1, 7, -1)
    assert info[0] == dict(dead=0, kept=[3], g=1, ns=[]) and w[0] == 1 and np.array_equal(rows[0], cur)
    # two kept cards do not fit a hand of one
    assert carry_one(cfg, cur, [3, 7], -1, -1, -1)[2][0]["dead"] == 2


def test_dead_inputs_give_unchanged_copies():
    cfg = small_cfg()
    for cur in (synth_row(cfg, [7, 3], [3, 8], status=1), synth_row(cfg, [7, 3], [3, 8], status=3),   # a finished root
                synth_row(cfg, [7, 3], [3, 8], cur=1)):                                                # not my turn
        rows, w, info = carry_one(cfg, cur, [3, 7], -1, -1, -1)
        assert info[0]["dead"] == 1 and w[0] == 0 and np.array_equal(rows[0], cur)
    cur = synth_row(cfg, [7, 3], [3, 8])
    rows, w, info = carry_one(cfg, cur, [3, 7], -1, -1, -1, weight=0)   # old_weight == 0
    assert info[0]["dead"] == 1 and w[0] == 0 and np.array_equal(rows[0], cur)
    assert carry_one(cfg, cur, [3, 7], -1, -1, -1, weight=0xFFFFFFFF)[1][0] == 1   # any other weight counts as 1


def test_a_split_call_gives_the_same_rows():
    from hanabi_hip import belief_carry_ref

    cfg = small_cfg()
    cur = np.stack([synth_row(cfg, [7, 1], [2, 2, 8, 5]), synth_row(cfg, [0, 6], [0, 1, 1, 9])])
    old = np.stack([old_row(cfg, h) for h in ([3, 7], [7, 3], [3, 31], [0, 6], [6, 6], [31, 6])])
    args = ([0, 1], [3, 6], [2, -1])
    whole = belief_carry_ref(cfg, cur, old, np.ones(6, np.uint32), *args, 0, 3, (5 << 40) | 9, (1 << 35) | 2, first_row_id=100)
    for i in range(2):
        part = belief_carry_ref(cfg, cur[i:i + 1], old[3 * i:3 * i + 3], np.ones(3, np.uint32), *(a[i:i + 1] for a in args), 0, 3,
                                (5 << 40) | 9, (1 << 35) | 2, first_row_id=100 + 3 * i)
        assert np.array_equal(part[0], whole[0][3 * i:3 * i + 3]) and np.array_equal(part[1], whole[1][3 * i:3 * i + 3])
    # root 0 (slot 0 played, a 3 seen, the partner drew a 2; pool 7 1 | 2 2 8 5): [3, 7] keeps the 7, g = 3, n = 5; [7, 3] holds a
    # 7 where the 3 was seen: dead; [3, -] keeps nothing: g = 3, n = 6 * 5. root 1 (slot 1 played, a 6 seen, no draw; pool 0 6 | 0 1
    # 1 9): [0, 6] keeps the 0, n = 5; [6, 6] keeps a 6, n = 5; [-, 6] keeps nothing, n = 6 * 5
    assert whole[1].tolist() == [15, 0, 90, 5, 5, 30]


# ---- exactness by enumeration ------------------------------------------------------------------------------------------------------
# Scripted Hanabi-Small games, 2 players (uids: 0-1 discard, 2-3 play, 4-5 reveal colour, 6-10 reveal rank). The last two moves are
# mine and the partner's: the particles are exact V0 samples of the state before them, the target is the V0 belief of the state
# after them (uniform over the physical assignments of what I cannot see, given everything public by then).
DECK_A = [1, 9, 2, 0, 6, 7, 1, 5, 5, 3, 0, 5, 3, 2, 8, 8, 6, 4, 0, 7]
DECK_B = [5, 7, 1, 3, 2, 0, 1, 2, 8, 0, 5, 4, 6, 9, 3, 6, 5, 7, 8, 0]
TRANSITIONS = {
    "discard_then_discard_and_draw": (DECK_A, [8, 5, 1, 5, 1, 0]),   # the case built for g: the partner draws a card I may hold
    "discard_then_discard_and_draw_2": (DECK_A, [8, 5, 0, 1]),
    "hint_then_hinted": (DECK_B, [4, 0, 4, 6]),
    "play_then_play": (DECK_B, [4, 0, 4, 1, 2, 3]),
}
N_PARTICLES = 12000


def transition(deck, moves):
    """(cfg, then, prev, now): the oracle's rows before my move (the last but one), after it, and after the partner's."""
    O = _oracle()
    cfg = O.make_config("Hanabi-Small", 2, 0)
    env = O.OracleEnv(cfg, 1, seed=1, decks=np.asarray(deck, np.uint8)[None])
    rows = []
    for j, u in enumerate(moves):
        if j >= len(moves) - 2:
            rows.append(env.export_state()[0].copy())
        env.step(np.asarray([u], np.int32))
    assert env.illegal_count() == 0
    rows.append(env.export_state()[0].copy())
    return (cfg,) + tuple(rows)


def as_tensor(rows):
    return torch.from_numpy(np.ascontiguousarray(rows, np.uint32).view(np.int32).copy())


def observed(game, now, then, moves, prev, seat):
    from hanabi_hip import TrackedBelief

    got = TrackedBelief(game, 2).observed(as_tensor(now), as_tensor(then), torch.as_tensor(moves), as_tensor(prev), seat)
    return tuple(t.numpy() for t in got)


_CARRIED = {}


def carried(name, draw_weight=True):
    """The N_PARTICLES exact V0 samples of the state before my move, carried -> (cfg, now, seat, rows, weights)."""
    from hanabi_hip import belief_carry_ref

    key = (name, draw_weight)
    if key not in _CARRIED:
        deck, moves = TRANSITIONS[name]
        cfg, then, prev, now = transition(deck, moves)
        seat = (int(then[0]) >> 13) & 7
        assert (int(now[0]) >> 13) & 7 == seat and (int(now[0]) >> 19) & 3 == 0
        if (name, "old") not in _CARRIED:
            old, ow = np.empty((N_PARTICLES, len(then)), np.uint32), np.empty(N_PARTICLES, np.uint32)
            for o in range(N_PARTICLES):
                old[o], ow[o], _ = determinize_row(cfg, then, seat, 5, 1, o)
            assert ow.min() == ow.max() > 0   # a state reached by play: the V0 samples weigh the same
            _CARRIED[(name, "old")] = (old, ow)
        old, ow = _CARRIED[(name, "old")]
        slot, rev, drew = observed("Hanabi-Small", now[None], then[None], moves[-2:-1], prev[None], seat)
        rows, w = belief_carry_ref(cfg, now[None], old, ow, slot, rev, drew, seat, N_PARTICLES, 7, 2, draw_weight=draw_weight)
        _CARRIED[key] = (cfg, now, seat, rows, w, (int(slot[0]), int(rev[0]), int(drew[0])))
    return _CARRIED[key]


def worst_deviation(cfg, now, seat, rows, w):
    """The largest |weighted frequency - exact probability| over whole hands, in binomial standard errors. The standard error
    of a weighted frequency is that of n_eff = (sum w)^2 / sum w^2 equally weighted draws (Kish); the weights here take at most
    a handful of values (g in 1 .. 4 times one n), so n_eff is within a few percent of the live count."""
    exact = enumerate_hands(cfg, now, seat)
    total = sum(t for t, _, _ in exact.values())
    acc = {}
    for o in np.nonzero(w)[0]:
        h = hand_types(cfg, rows[o], seat)
        acc[h] = acc.get(h, 0) + int(w[o])
    assert set(acc) <= set(exact)   # nothing the posterior excludes is ever drawn
    sw = float(w.sum())
    n_eff = sw * sw / float((w.astype(np.float64) ** 2).sum())
    assert min(t for t, _, _ in exact.values()) / total * n_eff >= 10   # every hand is expected often enough for the bound
    worst = max(abs(acc.get(h, 0) / sw - t / total) / math.sqrt(t / total * (1 - t / total) / n_eff) for h, (t, _, _) in exact.items())
    return worst, len(exact), n_eff


@pytest.mark.parametrize("name", sorted(TRANSITIONS))
def test_carried_samples_follow_the_enumerated_posterior(name):
    cfg, now, seat, rows, w, seen = carried(name)
    worst, hands, n_eff = worst_deviation(cfg, now, seat, rows, w)
    print(name, "(own_slot, revealed, drew) =", seen, "hands", hands, "n_eff", round(n_eff), "worst deviation", round(worst, 2), "SE")
    assert hands >= 10 and worst <= 6.0


def test_the_transitions_are_the_three_kinds():
    seen = {name: carried(name)[5] for name in TRANSITIONS}
    slot, rev, drew = seen["discard_then_discard_and_draw"]
    assert slot >= 0 and rev >= 0 and drew >= 0     # I discard; the partner discards and draws
    assert seen["hint_then_hinted"] == (-1, -1, -1)   # I hint, the partner hints me: nothing leaves, nothing is drawn
    cfg, now, seat, rows, w, _ = carried("hint_then_hinted")
    assert 0 < np.count_nonzero(w) < len(w)           # ... and the hint I received rules samples out
    slot, rev, drew = seen["play_then_play"]
    deck, moves = TRANSITIONS["play_then_play"]
    assert slot == moves[-2] - 2 and rev >= 0 and 2 <= moves[-1] <= 3 and drew >= 0
    cfg, then, prev, now = transition(deck, moves)
    played = ((int(now[2]) >> 12) & 7) * 5 + ((int(now[2]) >> 15) & 7)   # the card the partner played: of a kind I may hold
    assert any(played in h for h in enumerate_hands(cfg, prev, seat)) and (int(now[2]) >> 4) & 3 < 2   # (a card move of the partner's)


def test_without_the_draw_weight_the_bound_fails():
    name = "discard_then_discard_and_draw"
    cfg, now, seat, rows, w, seen = carried(name, draw_weight=False)
    worst, hands, n_eff = worst_deviation(cfg, now, seat, rows, w)
    print(name, "with g = 1: worst deviation", round(worst, 2), "SE")
    assert worst > 6.0
    # the case is one: some hypotheses hold the card the partner drew and some do not
    exact = enumerate_hands(cfg, now, seat)
    assert any(seen[2] in h for h in exact) and any(seen[2] not in h for h in exact)


# ---- invariants on random play ------------------------------------------------------------------------------------------------------
def test_the_true_hand_is_never_killed_on_random_play():
    from hanabi_hip import belief_carry_ref

    O = _oracle()
    cfg = O.make_config("Hanabi-Full", 2, 0)
    n, H = 64, cfg.hand_size   # (random play loses its lives within some 30 turns: most of the checks come from the first 20)
    env = O.OracleEnv(cfg, n, seed=5)
    legal = env.observe()["legal"]
    history = [env.export_state().copy()]   # history[t] = the rows before move t
    moves = []
    for t in range(60):
        act = O.random_legal_actions(legal, 6, t)
        moves.append(act.copy())
        legal = env.step(act)["legal"]
        history.append(env.export_state().copy())
    checked = branches = 0
    for t in range(58):
        then, prev, now = history[t], history[t + 1], history[t + 2]
        seat = t % 2
        ok = (((now[:, 0] >> 19) & 3) == 0) & (((then[:, 0] >> 13) & 7) == seat)
        if not ok.any():
            continue
        slot, rev, drew = observed("Hanabi-Full", now, then, moves[t], prev, seat)
        rows, w, info = belief_carry_ref(cfg, now, then, np.ones(n, np.uint32), slot, rev, drew, seat, 1, 9, t, details=True)
        for i in np.nonzero(ok)[0]:
            assert w[i] > 0 and info[i]["dead"] == 0, (t, i, info[i])
            k = len(info[i]["kept"])
            true_now = [(int(now[i, 10 + seat]) >> (5 * s)) & 31 for s in range(H)]
            got = [(int(rows[i, 10 + seat]) >> (5 * s)) & 31 for s in range(H)]
            assert got[:k] == true_now[:k] == info[i]["kept"]
            # what was observed is what happened: the slot of my card move and the card the oracle's last-move word names
            mv = int(moves[t][i])
            assert slot[i] == (mv % H if mv < 2 * H else -1)
            if mv < 2 * H:
                assert rev[i] == (int(then[i, 10 + seat]) >> (5 * (mv % H))) & 31
            pm = int(moves[t + 1][i])
            n_p = (int(now[i, 1]) >> (15 + 3 * (1 - seat))) & 7
            drew_true = pm < 2 * H and n_p == (int(prev[i, 1]) >> (15 + 3 * (1 - seat))) & 7
            assert drew[i] == ((int(now[i, 10 + 1 - seat]) >> (5 * (n_p - 1))) & 31 if drew_true else -1)
            checked += 1
            branches |= (1 if mv < 2 * H else 2) | (4 if drew_true else 8)
    assert checked > 500 and branches == 15   # my card moves and my hints, a partner that drew and one that did not


# ---- arguments, symbol ------------------------------------------------------------------------------------------------------------
class _Agent:
    def eval_moves(self, *a, **k):
        raise AssertionError("not called")

    def requires_vectorized_observation(self):
        return False


def test_argument_validation_needs_no_gpu():
    import hanabi_hip
    from hanabi_hip import SearchPlayer, TrackedBelief, belief_carry, exact_table

    cfg = hanabi_hip.make_config("Hanabi-Small", 2, 0)
    SW = state_words(cfg)
    z = lambda *shape: torch.zeros(shape, dtype=torch.int32)

    def call(m=2, Kn=3, seat=0, n_particles=None, **kw):
        a = dict(cur=z(m, SW), old=z(m * Kn, SW), w=z(m * Kn), slot=z(m), rev=z(m), drew=z(m))
        a.update(kw)
        return belief_carry(cfg, a["cur"], a["old"], a["w"], a["slot"], a["rev"], a["drew"], seat, Kn if n_particles is None else n_particles,
                            1, 0)

    with pytest.raises(ValueError, match="n_particles"):
        call(n_particles=0)
    for seat in (-1, 2):
        with pytest.raises(ValueError, match="seat"):
            call(seat=seat)
    with pytest.raises(ValueError, match="cur_rows"):
        call(cur=z(SW))
    for bad in (dict(old=z(5, SW)), dict(w=z(5)), dict(slot=z(3)), dict(rev=z(2).long()), dict(drew=z(2, 1)), dict(cur=z(2, SW + 1))):
        with pytest.raises(AssertionError):
            call(**bad)
    with pytest.raises(hanabi_hip.HbError):   # tensors that are not on a GPU: no CPU path
        call()

    team = [_Agent(), _Agent()]
    assert SearchPlayer(team, 0).track is False and SearchPlayer(team, 0, condition=True, track=True).track is True
    with pytest.raises(ValueError, match="condition=True"):
        SearchPlayer(team, 0, track=True)
    for bad in (1, "yes", None):
        with pytest.raises(TypeError, match="track"):
            SearchPlayer(team, 0, condition=True, track=bad)
    with pytest.raises(ValueError, match="2 players"):
        SearchPlayer(team + [_Agent()], 0, condition=True, track=True)
    with pytest.raises(ValueError, match="confirm_replicas"):
        SearchPlayer(team, 0, condition=True, track=True, replicas=4, oversample=2, confirm_replicas=5)
    SearchPlayer(team, 0, condition=True, track=True, replicas=4, oversample=2, confirm_replicas=4)
    with pytest.raises(ValueError, match="4096"):
        SearchPlayer(team, 0, condition=True, track=True, replicas=1024, oversample=8)
    sp = SearchPlayer(team, 1, condition=True, track=True, depth=2, epsilon=0.25)
    assert [getattr(sp, k) for k in SearchPlayer.TRACK_COUNTERS] == [0, 0, 0] and SearchPlayer.TRACK_COUNTERS == ("tracked", "restarts", "carried_live")
    assert sp.depth_stats()["carried_ess"] == 0.0 and "carried_ess" not in SearchPlayer(team, 1, condition=True, depth=2).depth_stats()
    assert sp._tracked is None and sp._track_stats is None   # nothing is allocated before the first call
    assert set(SearchPlayer(team, 0, condition=True, track=True, score_belief=True).belief_stats()) >= {"tracked", "restarted"}
    assert "tracked" not in SearchPlayer(team, 0, condition=True, score_belief=True).belief_stats()
    with pytest.raises(ValueError, match="2 players"):
        TrackedBelief("Hanabi-Full", 3)
    with pytest.raises(ValueError, match="replicas and oversample"):
        TrackedBelief("Hanabi-Full", 2, replicas=0)
    with pytest.raises(ValueError, match="4096"):
        TrackedBelief("Hanabi-Full", 2, replicas=1024, oversample=8)
    t = exact_table(4).numpy()
    assert t.tolist() == [[0, 1, 1, 1, 1], [0, 0, 0, 0, 0]]
    with pytest.raises(ValueError, match="n_actions"):
        exact_table(0)


def test_symbol_is_exported_and_bound():
    import hanabi_hip
    from hanabi_hip import _capi

    assert "hb_belief_carry" in _capi.SIGNATURES
    fn = hanabi_hip.lib().hb_belief_carry
    assert fn.argtypes == _capi.SIGNATURES["hb_belief_carry"][1] and len(fn.argtypes) == 16
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hanabi_hip.h")).read()
    assert "int hb_belief_carry(const hb_config* cfg" in header
    for name in ("belief_carry", "belief_carry_ref", "TrackedBelief", "TrackedRows", "exact_table"):
        assert name in hanabi_hip.__all__ and hasattr(hanabi_hip, name)
    # the entry point checks its arguments before anything else: a null config is refused
    rc = fn(None, None, None, None, None, None, None, 1, 0, 1, 0, 0, 0, None, None, None)
    assert rc != 0
