"""Belief-sampled rollout search, the parts that need no GPU: a numpy restatement of hb_belief_determinize's rule
(include/hanabi_hip.h), its unbiasedness by exact enumeration, its invariants on states reached by random play, and the argument
validation of the two new entry points. tests/test_search_gpu.py holds the kernel to this restatement bit for bit."""
import ctypes as C
import math

import numpy as np
import pytest

M32 = 0xFFFFFFFF


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def philox_np(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays (broadcast); returns the four output words as uint32 arrays."""
    c0, c1, c2, c3 = (np.asarray(x, np.uint64) & np.uint64(M32) for x in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = int(k0) & M32, int(k1) & M32
    m32 = np.uint64(M32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)
        c0, c1, c2, c3 = n0, p1 & m32, n2, p0 & m32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return tuple(x.astype(np.uint32) for x in (c0, c1, c2, c3))


def deck_size_of(cfg):
    return cfg.colors * sum(3 if r == 0 else 1 if r == cfg.ranks - 1 else 2 for r in range(cfg.ranks))


def seat_view(cfg, row, seat):
    """What the rule reads of a state row: (observing seat or None when the row gives weight 0, hand word,
    knowledge u64, pool = the cards of the hand slots oldest first then of the undealt deck positions ascending, hand size,
    first undealt deck position)."""
    P, D = cfg.players, deck_size_of(cfg)
    w0, w1 = int(row[0]), int(row[1])
    st = seat if seat >= 0 else (w0 >> 13) & 7
    if (w0 >> 19) & 3 != 0 or st >= P:
        return None, 0, 0, [], 0, 0
    hand = int(row[10 + st])
    know = int(row[10 + P + 2 * st]) | int(row[10 + P + 2 * st + 1]) << 32
    n_hand = min((w1 >> (15 + 3 * st)) & 7, cfg.hand_size)
    deck_size = min(w0 & 63, D)
    deck_pos = D - deck_size
    deck = np.ascontiguousarray(row[10 + 3 * P:], dtype="<u4").view(np.uint8)
    pool = [(hand >> (5 * l)) & 31 for l in range(n_hand)] + [int(deck[q]) for q in range(deck_pos, D)]
    return st, hand, know, pool, n_hand, deck_pos


def plausible(cfg, know, s, card):
    kn = (know >> (12 * s)) & 0xFFF
    col, rk = divmod(card, cfg.ranks)
    return col < cfg.colors and bool((kn >> col) & 1) and bool((kn >> (5 + rk)) & 1)


def determinize_row(cfg, row, seat, seed, draw, row_id, unit_weights=False):
    """One output row of hb_belief_determinize: (row_out uint32 [SW], weight, [n_0, n_1, ...] as far as the slots got).
    unit_weights: the deliberately wrong variant whose weights are all 1."""
    row = np.asarray(row, np.uint32)
    st, hand, know, pool, n_hand, deck_pos = seat_view(cfg, row, seat)
    if st is None:
        return row.copy(), 0, []
    P, D = cfg.players, deck_size_of(cfg)
    rid = int(row_id) & 0xFFFFFFFFFFFFFFFF
    rnd = philox_np(128 + np.arange(64), draw & M32, rid & M32, rid >> 32, seed & M32, ((seed >> 32) ^ (draw >> 32)) & M32)
    taken, weight, ns, new_hand = set(), 1, [], hand
    for s in range(n_hand):
        cand = [l for l in range(len(pool)) if l not in taken and plausible(cfg, know, s, pool[l])]
        ns.append(len(cand))
        if not cand:
            return row.copy(), 0, ns
        idx = cand[(int(rnd[0][s]) * len(cand)) >> 32]
        taken.add(idx)
        weight *= len(cand)
        new_hand = (new_hand & ~(31 << (5 * s))) | (pool[idx] << (5 * s))
    rest = [l for l in range(len(pool)) if l not in taken]
    rest.sort(key=lambda l: (int(rnd[1][l]) & ~63) | l)
    out = row.copy()
    out[10 + st] = new_hand
    deck = out[10 + 3 * P:].view(np.uint8)
    for r, l in enumerate(rest):
        deck[deck_pos + r] = pool[l]
    return out, (1 if unit_weights else weight), ns


def determinize_ref(cfg, rows, seat, replicas, seed, draw, first_row_id=0):
    """hb_belief_determinize: rows [m, SW] -> (rows_out uint32 [m * replicas, SW], weights uint32 [m * replicas])."""
    rows = np.asarray(rows).astype(np.uint32)
    out = np.empty((rows.shape[0] * replicas, rows.shape[1]), np.uint32)
    w = np.empty(rows.shape[0] * replicas, np.uint32)
    for o in range(out.shape[0]):
        out[o], w[o], _ = determinize_row(cfg, rows[o // replicas], seat, seed, draw, first_row_id + o)
    return out, w


def hand_types(cfg, row, seat):
    st, hand, _, _, n_hand, _ = seat_view(cfg, row, seat)
    return tuple((hand >> (5 * s)) & 31 for s in range(n_hand))


# ---- exact enumeration ------------------------------------------------------------------------------------------------------------
def enumerate_hands(cfg, row, seat):
    """Every way the rule's slot-by-slot walk can go, over card TYPES with multiplicities. Returns {hand: (T, S2, p)}:
    T  = number of assignments of distinct physical pool cards to the hand slots, every slot plausible, that give `hand`
         (each extends to the same deck_size! orders of the undealt deck, so these are the full assignment counts up to that
         constant factor);
    S2 = E[w^2 [hand]] of the importance sampler = sum over the physical paths of their weight prod n_s;
    p  = probability that the sampler draws `hand`."""
    st, _, know, pool, n_hand, _ = seat_view(cfg, row, seat)
    counts = {}
    for c in pool:
        counts[c] = counts.get(c, 0) + 1
    res = {}

    def walk(s, hand, paths, weight):
        # `paths` physical paths lead here, each with weight `weight` so far and probability 1 / weight
        if s == n_hand:
            t, s2, p = res.get(hand, (0, 0, 0.0))
            res[hand] = (t + paths, s2 + paths * weight, p + paths / weight)
            return
        n = sum(k for c, k in counts.items() if k and plausible(cfg, know, s, c))
        for c in sorted(counts):
            k = counts[c]
            if k and plausible(cfg, know, s, c):
                counts[c] -= 1
                walk(s + 1, hand + (c,), paths * k, weight * n)
                counts[c] += 1

    walk(0, (), 1, 1)
    return res


# ---- oracle states ------------------------------------------------------------------------------------------------------------------
def _oracle():
    from oracle import oracle_py as O

    return O


def scripted_state(game, players, deck, moves):
    """The oracle's state row after `moves` (uids, one per turn) on the explicit `deck`; every move must be legal."""
    O = _oracle()
    cfg = O.make_config(game, players, 0)
    env = O.OracleEnv(cfg, 1, seed=1, decks=np.asarray(deck, np.uint8)[None])
    for u in moves:
        env.step(np.asarray([u], np.int32))
    assert env.illegal_count() == 0
    return cfg, env.export_state()[0]


def random_play_rows(game, players, n, seed, turns):
    """n oracle games after `turns` random legal moves each (games that ended earlier stay as they ended)."""
    O = _oracle()
    cfg = O.make_config(game, players, 0)
    env = O.OracleEnv(cfg, n, seed=seed)
    legal = env.observe()["legal"]
    for t in range(turns):
        legal = env.step(O.random_legal_actions(legal, seed + 1, t))["legal"]
    return cfg, env.export_state()


# Hanabi-Small, 2 players (cards: colour * 5 + rank; 2 colours, hand of 2, 3 information tokens, 1 life): (deck, moves). Each
# script was found by a search over careful play (hints, discards, plays of playable cards) and ends with 3 - 5 cards left to
# draw, the observer (the seat to move) holding cards it was told a colour and a rank of.
# uids: 0-1 discard, 2-3 play, 4-5 reveal colour, 6-10 reveal rank.
SMALL_SCRIPTS = [
    ([2, 2, 5, 7, 4, 9, 3, 0, 5, 5, 8, 6, 0, 1, 6, 8, 1, 7, 0, 3],
     [8, 2, 4, 0, 1, 4, 0, 4, 1, 9, 4, 9, 1, 5, 1, 5, 1, 4, 3, 1, 1, 7, 7]),
    ([6, 0, 1, 5, 0, 6, 9, 2, 5, 8, 7, 5, 4, 3, 8, 2, 3, 1, 7, 0],
     [6, 1, 3, 2, 5, 7, 4, 0, 1, 3, 9, 6, 3, 0, 6, 0, 2, 1, 1, 5, 1, 8]),
    ([6, 0, 5, 1, 9, 4, 3, 0, 7, 0, 3, 5, 2, 1, 6, 8, 7, 2, 5, 8],
     [6, 7, 6, 2, 3, 2, 2, 0, 4, 3, 0, 1, 5, 6, 1, 0, 4, 8, 0, 4]),
    ([7, 1, 3, 6, 1, 8, 5, 4, 9, 8, 5, 0, 0, 2, 7, 5, 0, 3, 2, 6],
     [7, 7, 0, 7, 4, 1, 4, 0, 9, 0, 1, 2, 4, 1, 0, 4, 0, 4, 1, 8, 1, 6]),
]
# Hanabi-Full, 2 players (hand of 5), found the same way: 9 cards left to draw, 60 possible hands.
# uids: 0-4 discard, 5-9 play, 10-14 reveal colour, 15-19 reveal rank.
FULL_SCRIPT = (
    [15, 23, 2, 21, 12, 2, 12, 5, 7, 11, 24, 4, 9, 15, 3, 20, 11, 10, 0, 5, 5, 10, 8, 6, 13, 10, 0, 18, 1, 21, 6, 8, 17, 17, 1, 7, 22,
     16, 13, 22, 19, 16, 0, 14, 3, 18, 20, 20, 23, 15],
    [16, 12, 5, 3, 2, 7, 10, 0, 12, 17, 13, 18, 10, 11, 19, 14, 3, 10, 3, 18, 1, 16, 7, 0, 8, 16, 4, 0, 11, 15, 8, 0, 1, 16, 0, 4, 0, 2,
     6, 4, 4, 0, 8, 10, 0, 15, 9, 8, 2, 15, 13, 4, 4, 19])


def small_states():
    return [scripted_state("Hanabi-Small", 2, deck, moves) for deck, moves in SMALL_SCRIPTS]


def played_states():
    return small_states() + [scripted_state("Hanabi-Full", 2, *FULL_SCRIPT)]


def weights_vary(exact):
    """The walk's weights differ from path to path (n_1 depends on the card slot 0 took): T / p is the weight of a hand's paths."""
    return len({round(t / p, 6) for t, s2, p in exact.values()}) >= 2


def crossed_states():
    """States in which n_1 DOES depend on the card slot 0 took. No sequence of moves reaches one: a slot's knowledge changes only
    when a hint is given, every hint tells every card in the hand at that time something, and the slots are ordered by age, so an
    older slot has been through every hint a newer one has; where the two were told the same their constraints agree, where not
    they exclude each other. The plausible sets of a hand are therefore nested or disjoint, older inside newer, and the walk's
    n_s = |S_s| - (older slots inside S_s) does not depend on the cards taken: in every state reached by play all replicas carry
    the same weight and none is dead (test_weights_are_constant_on_states_reached_by_play). The rule itself is defined, and
    unbiased, for any knowledge bits; to exercise it the scripted Small states get the observer's knowledge overwritten by a
    crossing pair: slot 0 knows its colour (only), slot 1 its rank (only)."""
    out = []
    for cfg, row in small_states():
        st = (int(row[0]) >> 13) & 7
        for col in range(cfg.colors):
            for rk in range(cfg.ranks):
                r = row.copy()
                know = ((1 << col) | 0x3E0 | 0x400) | (((0x1F | (1 << (5 + rk))) | 0x800) << 12)
                r[10 + cfg.players + 2 * st], r[10 + cfg.players + 2 * st + 1] = know & M32, know >> 32
                ex = enumerate_hands(cfg, r, -1)
                if len(ex) >= 2 and weights_vary(ex) and min(p for _, _, p in ex.values()) * N_SAMPLES >= 50:
                    out.append((cfg, r))
                    break
            else:
                continue
            break
    return out


N_SAMPLES = 20000


def _sample_means(cfg, row, n, unit_weights, seed=11, draw=3):
    """Sample mean of w * [hand == h] for every hand h the n samples drew."""
    acc = {}
    for o in range(n):
        out, w, _ = determinize_row(cfg, row, -1, seed, draw, o, unit_weights=unit_weights)
        if w:
            h = hand_types(cfg, out, -1)
            acc[h] = acc.get(h, 0) + w
    return {h: v / n for h, v in acc.items()}


def _violations(exact, means, n, scale=1.0, wrong=False):
    """Hands whose sample mean lies more than 6 sigma from the exact count T. sigma^2 = (E[w^2 [h]] - T^2) / n, from the
    enumeration. For the weight-blind variant (`wrong`: every sample weighs `scale`) the estimator is scale * [hand == h]: a
    Bernoulli(p) scaled, whose sigma^2 = scale^2 p (1 - p) / n."""
    bad = []
    for h, (t, s2, p) in exact.items():
        var = (scale * scale * p * (1 - p) if wrong else s2 - t * t) / n
        got = scale * means.get(h, 0.0)
        if abs(got - t) > 6 * math.sqrt(max(var, 0.0)) + 1e-9 * t:
            bad.append((h, t, got, math.sqrt(max(var, 0.0))))
    return bad


def _check_state_is_a_real_test(cfg, row, exact):
    st, _, know, pool, n_hand, _ = seat_view(cfg, row, -1)
    assert st is not None and n_hand == cfg.hand_size
    bits = [(know >> (12 * s)) & 0xFFF for s in range(n_hand)]
    assert any(b & 0x400 for b in bits) and any(b & 0x800 for b in bits)   # the observer holds a colour-hinted and a rank-hinted card
    assert len(exact) >= 3
    # every hand is drawn often enough for the 6 sigma bound to mean what it says
    assert min(p for _, _, p in exact.values()) * N_SAMPLES >= 50


def test_philox_restatement_matches_the_oracle():
    O = _oracle()
    rng = np.random.default_rng(0)
    for _ in range(20):
        c = rng.integers(0, 2 ** 32, 4, dtype=np.uint64)
        k = rng.integers(0, 2 ** 32, 2, dtype=np.uint64)
        want = O.philox(c.astype(np.uint32), k.astype(np.uint32))
        got = philox_np(c[0], c[1], c[2], c[3], int(k[0]), int(k[1]))
        assert [int(x) for x in got] == [int(x) for x in want]


def test_search_is_exported():
    import hanabi_hip
    from hanabi_hip import _capi

    for name in ("Determinizer", "RolloutSearch", "SearchPlayer", "SearchResult"):
        assert hasattr(hanabi_hip, name) and name in hanabi_hip.__all__
    assert "hb_belief_determinize" in _capi.SIGNATURES and "hb_search_reduce" in _capi.SIGNATURES
    from hanabi_hip.selfplay import SelfPlaySession

    assert callable(SelfPlaySession.search)
    with pytest.raises(ValueError):
        hanabi_hip.RolloutSearch(replicas=0)


def test_argument_validation_needs_no_gpu():
    import hanabi_hip

    L = hanabi_hip.lib()
    cfg = hanabi_hip.make_config()
    ref = C.byref(cfg)
    one = C.c_void_p(16)
    err = lambda: L.hb_last_error()
    assert L.hb_belief_determinize(None, one, 4, -1, 2, 1, 1, 0, one, one, None) < 0 and b"null" in err()
    assert L.hb_belief_determinize(ref, None, 4, -1, 2, 1, 1, 0, one, one, None) < 0 and b"null" in err()
    assert L.hb_belief_determinize(ref, one, 4, -1, 2, 1, 1, 0, None, one, None) < 0 and b"null" in err()
    assert L.hb_belief_determinize(ref, one, 4, -1, 2, 1, 1, 0, one, None, None) < 0 and b"null" in err()
    assert L.hb_belief_determinize(ref, one, 4, -1, 0, 1, 1, 0, one, one, None) < 0 and b"replicas" in err()
    assert L.hb_belief_determinize(ref, one, 4, 2, 2, 1, 1, 0, one, one, None) < 0 and b"seat" in err()
    assert L.hb_belief_determinize(ref, one, 4, -2, 2, 1, 1, 0, one, one, None) < 0 and b"seat" in err()
    assert L.hb_belief_determinize(ref, one, -1, -1, 2, 1, 1, 0, one, one, None) < 0
    assert L.hb_belief_determinize(ref, one, 1 << 30, -1, 4, 1, 1, 0, one, one, None) < 0 and b"2^31" in err()
    bad = hanabi_hip.HbConfig(6, 5, 5, 5, 8, 3, 0)
    assert L.hb_belief_determinize(C.byref(bad), one, 4, -1, 2, 1, 1, 0, one, one, None) < 0 and b"players" in err()
    assert L.hb_belief_determinize(ref, one, 0, -1, 2, 1, 1, 0, one, one, None) == 0       # empty: no-op
    assert L.hb_search_reduce(None, one, one, 4, 20, 8, one, one, one, one, None) < 0 and b"null" in err()
    assert L.hb_search_reduce(one, one, one, 4, 20, 8, None, one, one, one, None) < 0 and b"null" in err()
    assert L.hb_search_reduce(one, one, one, 4, 0, 8, one, one, one, one, None) < 0 and b"n_actions" in err()
    assert L.hb_search_reduce(one, one, one, 4, 65, 8, one, one, one, one, None) < 0 and b"n_actions" in err()
    assert L.hb_search_reduce(one, one, one, 4, 20, 0, one, one, one, one, None) < 0 and b"replicas" in err()
    assert L.hb_search_reduce(one, one, one, -1, 20, 8, one, one, one, one, None) < 0
    assert L.hb_search_reduce(one, one, one, 0, 20, 8, one, one, one, None, None) == 0


def test_played_states_are_late_hinted_and_constraining():
    for cfg, row in played_states():
        _, _, _, pool, n_hand, _ = seat_view(cfg, row, -1)
        assert n_hand + 1 <= len(pool) <= n_hand + 9   # a handful of cards left to draw
        exact = enumerate_hands(cfg, row, -1)
        _check_state_is_a_real_test(cfg, row, exact)
        assert len(exact) < len(set(pool)) ** n_hand   # plausibility rules hands out
    assert len(crossed_states()) >= 3


def test_weights_are_constant_on_states_reached_by_play():
    """crossed_states' argument, checked: on rows reached by play every replica has the same weight and none is dead."""
    for game, players in (("Hanabi-Full", 2), ("Hanabi-Full", 5), ("Hanabi-Small", 2)):
        cfg, rows = random_play_rows(game, players, 32, seed=8, turns=18)
        for i, row in enumerate(rows):
            ws = {determinize_row(cfg, row, -1, 5, 1, 4 * i + r)[1] for r in range(4)}
            assert len(ws) == 1 and ((0 in ws) == (seat_view(cfg, row, -1)[0] is None))
    for cfg, row in played_states():
        assert not weights_vary(enumerate_hands(cfg, row, -1))


def test_enumeration_agrees_with_brute_force_over_physical_cards():
    """enumerate_hands walks card types with multiplicities; on the small states the same three numbers come from the plain
    walk over physical pool elements."""
    for cfg, row in small_states() + crossed_states():
        _, _, know, pool, n_hand, _ = seat_view(cfg, row, -1)
        brute = {}

        def walk(s, taken, hand, weight):
            if s == n_hand:
                t, s2, p = brute.get(hand, (0, 0, 0.0))
                brute[hand] = (t + 1, s2 + weight, p + 1 / weight)
                return
            cand = [l for l in range(len(pool)) if l not in taken and plausible(cfg, know, s, pool[l])]
            for l in cand:
                walk(s + 1, taken | {l}, hand + (pool[l],), weight * len(cand))

        walk(0, frozenset(), (), 1)
        exact = enumerate_hands(cfg, row, -1)
        assert set(brute) == set(exact)
        for h in brute:
            assert brute[h][:2] == exact[h][:2] and abs(brute[h][2] - exact[h][2]) < 1e-12
        assert sum(p for _, _, p in exact.values()) < 1 + 1e-12   # (below 1: the walk can die on a crossed state)


def test_importance_weights_are_unbiased_by_exact_enumeration():
    """The unnormalised estimator mean(w * [hand == h]) against the exact number of consistent assignments T(h), within 6 sigma
    of its exact standard deviation (derived from the enumeration and N, not tuned), for every hand of every state; the variant
    whose weights are all 1 misses that bound.

    On the states reached by play the weights are constant (crossed_states' docstring), so there the all-ones variant is wrong
    only by that constant; the crossed states are where a weight-blind sampler cannot be right whatever constant it uses: there
    the variant is given the best constant there is (the total number of assignments) and must still miss the bound."""
    ones_fail = 0
    for cfg, row in played_states():
        exact = enumerate_hands(cfg, row, -1)
        means = _sample_means(cfg, row, N_SAMPLES, unit_weights=False)
        assert set(means) <= set(exact), "a sampled hand is not a consistent assignment"
        bad = _violations(exact, means, N_SAMPLES)
        assert not bad, f"importance-sampling estimate off by more than 6 sigma: {bad}"
        ones = _sample_means(cfg, row, N_SAMPLES, unit_weights=True)
        ones_fail += bool(_violations(exact, ones, N_SAMPLES, scale=1.0, wrong=True))
    assert ones_fail >= 1, "weights all 1 pass on every state: the states do not exercise the weights"
    crossed = crossed_states()
    assert len(crossed) >= 3
    for cfg, row in crossed:
        exact = enumerate_hands(cfg, row, -1)
        means = _sample_means(cfg, row, N_SAMPLES, unit_weights=False)
        assert set(means) <= set(exact)
        bad = _violations(exact, means, N_SAMPLES)
        assert not bad, f"importance-sampling estimate off by more than 6 sigma: {bad}"
        total = sum(t for t, _, _ in exact.values())
        blind = _sample_means(cfg, row, N_SAMPLES, unit_weights=True)
        assert _violations(exact, blind, N_SAMPLES, scale=total, wrong=True), "a weight-blind sampler passes on a crossed state"


@pytest.mark.parametrize("game,players", [("Hanabi-Full", 2), ("Hanabi-Full", 5)])
def test_restatement_invariants_on_random_play(game, players):
    cfg, rows = random_play_rows(game, players, 48, seed=5, turns=12)
    P, D = cfg.players, deck_size_of(cfg)
    n_live = n_dead = n_over = 0
    for i, row in enumerate(rows):
        for seat in (-1, (i % P)):
            for r in range(3):
                out, w, ns = determinize_row(cfg, row, seat, 7, 2, 3 * i + r)
                st, hand, know, pool, n_hand, deck_pos = seat_view(cfg, row, seat)
                if st is None:
                    n_over += 1
                    assert w == 0 and np.array_equal(out, row)
                    continue
                assert (w == 0) == (0 in ns), "dead exactly where some n_s is 0"
                if w == 0:
                    n_dead += 1
                    assert np.array_equal(out, row)
                    continue
                n_live += 1
                assert w == math.prod(ns) and len(ns) == n_hand
                # only the seat's hand word and the undealt deck bytes may differ
                same = np.ones(len(row), bool)
                same[10 + st] = False
                assert np.array_equal(out[:10 + 3 * P][same[:10 + 3 * P]], row[:10 + 3 * P][same[:10 + 3 * P]])
                db, da = row[10 + 3 * P:].view(np.uint8), out[10 + 3 * P:].view(np.uint8)
                assert np.array_equal(db[:deck_pos], da[:deck_pos]) and np.array_equal(db[D:], da[D:])
                st2, hand2, know2, pool2, n_hand2, deck_pos2 = seat_view(cfg, out, seat)
                assert (st2, know2, n_hand2, deck_pos2) == (st, know, n_hand, deck_pos)
                assert sorted(pool2) == sorted(pool), "the cards of hand + undealt deck are conserved"
                assert (hand2 >> (5 * n_hand)) == (hand >> (5 * n_hand))
                assert all(plausible(cfg, know, s, pool2[s]) for s in range(n_hand))
    assert n_live > 50
    assert n_dead == 0   # (states reached by play: crossed_states' docstring)


def test_restatement_is_keyed_by_row_id_only():
    cfg, rows = random_play_rows("Hanabi-Full", 2, 6, seed=3, turns=20)
    a, wa = determinize_ref(cfg, rows, -1, 4, 9, 5, first_row_id=0)
    b, wb = determinize_ref(cfg, rows[3:], -1, 4, 9, 5, first_row_id=12)
    assert np.array_equal(a[12:], b) and np.array_equal(wa[12:], wb)
    c, _ = determinize_ref(cfg, rows, -1, 4, 9, 6)
    assert not np.array_equal(a, c)
