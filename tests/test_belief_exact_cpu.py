"""The exact, enumerated belief without a GPU (include/hanabi_hip_exact.h, hanabi_hip/exact.py, hanabi_hip.belief_ref):
declarations and argument checks, and `belief_enumerate_ref` — what tests/test_belief_exact_gpu.py holds the kernel to — held to
an independent brute-force model, to its own identities, to the CPU rule oracle on games that rule-list teams really played, and
to hand-worked roots."""
import ctypes as C
import os

import numpy as np
import pytest

import exact_util as XU
from oracle import oracle_py as O

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def _ref(cfg, rows, seat, hist=None, move_fn=None, max_hands=1 << 20, replicas=4, seed=5, draw=3, first_row_id=0, details=True):
    from hanabi_hip import belief_enumerate_ref

    h = hist or {}
    return belief_enumerate_ref(cfg, rows, seat, h.get("rows"), h.get("moves"), h.get("alive"), h.get("valid"), h.get("draws"),
                                move_fn, max_hands, replicas, seed, draw, first_row_id, details=details)


def _no_moves(*a):
    raise AssertionError("D = 0 walks no rule")


# ---- declarations ------------------------------------------------------------------------------------------------------------------------
def test_the_entry_is_declared_in_its_own_header_exported_and_bound():
    import hanabi_hip
    from hanabi_hip import _capi, exact

    for name in ("belief_enumerate", "belief_enumerate_ref", "exact_rows", "exact_supported", "ExactBelief", "ExactDeterminizer"):
        assert hasattr(hanabi_hip, name) and name in hanabi_hip.__all__
    own = open(os.path.join(ROOT, "include", "hanabi_hip_exact.h")).read()
    assert "int hb_belief_enumerate(const hb_config* cfg" in own and "int64_t hb_belief_enumerate_scratch(const hb_config* cfg" in own
    assert '#include "hanabi_hip.h"' in own
    pinned = open(os.path.join(ROOT, "include", "hanabi_hip.h")).read()
    assert "hb_belief_enumerate" not in pinned and "#define HB_ABI_VERSION 1" in pinned
    assert not any("enumerate" in k for k in _capi.SIGNATURES)
    import kernel_bounds_cases

    assert "hb_belief_enumerate" not in open(kernel_bounds_cases.__file__).read()
    L = hanabi_hip.lib()
    assert L.hb_belief_enumerate and L.hb_belief_enumerate_scratch and L.hb_abi_version() == 1
    f, s = exact._fn()
    assert len(f.argtypes) == 30 and f.restype is C.c_int and s.restype is C.c_int64
    mk = open(os.path.join(ROOT, "hanabi-agents_amd", "csrc", "Makefile")).read()
    assert "belief_exact.hip" in mk and "hanabi_hip_exact.h" in mk


def test_scratch_size_is_the_documented_function():
    import hanabi_hip
    from hanabi_hip import exact

    full, small = hanabi_hip.make_config("Hanabi-Full", 2), hanabi_hip.make_config("Hanabi-Small", 2)
    assert exact.scratch_bytes(full, 3, 1000) == 3 * (1000 + 8 * 1)
    assert exact.scratch_bytes(full, 3, 1025) == 3 * (1025 + 8 * 2)
    assert exact.scratch_bytes(full, 1, 1 << 40) == 25 ** 5 + 8 * ((25 ** 5 + 1023) // 1024)   # no root has more hands than NC^H
    assert exact.scratch_bytes(small, 2, 1 << 40) == 2 * (100 + 8)
    assert exact.scratch_bytes(full, 0, 5) == 0
    for m, mh in ((-1, 5), (1, 0)):
        with pytest.raises(ValueError):
            exact.scratch_bytes(full, m, mh)


# ---- argument checks, with fake pointers ---------------------------------------------------------------------------------------------
def test_argument_validation_needs_no_gpu():
    import hanabi_hip
    from hanabi_hip import _capi as K, exact

    L = hanabi_hip.lib()
    f = exact._fn()[0]
    cfg = hanabi_hip.make_config("Hanabi-Full", 2)
    one, odd = C.c_void_p(64), C.c_void_p(68)
    err = lambda: L.hb_last_error()
    tab = (K.HbRule * 2)()
    tabs = (C.POINTER(K.HbRule) * 2)(C.cast(tab, C.POINTER(K.HbRule)), C.cast(tab, C.POINTER(K.HbRule)))
    lens = (C.c_int32 * 2)(2, 0)
    draws = (C.c_uint64 * 8)()

    def call(cfg_ref=C.byref(cfg), cur=one, m=4, seat=0, hist=(one, one, one, one), depth=2, dr=draws, rules=tabs, n_rules=lens,
             max_hands=100, R=3, outs=None, scratch=one):
        o = [one] * 9 if outs is None else outs
        return f(cfg_ref, cur, m, seat, hist[0], hist[1], hist[2], hist[3], depth, dr, 1, 0, rules, n_rules, max_hands, R, 1, 1, 0,
                 *o, scratch, None)

    assert call(cfg_ref=None) == -1 and b"null config" in err()
    assert call(cur=None) == -1 and b"cur_rows_dev" in err()
    assert call(m=-1) == -1 and b"m must be" in err()
    for seat in (-1, 2):
        assert call(seat=seat) == -1 and b"seat" in err()
    for depth in (-1, 9):
        assert call(depth=depth) == -1 and b"depth" in err()
    for bad in (0, 1):   # hist_rows_dev and hist_moves_dev are required when depth > 0; alive and valid may be NULL
        h = [one] * 4
        h[bad] = None
        assert call(hist=h) == -1 and b"depth > 0" in err()
    assert call(dr=None) == -1 and b"depth > 0" in err()
    for R in (0, (1 << 20) + 1):
        assert call(R=R) == -1 and b"replicas" in err()
    assert call(max_hands=0) == -1 and b"max_hands" in err()
    assert call(rules=None) == -1 and b"rules" in err() and call(n_rules=None) == -1 and b"rules" in err()
    for n in (-1, 17):
        assert call(n_rules=(C.c_int32 * 2)(n, 0)) == -1 and b"n_rules" in err()
    assert call(rules=(C.POINTER(K.HbRule) * 2)(None, None)) == -1 and b"null rules" in err()
    tab[1].kind = 16
    assert call() == -1 and b"unknown kind" in err()
    tab[1].kind = -1
    assert call() == -1 and b"unknown kind" in err()
    tab[1].kind = 3
    for bad in range(9):
        o = [one] * 9
        o[bad] = None
        if bad == 7:   # marg0_dev may be NULL: the call gets as far as the device
            assert call(outs=o, m=0) == 0
        else:
            assert call(outs=o) == -1 and b"null argument" in err()
    assert call(scratch=None) == -1 and b"scratch" in err()
    assert call(scratch=odd) == -4 and b"aligned" in err()
    assert call(m=1 << 22, max_hands=1 << 40) == -1 and b"2^31" in err()   # m * ceil(25^5 / 1024) blocks
    assert call(m=1 << 12, R=1 << 20) == -1 and b"2^31" in err()
    bad_cfg = hanabi_hip.HbConfig(6, 5, 5, 5, 8, 3, 0)
    assert call(cfg_ref=C.byref(bad_cfg)) == -1 and b"players" in err()
    odd_cfg = hanabi_hip.HbConfig(2, 3, 5, 5, 8, 3, 0)   # a valid game no kernel is compiled for
    if L.hb_config_validate(C.byref(odd_cfg)) == 0:
        assert call(cfg_ref=C.byref(odd_cfg)) == -1 and b"no compiled kernel" in err()
    # no-ops and what may be NULL: m == 0; depth 0 reads no history pointer
    assert call(m=0) == 0 and call(m=0, hist=(one, one, None, None)) == 0
    assert call(m=0, depth=0, hist=(None,) * 4, dr=None) == 0
    import torch

    if not torch.cuda.is_available():   # everything passed: the device comes last
        assert call() == -2 and b"no HIP device" in err()


def test_python_arguments_and_switches_are_checked():
    import torch

    import hanabi_hip
    from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR
    from hanabi_hip import RolloutSearch, SearchPlayer, belief_enumerate, exact_rows, exact_supported

    piers, flawed = RulebasedAgent(PR.piers_rules), RulebasedAgent(PR.flawed_rules)

    class Dqn:
        def eval_moves(self, *a, **k):
            raise AssertionError("not called")

    assert exact_supported([piers, flawed], 2) and exact_supported((piers, piers), 2, epsilon=None, track=False, color_shuffle=False)
    assert not exact_supported([piers, Dqn()], 2) and not exact_supported([piers, piers, piers], 3)
    assert not exact_supported([piers, piers], 2, epsilon=0.1) and not exact_supported([piers, piers], 2, track=True)
    assert not exact_supported([piers, piers], 2, color_shuffle=True) and not exact_supported([piers], 2)
    with pytest.raises(TypeError, match="exact is a switch"):
        SearchPlayer([piers, piers], 0, condition=True, exact=1)
    with pytest.raises(ValueError, match="condition=True"):
        SearchPlayer([piers, piers], 0, exact=True)
    with pytest.raises(ValueError, match="max_hands"):
        SearchPlayer([piers, piers], 0, condition=True, exact=True, max_hands=0)
    with pytest.raises(TypeError, match="exact is a switch"):
        RolloutSearch(exact="yes")
    with pytest.raises(ValueError, match="max_hands"):
        RolloutSearch(exact=True, max_hands=0)
    sp = SearchPlayer([piers, piers], 0, condition=True, exact=True, max_hands=64, depth=2)
    assert sp.exact and sp.max_hands == 64 and sp.last_belief is None
    assert sp.depth_stats() == dict(reached=[0, 0], survivors=[0, 0], used=[0, 0], shallow=[0, 0], exact_roots=0, too_large_roots=0,
                                    exact_hands=0)
    off = SearchPlayer([piers, piers], 0, condition=True)
    assert off.exact is False and "exact_roots" not in off.depth_stats()
    rs = RolloutSearch(exact=True)
    assert rs.exact and rs.max_hands == hanabi_hip.exact.DEFAULT_MAX_HANDS and RolloutSearch().exact is False
    cfg = hanabi_hip.make_config("Hanabi-Full", 2)
    rows = torch.zeros((3, 32), dtype=torch.int32)
    with pytest.raises(ValueError, match="one agent per seat"):
        belief_enumerate(cfg, rows, None, [piers], 0, 4, 1, 1)
    with pytest.raises(TypeError, match="RulebasedAgent"):
        belief_enumerate(cfg, rows, None, [piers, Dqn()], 0, 4, 1, 1)
    with pytest.raises(ValueError, match="rows"):
        belief_enumerate(cfg, rows[:, :31], None, [piers, piers], 0, 4, 1, 1)
    with pytest.raises(ValueError, match="seat"):
        belief_enumerate(cfg, rows, None, [piers, piers], 2, 4, 1, 1)
    with pytest.raises(ValueError, match="replicas"):
        belief_enumerate(cfg, rows, None, [piers, piers], 0, 0, 1, 1)
    with pytest.raises(ValueError, match="max_hands"):
        belief_enumerate(cfg, rows, None, [piers, piers], 0, 4, 1, 1, max_hands=0)
    with pytest.raises(TypeError, match="history"):
        belief_enumerate(cfg, rows, (rows, 1, 1, 0), [piers, piers], 0, 4, 1, 1)
    with pytest.raises(hanabi_hip.HbError, match="GPU"):
        belief_enumerate(cfg, rows, None, [piers, piers], 0, 4, 1, 1)
    with pytest.raises(ValueError, match="hands"):
        exact_rows(cfg, rows, torch.zeros((2, 4), dtype=torch.int32), 0, 1, 1)
    with pytest.raises(ValueError, match="seat"):
        exact_rows(cfg, rows, torch.zeros((3, 4), dtype=torch.int32), 2, 1, 1)


# ---- the reference against an independent model --------------------------------------------------------------------------------------
@pytest.mark.parametrize("game", ["Hanabi-Very-Small", "Hanabi-Small"])
def test_mass_and_marg0_are_counts_of_physical_arrangements(game):
    cfg, rows, seats = XU.late_rows(game)
    assert len(rows) >= 3
    seen_dupe = False
    for row, seat in zip(rows, seats):
        ref = _ref(cfg, row[None], seat, move_fn=_no_moves)
        hands, slots, per_pick = XU.brute_force(cfg, row, seat)
        assert ref["status"][0] == 0 and ref["fallback"][0] == 2 and ref["depth_used"][0] == 0
        mine = {cards: mass for cards, mass, _ in ref["details"][0] if mass > 0}
        assert {h: c for h, c in hands.items()} == {h: mass * per_pick for h, mass in mine.items()}
        assert np.array_equal(ref["marg0"][0] * per_pick, slots) and np.array_equal(ref["marg"][0], ref["marg0"][0])
        assert ref["mass"][0, 0] * per_pick == sum(hands.values()) and ref["n_hands"][0, 0] == len(hands)
        assert ref["space"][0] == len(ref["details"][0]) >= len(hands)
        seen_dupe = seen_dupe or any(mass > 1 for mass in mine.values()) or len(mine) < ref["space"][0]
    assert seen_dupe, "no row where two copies of a card, or two slots competing for one, make mass differ from 1"


@pytest.fixture(scope="module")
def full2p_ref():
    cfg, rows = XU.full2p()
    return cfg, rows, _ref(cfg, rows, 0, move_fn=_no_moves, max_hands=XU.FULL2P_MAX_HANDS, replicas=8)


def test_the_full_fixture_has_both_enumerated_and_too_large_roots(full2p_ref):
    cfg, rows, ref = full2p_ref
    m = len(rows)
    assert 2 * int((ref["status"] == 0).sum()) >= m and int((ref["status"] == 1).sum()) >= 1 and int((ref["status"] == 2).sum()) >= 1
    big = ref["status"] == 1
    assert (ref["space"][big] > XU.FULL2P_MAX_HANDS).all() and (ref["space"][ref["status"] == 0] <= XU.FULL2P_MAX_HANDS).all()
    for k in ("mass", "n_hands"):
        assert not ref[k][:, ref["status"] != 0].any()
    for k in ("marg", "marg0", "depth_used", "fallback"):
        assert not ref[k][ref["status"] != 0].any()
    assert np.array_equal(ref["hands"][ref["status"] != 0], np.repeat(rows[ref["status"] != 0, 10:11], 8, axis=1))
    assert (ref["space"][ref["status"] == 2] == 0).all()
    assert (ref["mass"][0, ref["status"] == 0] > 0).all(), "a row reached by play has a hand"


def _identities(cfg, rows, seat, ref):
    H = cfg.hand_size
    for i in np.flatnonzero(ref["status"] == 0):
        n = min(XU.hand_n(rows[i], seat), H)
        used = int(ref["depth_used"][i])
        assert (ref["marg"][i, :n].sum(1) == ref["mass"][used, i]).all() and not ref["marg"][i, n:].any()
        assert (ref["marg0"][i, :n].sum(1) == ref["mass"][0, i]).all() and not ref["marg0"][i, n:].any()
        assert (np.diff(ref["mass"][:, i]) <= 0).all() and (np.diff(ref["n_hands"][:, i]) <= 0).all()
        assert (ref["marg"][i] <= ref["marg0"][i]).all()


def test_identities_on_the_full_fixture(full2p_ref):
    cfg, rows, ref = full2p_ref
    _identities(cfg, rows, 0, ref)


# ---- the invariant that makes the filter exact: the true hand reproduces every move -----------------------------------------------------
@pytest.mark.parametrize("game,team,plies", [("Hanabi-Small", "piers", (3, 6, 11)), ("Hanabi-Small", "mixed", (4, 9)),
                                             ("Hanabi-Very-Small", "piers", (3, 8, 12)), ("Hanabi-Small", "everything", (3, 8))])
def test_the_true_hand_passes_every_entry_on_games_the_team_played(game, team, plies):
    G = XU.rule_games(game, 2, team, 6)
    checked = filtered = 0
    for t in plies:
        if t >= G.moves.shape[0]:
            continue
        games = [g for g in range(6) if XU.running(G.rows[t][g])]
        if not games:
            continue
        h = XU.history_at(G, t, 3, games)
        seat = h["seat"]
        ref = _ref(G.cfg, h["cur"], seat, h, XU.oracle_move_fn(G, games, seat))
        _identities(G.cfg, h["cur"], seat, ref)
        for i in range(len(games)):
            assert ref["status"][i] == 0
            L = int(np.cumprod(h["valid"][:, i]).sum())
            n = XU.hand_n(h["cur"][i], seat)
            truth = tuple(XU.hand_cards(h["cur"][i], seat, n))
            by_hand = {cards: (mass, passed) for cards, mass, passed in ref["details"][i]}
            assert by_hand[truth][0] > 0 and by_hand[truth][1] == L, (t, games[i], by_hand[truth], L)
            assert ref["depth_used"][i] == L and ref["fallback"][i] == (2 if L == 0 else 0)
            assert all(ref["marg"][i, s, truth[s]] > 0 for s in range(n))
            checked += 1
            filtered += int(ref["n_hands"][L, i] < ref["n_hands"][0, i])
    assert checked >= 6 and filtered >= 1, "no root where the partner's moves rule a hand out"


# ---- crafted roots ------------------------------------------------------------------------------------------------------------------
def _small_root():
    """A Small 2-player game of Piers at ply 4, game 0, seen by the seat to act, with its one-entry history."""
    G = XU.rule_games("Hanabi-Small", 2, "piers", 6)
    return G, XU.history_at(G, 4, 1, [0])


def test_a_move_no_hand_reproduces_falls_back_to_level_0():
    G, h = _small_root()
    never = lambda rows, movers, draw, root: np.full(len(rows), -7, np.int32)
    ref = _ref(G.cfg, h["cur"], h["seat"], h, never)
    assert ref["status"][0] == 0 and ref["fallback"][0] == 1 and ref["depth_used"][0] == 0
    assert ref["mass"][1, 0] == 0 and ref["n_hands"][1, 0] == 0 and ref["mass"][0, 0] > 0
    assert np.array_equal(ref["marg"], ref["marg0"])
    free = _ref(G.cfg, h["cur"], h["seat"], move_fn=_no_moves)
    assert np.array_equal(ref["hands"], free["hands"]) and np.array_equal(ref["marg"], free["marg"])


def test_an_invalid_entry_cuts_the_chain_and_a_finished_root_is_not_scored():
    G = XU.rule_games("Hanabi-Small", 2, "piers", 6)
    h = XU.history_at(G, 6, 3, [0, 1])
    h["valid"][1, 0] = 0
    calls = []

    def always(rows, movers, draw, root):
        calls.append((int(draw), sorted(set(int(r) for r in root))))
        return np.array([h["moves"][h["draws"].index(int(draw)), int(r)] for r in root], np.int32)

    cur = h["cur"].copy()
    ref = _ref(G.cfg, cur, h["seat"], h, always)
    assert ref["depth_used"].tolist() == [1, 3] and ref["fallback"].tolist() == [0, 0]
    assert [c[1] for c in calls] == [[0, 1], [1], [1]], "entries behind an invalid one are never walked"
    assert ref["mass"][2:, 0].tolist() == [0, 0] and (ref["mass"][:, 1] == ref["mass"][0, 1]).all()
    cur[1, 0] |= 1 << 19
    done = _ref(G.cfg, cur, h["seat"], h, always)
    assert done["status"].tolist() == [0, 2] and done["space"][1] == 0 and not done["marg"][1].any()
    assert (done["hands"][1] == cur[1, 10 + h["seat"]]).all()


def test_the_drawn_hands_follow_the_prefix_sum_rule_on_a_hand_worked_root():
    """Very-Small, 2 players: one colour, ranks 0..4 with 3/2/2/2/1 copies, hands of 2. The root is built by hand: seat 0 holds
    (card 0, card 1), the undealt deck is (0, 2), no hints. cnt = [2, 1, 1]; the 9 hands in enumeration order (slot 0 the fast
    digit) and their masses: (0,0) 2, (1,0) 2, (2,0) 2, (0,1) 2, (1,1) 0, (2,1) 1, (0,2) 2, (1,2) 1, (2,2) 0; T = 12."""
    from hanabi_hip.belief_ref import _philox_np

    cfg = O.make_config("Hanabi-Very-Small", 2, 0)
    assert (cfg.colors, cfg.ranks, cfg.hand_size) == (1, 5, 2) and XU.deck_size(cfg) == 10
    row = np.zeros(32, np.uint32)
    row[0] = 2 | (3 << 6) | (1 << 10)            # two cards to draw, 3 hints, 1 life, seat 0 to act, running
    row[1] = (2 << 15) | (2 << 18)               # both hands hold two cards
    row[10] = 0 | (1 << 5) | (0x7FFF << 10) | (5 << 25)    # (card 0, card 1), empty slots 31, and bits above the fields
    row[11] = 3 | (4 << 5) | (0x7FFF << 10)
    all_plausible = 1 | (31 << 5)
    row[12] = row[14] = all_plausible | (all_plausible << 12)
    deck = np.zeros(20, np.uint8)
    deck[:10] = [0, 1, 3, 4, 0, 1, 2, 3, 0, 2]   # the last two positions are undealt
    row[16:21] = deck.view("<u4")
    R, seed, draw, rid = 64, 11, 7, 40
    ref = _ref(cfg, row[None], 0, move_fn=_no_moves, replicas=R, seed=seed, draw=draw, first_row_id=rid)
    want = [((0, 0), 2), ((1, 0), 2), ((2, 0), 2), ((0, 1), 2), ((1, 1), 0), ((2, 1), 1), ((0, 2), 2), ((1, 2), 1), ((2, 2), 0)]
    assert [(c, mass) for c, mass, _ in ref["details"][0]] == want and ref["mass"][0, 0] == 12 and ref["n_hands"][0, 0] == 7
    assert ref["marg"][0, 0, :3].tolist() == [6, 3, 3] and ref["marg"][0, 1, :3].tolist() == [6, 3, 3]
    x = _philox_np(0x10000 + np.arange(R, dtype=np.uint64), draw, rid, 0, seed, 0)
    prefix = np.cumsum([mass for _, mass in want])
    got = set()
    for r in range(R):
        target = (((int(x[0][r]) << 32) | int(x[1][r])) * 12) >> 64
        cards = want[int(np.searchsorted(prefix, target, side="right"))][0]
        assert int(ref["hands"][0, r]) == cards[0] | (cards[1] << 5) | (0x7FFF << 10) | (5 << 25), r
        got.add(cards)
    assert len(got) >= 5 and (1, 1) not in got and (2, 2) not in got
    again = _ref(cfg, row[None], 0, move_fn=_no_moves, replicas=R, seed=seed, draw=draw, first_row_id=rid + 1)
    assert not np.array_equal(again["hands"], ref["hands"])


def test_root_over_max_hands_is_reported_not_filled():
    cfg, rows, seats = XU.late_rows("Hanabi-Small")
    ref = _ref(cfg, rows[:1], seats[0], move_fn=_no_moves)
    N = int(ref["space"][0])
    assert N >= 2
    cut = _ref(cfg, rows[:1], seats[0], move_fn=_no_moves, max_hands=N - 1)
    assert cut["status"][0] == 1 and cut["space"][0] == N and not cut["mass"].any() and not cut["marg"].any()
    assert cut["details"][0] is None and (cut["hands"][0] == rows[0, 10 + seats[0]]).all()
    same = _ref(cfg, rows[:1], seats[0], move_fn=_no_moves, max_hands=N)
    assert same["status"][0] == 0 and np.array_equal(same["marg"], ref["marg"])
