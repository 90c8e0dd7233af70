"""hb_belief_enumerate on the GPU (include/hanabi_hip_exact.h, csrc/belief_exact.hip, hanabi_hip/exact.py): every output against
`belief_enumerate_ref` (itself held to independent models in tests/test_belief_exact_cpu.py), exact equality throughout; guard
bands; the independence of the grid; `exact_rows`; today's conditioned sampler as a cross-check; the `SearchPlayer` switch.

The reference's `move_fn` here is the EXISTING hb_rule_act_grouped on the hypothetical rows (one block per row, so that every row
of a root is keyed by the root's game id): "what hb_rule_act returns on the spliced slab". tests/test_belief_exact_cpu.py holds
the same reference to the CPU rule oracle."""
import ctypes as C

import numpy as np
import pytest

import exact_util as XU
import guard_util as GU

pytestmark = pytest.mark.gpu

OUTS = ("status", "space", "mass", "n_hands", "depth_used", "fallback", "marg", "marg0", "hands")


def _cfg(c):
    """The oracle's configuration as the library's own struct."""
    from hanabi_hip import HbConfig

    return HbConfig(c.players, c.colors, c.ranks, c.hand_size, c.max_info, c.max_life, 0)


def _team(name, players):
    from hanabi_agents.rule_based import RulebasedAgent
    from playout_util import teams

    return [RulebasedAgent(r) for r in teams()[name](players)]


def _gpu_move_fn(cfg, team, partner_seed, first_game_id):
    import torch

    from hanabi_hip import _capi as K
    from hanabi_hip.grouped import RuleSets

    sets = RuleSets(team).upload("cuda")
    L = K.lib()

    def fn(rows, movers, draw, root):
        dev_rows = torch.from_numpy(np.ascontiguousarray(rows).view(np.int32)).cuda()
        out = torch.empty(len(rows), dtype=torch.int32, device="cuda")
        root, movers = np.asarray(root), np.asarray(movers)
        for i in np.unique(root):
            idx = np.flatnonzero(root == i)
            assert (movers[idx] == movers[idx[0]]).all()
            sub = dev_rows[torch.from_numpy(idx).cuda()].contiguous()
            which = torch.full((len(idx),), int(movers[idx[0]]), dtype=torch.int32, device="cuda")
            act = torch.empty(len(idx), dtype=torch.int32, device="cuda")
            K.check(L.hb_rule_act_grouped(C.byref(cfg), K.dptr(sub), len(idx), 1, int(first_game_id) + int(i), K.dptr(which),
                                          K.dptr(sets.table_dev), K.dptr(sets.n_rules_dev), len(sets), int(partner_seed), int(draw),
                                          K.dptr(act), None, K.current_stream()))
            out[torch.from_numpy(idx).cuda()] = act
        return out.cpu().numpy()

    return fn


def _history(cfg, hist, m, partner_seed, first_game_id, null_alive=False, null_valid=False):
    """exact_util's history arrays as the PartnerHistory the wrapper takes (None: no history)."""
    import torch

    from hanabi_hip import PartnerHistory

    if hist is None:
        return None
    D = hist["rows"].shape[0]
    ph = PartnerHistory(cfg, m, D, "cuda", partner_seed=partner_seed, first_game_id=first_game_id)
    ph.prev_rows = torch.from_numpy(hist["rows"].view(np.int32)).cuda()
    ph.moves = torch.from_numpy(hist["moves"]).cuda()
    ph.alive = None if null_alive else torch.from_numpy(hist["alive"]).cuda()
    ph.valid = None if null_valid else torch.from_numpy(hist["valid"]).cuda()
    ph.draws, ph.filled = list(hist["draws"]), D
    return ph


def _kernel(cfg, cur, seat, hist, team, R, seed=5, draw=3, partner_seed=XU.DEAL_SEED, first_game_id=0, first_row_id=0,
            max_hands=1 << 12, out=None, **nulls):
    import torch

    from hanabi_hip import belief_enumerate

    rows = torch.from_numpy(np.array(cur, dtype=np.uint32).view(np.int32)).cuda()
    return belief_enumerate(cfg, rows, _history(cfg, hist, len(cur), partner_seed, first_game_id, **nulls), team, seat, R, seed, draw,
                            partner_seed=partner_seed, first_game_id=first_game_id, first_row_id=first_row_id, max_hands=max_hands,
                            marg0=True, out=out)


def _reference(cfg, cur, seat, hist, team, R, seed=5, draw=3, partner_seed=XU.DEAL_SEED, first_game_id=0, first_row_id=0,
               max_hands=1 << 12, null_alive=False, null_valid=False):
    from hanabi_hip import belief_enumerate_ref

    h = hist or {}
    return belief_enumerate_ref(cfg, cur, seat, h.get("rows"), h.get("moves"), None if null_alive else h.get("alive"),
                                None if null_valid else h.get("valid"), h.get("draws"),
                                _gpu_move_fn(cfg, team, partner_seed, first_game_id), max_hands, R, seed, draw, first_row_id)


def _same(belief, ref, where=""):
    import torch

    torch.cuda.synchronize()
    for name in OUTS:
        got = getattr(belief, name).cpu().numpy()
        want = ref[name]
        if name == "hands":
            got = got.view(np.uint32)
        assert got.dtype == want.dtype and got.shape == want.shape, (where, name, got.dtype, want.dtype, got.shape, want.shape)
        assert np.array_equal(got, want), (where, name, np.argwhere(got != want)[:4].tolist())


def _slice(hist, sl):
    return None if hist is None else dict(hist, rows=hist["rows"][:, sl].copy(), moves=hist["moves"][:, sl].copy(),
                                          alive=hist["alive"][:, sl].copy(), valid=hist["valid"][:, sl].copy())


# ---- games the team really played: the history is the real one --------------------------------------------------------------------------
PLAYED = [  # game, players, team, ply, depth, replicas
    ("Hanabi-Very-Small", 2, "piers", 7, 8, 32),
    ("Hanabi-Very-Small", 2, "flawed", 1, 1, 32),
    ("Hanabi-Small", 2, "piers", 12, 2, 100),
    ("Hanabi-Small", 2, "mixed", 9, 1, 1),
    ("Hanabi-Small", 3, "mixed", 10, 8, 32),
    ("Hanabi-Small", 2, "everything", 8, 0, 32),
]


@pytest.mark.parametrize("game,players,team,ply,depth,R", PLAYED)
def test_kernel_is_the_reference_on_played_games(game, players, team, ply, depth, R):
    G = XU.rule_games(game, players, team, 65)
    hist = XU.history_at(G, ply, depth) if depth else None
    cur, seat = G.rows[ply].copy(), ply % players
    assert XU.running(cur).any()
    agents, cfg = _team(team, players), _cfg(G.cfg)
    for sl in (slice(0, 65), slice(7, 10), slice(64, 65)):   # m = 65, 3, 1 (the last two keep their game ids)
        first = sl.start
        ref = _reference(cfg, cur[sl], seat, _slice(hist, sl), agents, R, first_game_id=first, first_row_id=first)
        got = _kernel(cfg, cur[sl], seat, _slice(hist, sl), agents, R, first_game_id=first, first_row_id=first)
        _same(got, ref, (game, team, sl))
        if sl.stop - sl.start == 65 and depth:
            live = ref["status"] == 0
            L = np.cumprod(hist["valid"], axis=0).sum(0)
            assert (ref["depth_used"][live] == L[live]).all(), "the true hand reproduces every move of a game the team played"
            if team != "flawed":
                assert (ref["n_hands"][1, live] < ref["n_hands"][0, live]).any(), "no root where the move rules a hand out"


# ---- crafted histories on deep rows: dead slots, invalid entries, finished roots, roots over max_hands -----------------------------
def _crafted(game, players, seat, depth, seed):
    """The picked deep rows of a variant seen by `seat`, with a history made of OTHER deep rows (every entry some running row of
    the corpus whose hand for `seat` may be shorter or longer), the move the mover's list makes on that row as it is, random
    alive masks and a tenth of the entries invalid."""
    import torch

    import deep_rows as DR
    from hanabi_hip import _capi as K
    from oracle import oracle_py as O

    cfg = _cfg(O.make_config(game, players, 0))
    cur = np.ascontiguousarray(DR.pick(game, players).rows)
    m = len(cur)
    rng = np.random.default_rng(seed)
    c = DR.corpus(game, players)
    pool = np.flatnonzero(c.running)
    hist = dict(rows=np.zeros((depth, m, cur.shape[1]), np.uint32), moves=np.zeros((depth, m), np.int32),
                alive=rng.integers(0, 32, (depth, m)).astype(np.uint8), valid=(rng.random((depth, m)) > 0.1).astype(np.uint8),
                draws=[int(x) for x in rng.integers(1, 60, depth)])
    team = _team("mixed", players)
    L = K.lib()
    for d in range(depth):
        hist["rows"][d] = c.rows[rng.choice(pool, m)]
        rows = torch.from_numpy(hist["rows"][d].view(np.int32)).cuda()
        acts = []
        for a in team:   # the move of every seat's list on the rows as they are; each row takes its mover's
            act = torch.empty(m, dtype=torch.int32, device="cuda")
            K.check(L.hb_rule_act(C.byref(cfg), K.dptr(rows), m, 100, a._tab, len(a.rules), 9, hist["draws"][d], K.dptr(act), None,
                                  K.current_stream()))
            acts.append(act.cpu().numpy())
        mover = (hist["rows"][d][:, 0] >> 13) & 7
        hist["moves"][d] = np.stack(acts)[mover, np.arange(m)]
    return cfg, cur, hist, team


def test_kernel_is_the_reference_on_the_full_fixture_with_a_crafted_history():
    cfg, cur, hist, team = _crafted("Hanabi-Full", 2, 0, 2, 1)
    assert np.array_equal(cur, XU.full2p()[1])
    kw = dict(partner_seed=9, first_game_id=100, max_hands=XU.FULL2P_MAX_HANDS)
    ref = _reference(cfg, cur, 0, hist, team, 32, **kw)
    m = len(cur)
    assert 2 * int((ref["status"] == 0).sum()) >= m and (ref["status"] == 1).any() and (ref["status"] == 2).any()
    assert (ref["depth_used"] == 2).any() and (ref["fallback"] == 1).any() and (ref["space"] > 1024).any()
    _same(_kernel(cfg, cur, 0, hist, team, 32, **kw), ref, "full")
    for nulls in (dict(null_alive=True), dict(null_valid=True)):
        _same(_kernel(cfg, cur[:9], 0, _slice(hist, slice(0, 9)), team, 4, **kw, **nulls),
              _reference(cfg, cur[:9], 0, _slice(hist, slice(0, 9)), team, 4, **kw, **nulls), nulls)


def test_kernel_is_the_reference_on_small_deep_rows_at_depth_8():
    cfg, cur, hist, team = _crafted("Hanabi-Small", 3, 1, 8, 2)
    kw = dict(partner_seed=9, first_game_id=100, max_hands=64)
    ref = _reference(cfg, cur, 1, hist, team, 32, **kw)
    assert (ref["status"] == 1).any() and len(set(ref["depth_used"].tolist())) >= 3
    _same(_kernel(cfg, cur, 1, hist, team, 32, **kw), ref, "small3")


def test_kernel_is_the_reference_on_the_48_word_rows_of_full_5p_without_a_history():
    import deep_rows as DR
    from oracle import oracle_py as O

    cfg = _cfg(O.make_config("Hanabi-Full", 5, 0))
    cur = np.ascontiguousarray(DR.pick("Hanabi-Full", 5).rows)
    assert cur.shape[1] == 48
    team = _team("mixed", 5)
    ref = _reference(cfg, cur, 2, None, team, 32, max_hands=1 << 12)
    assert (ref["status"] == 0).any() and (ref["status"] == 1).any() and (ref["fallback"][ref["status"] == 0] == 2).all()
    _same(_kernel(cfg, cur, 2, None, team, 32, max_hands=1 << 12), ref, "full5")


# ---- guard bands; calls repeated and split ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 65])
def test_every_output_and_the_scratch_stay_inside_their_buffers(m):
    import torch

    from hanabi_hip import exact

    G = XU.rule_games("Hanabi-Small", 2, "piers", 65)
    hist, cur = _slice(XU.history_at(G, 12, 2), slice(0, m)), G.rows[12][:m].copy()
    team, R, D, max_hands, cfg = _team("piers", 2), 32, 2, 40, _cfg(G.cfg)
    H, NC = cfg.hand_size, cfg.colors * cfg.ranks
    plain = _kernel(cfg, cur, 0, hist, team, R, max_hands=max_hands)
    gs = GU.GuardSet("hb_belief_enumerate")
    specs = dict(status=((m,), "uint8"), space=((m,), "int64"), mass=((D + 1, m), "int64"), n_hands=((D + 1, m), "int32"),
                 depth_used=((m,), "int32"), fallback=((m,), "uint8"), marg=((m, H, NC), "int64"), marg0=((m, H, NC), "int64"),
                 hands=((m, R), "int32"), scratch=((exact.scratch_bytes(cfg, m, max_hands),), "uint8"))
    out = tuple(gs.out(name, shape, dtype, 1024) for name, (shape, dtype) in specs.items())
    got = _kernel(cfg, cur, 0, hist, team, R, max_hands=max_hands, out=out)
    torch.cuda.synchronize()
    gs.check(f"m = {m}")
    assert [n for n in gs.untouched() if n != "scratch"] == []
    for name in OUTS:
        assert GU.same_bits(getattr(got, name), getattr(plain, name)) == -1, name


def test_two_calls_and_a_split_call_give_the_same_bits():
    G = XU.rule_games("Hanabi-Small", 2, "piers", 65)
    hist, cur = XU.history_at(G, 12, 2), G.rows[12].copy()
    team, cfg = _team("piers", 2), _cfg(G.cfg)
    kw = dict(first_game_id=50, first_row_id=7000)
    whole, again = (_kernel(cfg, cur, 0, hist, team, 32, **kw) for _ in range(2))
    lo = _kernel(cfg, cur[:30], 0, _slice(hist, slice(0, 30)), team, 32, **kw)
    hi = _kernel(cfg, cur[30:], 0, _slice(hist, slice(30, 65)), team, 32, first_game_id=80, first_row_id=7030)
    import torch

    for name in OUTS:
        a = getattr(whole, name)
        assert GU.same_bits(a, getattr(again, name)) == -1, name
        both = torch.cat([getattr(lo, name), getattr(hi, name)], dim=1 if name in ("mass", "n_hands") else 0)
        assert GU.same_bits(a, both) == -1, name
    other = _kernel(cfg, cur, 0, hist, team, 32, first_game_id=50, first_row_id=7001)
    assert GU.same_bits(whole.marg, other.marg) == -1 and GU.same_bits(whole.hands, other.hands) != -1


# ---- exact_rows ---------------------------------------------------------------------------------------------------------------------
def test_exact_rows_are_the_drawn_hands_on_physically_consistent_rows():
    import torch

    from hanabi_hip import exact_rows

    G = XU.rule_games("Hanabi-Small", 2, "piers", 65)
    cfg, ply, R = _cfg(G.cfg), 12, 16
    cur, seat = G.rows[ply].copy(), ply % 2
    belief = _kernel(cfg, cur, seat, XU.history_at(G, ply, 2), _team("piers", 2), R)
    rows = torch.from_numpy(cur.view(np.int32)).cuda()
    det, w = exact_rows(cfg, rows, belief.hands, seat, seed=5, draw=3, first_row_id=11)
    det, w, hands = det.cpu().numpy().view(np.uint32), w.cpu().numpy(), belief.hands.cpu().numpy().view(np.uint32)
    live = XU.running(cur)
    assert live.sum() >= 32 and (w.reshape(65, R) == live[:, None]).all()
    D, W_DECK = XU.deck_size(cfg), 10 + 3 * 2
    changed = 0
    for i in range(65):
        for r in range(R):
            o = det[i * R + r]
            if not live[i]:
                assert np.array_equal(o, cur[i])
                continue
            assert o[10 + seat] == hands[i, r]
            same = np.ones(len(o), bool)
            same[10 + seat] = False
            same[W_DECK:] = False
            assert np.array_equal(o[same], cur[i][same])
            n, left = XU.hand_n(cur[i], seat), int(cur[i][0] & 63)
            a, b = XU.deck_bytes(cfg, o), XU.deck_bytes(cfg, cur[i])
            assert np.array_equal(a[:D - left], b[:D - left])
            assert sorted(XU.hand_cards(o, seat, n) + a[D - left:].tolist()) == sorted(XU.hand_cards(cur[i], seat, n) + b[D - left:].tolist())
            changed += int(o[10 + seat] != cur[i][10 + seat])
    assert changed > 0


# ---- today's sampled path as a cross-check ------------------------------------------------------------------------------------------
def test_a_survivor_of_the_conditioned_sampler_is_a_hand_that_passes():
    import torch

    from hanabi_hip import ConditionedDeterminizer, LastMove

    G = XU.rule_games("Hanabi-Small", 2, "piers", 65)
    cfg, ply, R, ov = _cfg(G.cfg), 12, 8, 4
    cur, seat = G.rows[ply].copy(), ply % 2
    hist = XU.history_at(G, ply, 1)
    team = _team("piers", 2)
    from hanabi_hip import belief_enumerate_ref

    ref = belief_enumerate_ref(cfg, cur, seat, hist["rows"], hist["moves"], hist["alive"], hist["valid"], hist["draws"],
                               _gpu_move_fn(cfg, team, XU.DEAL_SEED, 0), 1 << 12, R, 5, 3, 0, details=True)
    detail = ref["details"]
    rows = torch.from_numpy(cur.view(np.int32)).cuda()
    last = LastMove(torch.from_numpy(hist["rows"][0].view(np.int32)).cuda(), XU.DEAL_SEED, hist["draws"][0], 0,
                    torch.from_numpy(hist["valid"][0]).cuda(), m=65, words=cur.shape[1], device=rows.device)
    s = ConditionedDeterminizer(config=cfg).sample_history(rows, last, team[1 - seat], seat, R, ov, 5, 3, XU.DEAL_SEED, 0)
    det, w = s.rows.cpu().numpy().view(np.uint32), s.weights.cpu().numpy()
    used, fb = s.depth_used.cpu().numpy(), s.fallback.cpu().numpy()
    seen = 0
    for i in range(65):
        if ref["status"][i] != 0 or fb[i] != 0:
            continue
        assert used[i] == 1 and ref["depth_used"][i] == 1
        passed = {cards for cards, mass, p in detail[i] if mass > 0 and p >= 1}
        n = XU.hand_n(cur[i], seat)
        for r in range(R):
            if w[i * R + r]:
                assert tuple(XU.hand_cards(det[i * R + r], seat, n)) in passed, (i, r)
                seen += 1
    assert seen >= 100


# ---- the switch -------------------------------------------------------------------------------------------------------------------------
def test_search_player_with_the_exact_belief_plays_to_the_end_and_off_is_the_player_without_it():
    from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR
    from hanabi_hip import Evaluator, SearchPlayer

    piers = RulebasedAgent(PR.piers_rules)

    def play(**kw):
        sp = SearchPlayer([piers, piers], seat=0, condition=True, replicas=8, playout=True, **kw)
        res = Evaluator("Hanabi-Small", 2, n_games=64, seed=3).run([sp, piers])
        return sp, res

    sp, first = play(exact=True, max_hands=16)
    sp2, second = play(exact=True, max_hands=16)
    assert first.scores.tolist() == second.scores.tolist() and first.lengths.tolist() == second.lengths.tolist()
    stats = sp.depth_stats()
    assert stats == sp2.depth_stats() and sp.conditioned > 0
    assert stats["exact_roots"] + stats["too_large_roots"] == sp.conditioned
    assert stats["exact_roots"] > 0 and stats["too_large_roots"] > 0 and stats["exact_hands"] >= stats["exact_roots"]
    assert sp.last_belief in ("exact", "mixed")
    off, a = play(exact=False)
    plain, b = play()
    assert a.scores.tolist() == b.scores.tolist() and a.lengths.tolist() == b.lengths.tolist()
    assert off.deviations == plain.deviations and off.survivors == plain.survivors and off.last_belief == "sampled"
    assert "exact_roots" not in off.depth_stats()
