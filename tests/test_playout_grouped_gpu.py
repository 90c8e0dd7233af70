"""GPU: hb_rule_playout_grouped (many rule-list teams played to the end in one launch, one team per block of games) against the
CPU expectation of tests/playout_util.py and against hb_rule_playout on each block alone, CrossPlay(playout=True) against the
turn loop, and one RuleSearch run. Exact equality everywhere: every quantity is an integer or a copy of one."""
import ctypes as C

import numpy as np
import pytest

import playout_util as U
from guard_util import GuardSet

pytestmark = pytest.mark.gpu

SEED = U.DEAL_SEED
TEAMS = ["piers", "flawed", "mixed", "everything"]


def _cases():
    import test_playout_gpu as T

    return T.CASES[:6] + T.NEW_CASES + T.CASES[6:8]   # the twelve instantiations, then block_games 1 and 63 on Full 2p


def _agents(team, P):
    from hanabi_agents.rule_based import RulebasedAgent

    return tuple(RulebasedAgent(r, seed=50 + p) for p, r in enumerate(U.teams()[team](P)))


def _dev_rows(rows_u32):
    import torch

    return torch.from_numpy(np.ascontiguousarray(rows_u32).view(np.int32)).cuda()


def _np(t):
    return t.cpu().numpy()


def _assert_block(res, b, n, e):
    """Block b (n games) of a logged rule_playout_grouped against oracle_playout's figures of that block alone."""
    s = slice(b * n, (b + 1) * n)
    assert np.array_equal(_np(res.rows[s]).view(np.uint32), e["rows"]), b
    assert np.array_equal(_np(res.done[s]), e["done"]), b
    assert np.array_equal(_np(res.final_score[s]), e["final_score"]), b
    assert np.array_equal(_np(res.length[s]), e["length"]), b
    assert np.array_equal(_np(res.counters[b]), e["counters"]), b
    acts, want = _np(res.actions[:, s]), e["actions"]
    assert acts.shape == want.shape
    below = np.arange(acts.shape[0])[:, None] < e["length"].astype(np.int64)[None, :]
    assert np.array_equal(acts[below], want[below]), b
    assert (acts[~below] == -1).all(), b
    assert int(res.max_len[b]) == e["max_len"] and int(res.counters[b, 0]) == 0 == e["illegal"], b


def test_the_cases_launch_every_instantiation_with_a_block_edge_inside_a_wavefront():
    import deep_play

    cases = _cases()
    assert {(g, p) for g, p, _ in cases[:12]} == set(deep_play.VARIANTS) and len(deep_play.VARIANTS) == 12
    # four blocks of n games: a kernel that cut wavefronts across the whole array would straddle a block edge
    assert sum(1 for _, _, n in cases if n % 64) >= 13 and cases[12:] == [("Hanabi-Full", 2, 1), ("Hanabi-Full", 2, 63)]


@pytest.mark.parametrize("game,players,n", _cases())
def test_four_teams_in_one_launch_match_the_cpu_expectation(game, players, n):
    """piers / flawed / mixed / everything on the same deals (id_stride 0), one block each."""
    import torch

    import hanabi_hip

    exp = [U.expected(game, players, n, team) for team in TEAMS]
    cfg = hanabi_hip.make_config(game, players)
    rows = torch.cat([_dev_rows(e["rows0"]) for e in exp])
    res = hanabi_hip.rule_playout_grouped(cfg, rows, [_agents(team, players) for team in TEAMS], SEED, block_games=n, log=True)
    assert res.counters.shape == (4, len(exp[0]["counters"])) and res.max_len.shape == (4,)
    for b, e in enumerate(exp):
        _assert_block(res, b, n, e)
    assert int(res.illegal) == 0


@pytest.mark.parametrize("base", [0, 2 ** 32 - 200])
def test_distinct_games(base):
    """id_stride = block_games = 129: block b plays the games of ids base + 129 b .. ; from base 2^32 - 200 the ids cross 2^32
    at row 71 of block 1 (the id's high word is part of the rule walk's Philox key)."""
    import torch

    import hanabi_hip

    n, names = 129, ["mixed", "piers", "everything"]
    exp = [U.expected("Hanabi-Full", 2, n, team, first_game_id=base + n * b) for b, team in enumerate(names)]
    cfg = hanabi_hip.make_config("Hanabi-Full", 2)
    rows = torch.cat([_dev_rows(e["rows0"]) for e in exp])
    teams = [_agents(team, 2) for team in names]
    res = hanabi_hip.rule_playout_grouped(cfg, rows, teams, SEED, block_games=n, id_stride=n, first_game_id=base, log=True)
    for b, e in enumerate(exp):
        _assert_block(res, b, n, e)
    if base:   # on the same rows the moves depend on the ids: stride 0 plays blocks 1 and 2 otherwise
        same = hanabi_hip.rule_playout_grouped(cfg, torch.cat([_dev_rows(e["rows0"]) for e in exp]), teams, SEED, block_games=n,
                                               id_stride=0, first_game_id=base, log=True)
        assert torch.equal(same.actions[:, :n], res.actions[:, :n])
        assert not torch.equal(same.actions[:, n:2 * n], res.actions[:, n:2 * n])
        assert not torch.equal(same.actions[:, 2 * n:], res.actions[:, 2 * n:])


@pytest.mark.parametrize("variant", ["first_moves", "preset_done", "turn_cap", "first_seat"])
def test_every_block_equals_rule_playout_on_that_block(variant):
    """The single-team kernel (which tests/test_playout_gpu.py pins to the oracle) on each block's slices, with the options the
    oracle helper has no form of."""
    import torch

    import hanabi_hip

    n, names = 63, ["piers", "flawed", "mixed"]
    e = U.expected("Hanabi-Full", 2, n, "mixed")
    cfg = hanabi_hip.make_config("Hanabi-Full", 2)
    teams = [_agents(team, 2) for team in names]
    kw, first, done = {}, None, None
    if variant == "first_moves":   # another team's first moves on the same deals: legal, and not every team's own
        first = torch.from_numpy(np.tile(U.expected("Hanabi-Full", 2, n, "flawed")["actions"][0], 3).copy()).cuda()
        first[n:n + 5] = 0   # (and five that the env refuses — a discard with every hint token left: the illegal-move count)
    elif variant == "preset_done":
        done = torch.zeros(3 * n, dtype=torch.uint8, device="cuda")
        done[::3] = 0x80
        done[n + 7:n + 40] = 0x80
    elif variant == "turn_cap":
        kw["max_turns"] = 5
    else:
        kw["first_seat"] = 1
    rows = _dev_rows(np.tile(e["rows0"], (3, 1)))
    res = hanabi_hip.rule_playout_grouped(cfg, rows, teams, SEED, block_games=n, first_moves=first, done=done, log=True, **kw)
    illegal = 0
    for b, team in enumerate(teams):
        s = slice(b * n, (b + 1) * n)
        one = hanabi_hip.rule_playout(cfg, _dev_rows(e["rows0"]), team, SEED, first_moves=None if first is None else first[s].clone(),
                                      done=None if done is None else done[s].clone(), log=True, **kw)
        assert torch.equal(res.rows[s], one.rows) and torch.equal(res.done[s], one.done), b
        assert torch.equal(res.final_score[s], one.final_score) and torch.equal(res.length[s], one.length), b
        assert torch.equal(res.counters[b], one.counters) and torch.equal(res.actions[:, s], one.actions), b
        assert int(res.max_len[b]) == int(one.max_len), b
        illegal += int(one.illegal)
        if variant == "turn_cap":
            running = int((one.done < 0x80).sum())
            assert int(res.counters[b, 0]) == running and (0 < running if names[b] != "flawed" else True)
        if variant == "preset_done":
            skipped = _np(done[s]) >= 0x80
            assert np.array_equal(_np(res.rows[s]).view(np.uint32)[skipped], e["rows0"][skipped]) and skipped.sum() >= n // 3
    assert int(res.illegal) == illegal and illegal == (5 if variant == "first_moves" else 0)


@pytest.mark.parametrize("variant", ["log", "preset"])
@pytest.mark.parametrize("players", [2, 5])
@pytest.mark.parametrize("n", [1, 63, 65, 129])
def test_skipped_blocks_and_guard_bands(n, players, variant):
    """Four blocks, the second (index -1) and the last (index n_sets: not below it) skipped; every output of
    hb_rule_playout_grouped in a guarded buffer, every input registered. No guard byte and no input changes, and of a skipped
    block nothing is written but its log entries."""
    import torch

    import hanabi_hip
    from hanabi_hip import _capi as K, evaluate, playout
    from hanabi_hip.grouped import RuleSets

    game, nb = "Hanabi-Full", 4
    e = U.expected(game, players, n, "mixed")
    cfg = hanabi_hip.make_config(game, players)
    SW, NC, T = e["rows0"].shape[1], len(e["counters"]), evaluate.max_turns(cfg)
    team = _agents("mixed", players)
    sets = RuleSets(team).upload("cuda")
    index = [[sets.index(a) for a in team], [-1] * players, [sets.index(a) for a in team], [0] * (players - 1) + [len(sets)]]
    played_block = np.array([True, False, True, False])
    gs = GuardSet("hb_rule_playout_grouped")
    tile = 64   # one wavefront's games: the kernel's tile
    preset = variant == "preset"
    done0 = torch.zeros(nb * n, dtype=torch.uint8, device="cuda")
    first = None
    if preset:
        done0[::3] = 0x80                                   # slots that are not played
        first = gs.inp("first_moves", torch.from_numpy(np.tile(e["actions"][0], nb).copy()).cuda())   # the rule walk's own
    gs.inp("team_of_block", torch.tensor(index, dtype=torch.int32, device="cuda"))
    gs.inp("rules", sets.table_dev)
    gs.inp("n_rules", sets.n_rules_dev)
    rows0 = np.tile(e["rows0"], (nb, 1))
    rows = gs.out("rows", (nb * n, SW), torch.int32, tile * SW, init=_dev_rows(rows0))
    done = gs.out("done", (nb * n,), torch.uint8, 4 * tile, init=done0)
    fs = gs.out("final_score", (nb * n,), torch.int8, 4 * tile, init=torch.full((nb * n,), 77, dtype=torch.int8, device="cuda"))
    ln = gs.out("length", (nb * n,), torch.int16, 4 * tile, init=torch.full((nb * n,), 777, dtype=torch.int16, device="cuda"))
    c0 = torch.zeros(nb, NC, dtype=torch.int64, device="cuda")
    c0[:, 0] = (done0.view(nb, n) < 0x80).sum(1)
    c0[~torch.from_numpy(played_block).cuda()] = 123        # a skipped block's counter row is not the kernel's
    counters = gs.out("counters", (nb, NC), torch.int64, 64, init=c0)
    log = gs.out("log", (T, nb * n), torch.int32, 4 * tile)
    illegal = gs.out("illegal", (1,), torch.int64, 64, init=torch.zeros(1, dtype=torch.int64, device="cuda"))
    m0 = torch.tensor([0, 55, 0, 55], dtype=torch.int32, device="cuda")
    max_len = gs.out("max_len", (nb,), torch.int32, 64, init=m0)
    K.check(playout._fn_grouped()(C.byref(cfg), K.dptr(rows), nb, n, 0, 0, K.dptr(gs.inps["team_of_block"][0]), K.dptr(sets.table_dev),
                                  K.dptr(sets.n_rules_dev), len(sets), SEED, 0, K.dptr(first), T, K.dptr(done), K.dptr(fs), K.dptr(ln),
                                  K.dptr(counters), K.dptr(log), K.dptr(illegal), K.dptr(max_len), K.current_stream()))
    torch.cuda.synchronize()
    gs.check(f"n={n} players={players} {variant}")
    slot = _np(done0) < 0x80
    for b in range(nb):
        s = slice(b * n, (b + 1) * n)
        got_rows, play = _np(rows[s]).view(np.uint32), slot[s]
        if not played_block[b]:
            assert np.array_equal(got_rows, e["rows0"]) and np.array_equal(_np(done[s]), _np(done0[s]))
            assert (_np(fs[s]) == 77).all() and (_np(ln[s]) == 777).all() and (_np(counters[b]) == 123).all()
            assert int(max_len[b]) == 55 and (_np(log[:, s]) == -1).all()
            continue
        assert np.array_equal(got_rows[play], e["rows"][play]) and np.array_equal(got_rows[~play], e["rows0"][~play])
        assert np.array_equal(_np(done[s])[play], e["done"][play]) and (_np(done[s])[~play] == 0x80).all()
        assert np.array_equal(_np(fs[s])[play], e["final_score"][play]) and (_np(fs[s])[~play] == 77).all()
        assert np.array_equal(_np(ln[s])[play], e["length"][play]) and (_np(ln[s])[~play] == 777).all()
        assert int(counters[b, 0]) == 0 and int(max_len[b]) == (e["length"][play].max() if play.any() else 0)
        if not preset:
            assert np.array_equal(_np(counters[b]), e["counters"])
        want = e["actions"].copy()
        want[:, ~play] = -1
        assert np.array_equal(_np(log[:, s]), want)
    assert int(illegal) == 0


def _pool():
    from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR

    lists = [PR.piers_rules, PR.iggi_rules, PR.outer_rules, PR.flawed_rules, U.teams()["everything"](1)[0]]
    return [RulebasedAgent(r, seed=70 + i) for i, r in enumerate(lists)]


def _same_result(a, b):
    """Every figure of two EvalResults but `turns`."""
    da, db = a.as_dict(), b.as_dict()
    for d in (da, db):
        d.pop("turns")
    assert da == db
    assert np.array_equal(_np(a.scores), _np(b.scores)) and np.array_equal(_np(a.lengths), _np(b.lengths))


@pytest.mark.parametrize("explicit", [False, True])
@pytest.mark.parametrize("game,players", [("Hanabi-Full", 2), ("Hanabi-Small", 3)])
def test_crossplay_playout_equals_the_loop(game, players, explicit):
    """130 games: blocks of 256 rows with 126 padding rows; max_rows 600: two teams per chunk, several chunks. The explicit
    teams run with recorded actions."""
    import torch

    from hanabi_hip import CrossPlay

    pool = _pool()
    teams = None
    if explicit:
        teams = [(0, 1), (4, 4), (2, 3)] if players == 2 else [(0, 1, 2), (4, 4, 4), (3, 2, 1)]
    kw = dict(n_games=130, seed=SEED, max_rows=600, record_actions=explicit)
    fast, slow = CrossPlay(game, players, playout=True, **kw), CrossPlay(game, players, **kw)
    assert fast.n_pad == 256 and len(fast.chunks(25)) == 13
    a, b = fast.run(pool, teams=teams), slow.run(pool, teams=teams)
    assert fast.last_path == "playout" and slow.last_path == "loop"
    assert a.teams == b.teams and len(a.results) == (3 if explicit else 25)
    for x, y in zip(a.results, b.results):
        _same_result(x, y)
        assert x.turns == int(x.lengths.max()) <= y.turns
        if explicit:
            below = np.arange(x.turns)[:, None] < _np(x.lengths).astype(np.int64)[None, :]
            assert x.actions.shape == (x.turns, 130)
            assert np.array_equal(_np(x.actions)[below], _np(y.actions)[:x.turns][below])
            assert (_np(x.actions)[~below] == -1).all()
    if not explicit:
        assert torch.equal(a.mean_matrix(), b.mean_matrix()) and torch.equal(a.stderr_matrix(), b.stderr_matrix())
        assert len({r.mean for r in a.results}) > 5
    # a second run plays the same deals again: the scratch rows are re-copied
    again = fast.run(pool, teams=teams)
    for x, y in zip(again.results, b.results):
        _same_result(x, y)


def test_crossplay_takes_the_loop_where_the_kernel_does_not_apply():
    import torch

    import hanabi_hip
    from hanabi_agents.rlax_dqn import ActionSpec, DQNAgent, ObservationSpec, RlaxRainbowParams
    from hanabi_hip import CrossPlay

    rules = _pool()[:2]
    cfg = hanabi_hip.make_config("Hanabi-Full", 2)
    L = hanabi_hip.lib()
    torch.manual_seed(0)
    params = RlaxRainbowParams(train_batch_size=128, experience_buffer_size=1024, compute_dtype="bfloat16", packed_obs=True, layers=[512],
                               seed=5)
    dqn = DQNAgent(ObservationSpec((1, L.hb_obs_len(C.byref(cfg)))), ActionSpec(L.hb_num_actions(C.byref(cfg))), params, device="cuda")
    kw = dict(n_games=64, seed=SEED)
    fast, slow = CrossPlay("Hanabi-Full", 2, playout=True, **kw), CrossPlay("Hanabi-Full", 2, **kw)
    a, b = fast.run(rules + [dqn]), slow.run(rules + [dqn])
    assert fast.last_path == "loop" and slow.last_path == "loop"
    assert a.as_dict() == b.as_dict()
    only_rules = [(0, 1), (1, 0)]                      # the DQN agent stays in the pool, no team uses it
    c = fast.run(rules + [dqn], teams=only_rules)
    assert fast.last_path == "playout"
    for x, y in zip(c.results, slow.run(rules + [dqn], teams=only_rules).results):
        _same_result(x, y)
    resp = CrossPlay("Hanabi-Full", 2, playout=True, responses=True, **kw)
    r = resp.run(rules)
    assert resp.last_path == "loop" and r.responses is not None


def test_rule_search_scores_are_the_evaluators():
    """One run: 8 lists, 2 generations, Hanabi-Small 2p, 256 games. The best mean is the Evaluator's of [best, best] on the same
    deals (loop path), and validate() is the Evaluator's on other deals."""
    from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR
    from hanabi_hip import Evaluator, RuleSearch

    rs = RuleSearch("Hanabi-Small", 2, n_games=256, seed=11, population=8, elite=2)
    out = rs.run([PR.piers_rules, PR.flawed_rules], generations=2, rng_seed=3)
    assert len(out.history) == 3 and out.history[0] <= out.history[1] <= out.history[2] == out.mean
    best = [RulebasedAgent(out.best), RulebasedAgent(out.best)]
    assert out.mean == Evaluator("Hanabi-Small", 2, n_games=256, seed=11).run(best).mean
    assert out.mean >= Evaluator("Hanabi-Small", 2, n_games=256, seed=11).run([RulebasedAgent(PR.piers_rules)] * 2).mean
    fresh = rs.validate([out.best, PR.piers_rules], n_games=128, seed=12)
    assert fresh[0] == Evaluator("Hanabi-Small", 2, n_games=128, seed=12).run(best).mean
    assert rs.run([PR.piers_rules, PR.flawed_rules], generations=2, rng_seed=3) == out
