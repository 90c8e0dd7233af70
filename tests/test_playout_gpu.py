"""GPU: hb_rule_playout (rule-list teams played to the end in one launch) against the CPU expectation of tests/playout_util.py
and against the turn loop it replaces. Exact equality everywhere: every quantity is an integer or a copy of one."""
import ctypes as C

import numpy as np
import pytest

import playout_util as U
from guard_util import GuardSet

pytestmark = pytest.mark.gpu

SEED = U.DEAL_SEED
CASES = [("Hanabi-Very-Small", 2, 64), ("Hanabi-Small", 2, 193), ("Hanabi-Small", 4, 65), ("Hanabi-Full", 2, 257),
         ("Hanabi-Full", 3, 129), ("Hanabi-Full", 5, 65), ("Hanabi-Full", 2, 1), ("Hanabi-Full", 2, 63)]
# the other six instantiations of the kernel (with CASES: all twelve), each with a partial wavefront; all four teams
NEW_CASES = [("Hanabi-Full", 4, 65), ("Hanabi-Small", 3, 129), ("Hanabi-Small", 5, 65), ("Hanabi-Very-Small", 3, 63),
             ("Hanabi-Very-Small", 4, 65), ("Hanabi-Very-Small", 5, 193)]
TEAMS = ["piers", "flawed", "mixed", "everything"]


def _agents(team, P):
    from hanabi_agents.rule_based import RulebasedAgent

    return [RulebasedAgent(r, seed=50 + p) for p, r in enumerate(U.teams()[team](P))]


def _dev_rows(rows_u32):
    import torch

    return torch.from_numpy(np.ascontiguousarray(rows_u32).view(np.int32)).cuda()


def _np(t):
    return t.cpu().numpy()


def test_the_cases_launch_every_instantiation():
    import deep_play

    assert {(g, p) for g, p, _ in CASES + NEW_CASES} == set(deep_play.VARIANTS) and len(deep_play.VARIANTS) == 12
    assert all(n % 64 for _, _, n in NEW_CASES)


@pytest.mark.parametrize("team", TEAMS)
@pytest.mark.parametrize("game,players,n", CASES + NEW_CASES)
def test_kernel_matches_the_cpu_expectation(game, players, n, team):
    import hanabi_hip

    e = U.expected(game, players, n, team)
    cfg = hanabi_hip.make_config(game, players)
    res = hanabi_hip.rule_playout(cfg, _dev_rows(e["rows0"]), _agents(team, players), SEED, log=True)
    _assert_matches(res, e)


def _assert_matches(res, e):
    """Every output of a logged rule_playout against oracle_playout's."""
    assert np.array_equal(_np(res.rows).view(np.uint32), e["rows"])
    assert np.array_equal(_np(res.done), e["done"])
    assert np.array_equal(_np(res.final_score), e["final_score"])
    assert np.array_equal(_np(res.length), e["length"])
    assert np.array_equal(_np(res.counters), e["counters"])
    acts, want = _np(res.actions), e["actions"]
    assert acts.shape == want.shape
    below = np.arange(acts.shape[0])[:, None] < e["length"].astype(np.int64)[None, :]
    assert np.array_equal(acts[below], want[below])
    assert (acts[~below] == -1).all()
    assert int(res.illegal) == 0 == e["illegal"]
    assert int(res.max_len) == e["max_len"]
    assert int(res.counters[0]) == 0


@pytest.mark.parametrize("team", TEAMS)
def test_game_ids_across_two_to_the_32(team):
    """first_game_id = 2^32 - 40: games 0..39 have ids below 2^32, games 40..128 above (the id's high word is part of the rule
    walk's Philox key). The deals are the oracle env's of that id base; on the same deals the moves are not those of base 0."""
    import hanabi_hip

    base, n = 2 ** 32 - 40, 129
    e = U.expected("Hanabi-Full", 2, n, team, first_game_id=base)
    cfg = hanabi_hip.make_config("Hanabi-Full", 2)
    res = hanabi_hip.rule_playout(cfg, _dev_rows(e["rows0"]), _agents(team, 2), SEED, first_game_id=base, log=True)
    _assert_matches(res, e)
    zero = hanabi_hip.rule_playout(cfg, _dev_rows(e["rows0"]), _agents(team, 2), SEED, first_game_id=0, log=True)
    other = (_np(zero.actions) != _np(res.actions)).any(0)
    assert other[:40].any() and other[40:].any()


@pytest.mark.parametrize("game,players", [(g, p) for g, p, _ in NEW_CASES])
def test_search_playout_equals_the_loop_on_deep_roots(game, players):
    """The instantiations no search had driven, from mid-game rows: the running rows of tests/deep_rows.pick whose seat to act
    is the last seat (first_seat != 0; cards to draw and empty decks, Very-Small 5 empty decks only), every legal first move
    forced, [Piers] * P. One launch against the turn loop, figure for figure."""
    import torch

    import deep_rows as DR
    import hanabi_hip
    from hanabi_hip import RolloutSearch, encode_rows

    p = DR.pick(game, players)
    seat, deck = (p.rows[:, 0] >> 13) & 7, p.rows[:, 0] & 63
    mine = (((p.rows[:, 0] >> 19) & 3) == 0) & (seat == players - 1)
    assert (mine & (deck == 0)).sum() >= 4 and ((mine & (deck > 0)).sum() >= 2 or (game, players) == ("Hanabi-Very-Small", 5))
    rows = _dev_rows(p.rows[mine])
    cfg = hanabi_hip.make_config(game, players)
    _, legal = encode_rows(cfg, rows)
    assert bool((legal != 0).any(1).all())
    team = _agents("piers", players)
    fast = RolloutSearch(game, players, replicas=4, seed=3, playout=True)
    slow = RolloutSearch(game, players, replicas=4, seed=3, playout=False)
    a = fast.run(rows, legal, team, draw=5)
    assert fast.last_path == "playout"
    b = slow.run(rows, legal, team, draw=5)
    assert slow.last_path == "loop"
    for k in ("value", "wsum", "n_live", "best"):
        x, y = getattr(a, k), getattr(b, k)
        assert torch.equal(torch.nan_to_num(x.double(), nan=-7.0), torch.nan_to_num(y.double(), nan=-7.0)), k
        assert torch.equal(torch.isnan(x.double()), torch.isnan(y.double())), k
    assert a.rollouts == b.rollouts > 0 and a.dead == b.dead == 0 and a.turns <= b.turns
    assert bool((a.best >= 0).all()) and torch.equal(rows, _dev_rows(p.rows[mine]))


def _dqn(env_like, seed=5):
    from hanabi_agents.rlax_dqn import ActionSpec, DQNAgent, ObservationSpec, RlaxRainbowParams

    params = RlaxRainbowParams(train_batch_size=128, experience_buffer_size=8192, compute_dtype="bfloat16", packed_obs=True,
                               layers=[512], seed=seed)
    return DQNAgent(ObservationSpec((1, env_like.obs_len)), ActionSpec(env_like.num_actions), params, device="cuda")


def _same_result(a, b):
    """Every figure of two EvalResults but `turns` (and the response counts, which only one of them may carry)."""
    da, db = a.as_dict(), b.as_dict()
    for d in (da, db):
        d.pop("turns")
        d.pop("responses", None)
    assert da == db
    assert np.array_equal(_np(a.scores), _np(b.scores)) and np.array_equal(_np(a.lengths), _np(b.lengths))


@pytest.mark.parametrize("team", ["mixed", "everything"])
def test_evaluator_playout_equals_the_loop(team):
    from hanabi_hip import Evaluator

    agents = _agents(team, 2)
    fast = Evaluator("Hanabi-Full", 2, n_games=257, seed=SEED, playout=True, record_actions=True)
    slow = Evaluator("Hanabi-Full", 2, n_games=257, seed=SEED, playout=False, record_actions=True)
    a, b = fast.run(agents), slow.run(agents)
    assert fast.last_path == "playout" and slow.last_path == "loop"
    _same_result(a, b)
    assert a.turns == int(a.lengths.max()) <= b.turns
    below = np.arange(a.turns)[:, None] < _np(a.lengths).astype(np.int64)[None, :]
    assert np.array_equal(_np(a.actions)[below], _np(b.actions)[:a.turns][below])
    # the CPU expectation of the same deals (the evaluator's deals are the oracle env's of the same seed)
    e = U.expected("Hanabi-Full", 2, 257, team)
    assert np.array_equal(_np(a.scores), e["final_score"].astype(np.int32))
    # a second run plays the same deals again: the scratch rows are re-copied
    _same_result(fast.run(agents), b)


def test_evaluator_takes_the_loop_where_the_kernel_does_not_apply():
    import torch

    from hanabi_hip import Evaluator

    piers = _agents("piers", 2)
    fast = Evaluator("Hanabi-Full", 2, n_games=64, seed=SEED, playout=True)
    slow = Evaluator("Hanabi-Full", 2, n_games=64, seed=SEED)
    fast._setup()
    torch.manual_seed(0)
    team = [_dqn(fast.env), piers[1]]
    a, b = fast.run(team), slow.run(team)
    assert fast.last_path == "loop"
    assert a.as_dict() == b.as_dict()
    resp = Evaluator("Hanabi-Full", 2, n_games=64, seed=SEED, playout=True, responses=True)
    r = resp.run(piers)
    assert resp.last_path == "loop" and r.responses is not None
    _same_result(r, fast.run(piers))
    assert fast.last_path == "playout"


@pytest.mark.parametrize("game,players,n", [("Hanabi-Full", 2, 257), ("Hanabi-Small", 4, 65)])
def test_turn_cap_equals_five_turns_of_the_loop(game, players, n):
    import torch

    import hanabi_hip
    from hanabi_hip import _capi as K

    cap, team = 5, _agents("mixed", players)
    e = U.expected(game, players, n, "mixed", max_turns=cap)
    full = U.expected(game, players, n, "mixed")
    cfg = hanabi_hip.make_config(game, players)
    res = hanabi_hip.rule_playout(cfg, _dev_rows(e["rows0"]), team, SEED, max_turns=cap)
    # five turns of the loop: the agents' eval_moves, the env step, hb_eval_tally
    env = hanabi_hip.HanabiEnv(config=cfg, n_games=n, seed=SEED, packed=True)
    env.import_state(_dev_rows(e["rows0"]))
    L = hanabi_hip.lib()
    done = torch.zeros(n, dtype=torch.uint8, device="cuda")
    fs = torch.zeros(n, dtype=torch.int8, device="cuda")
    ln = torch.zeros(n, dtype=torch.int16, device="cuda")
    counters = torch.zeros(L.hb_eval_counters(C.byref(cfg)), dtype=torch.int64, device="cuda")
    counters[0] = n
    act = torch.zeros(n, dtype=torch.int32, device="cuda")
    for t in range(cap):
        team[t % players].eval_moves(env, SEED, t + 1, act)
        env.step(act)
        K.check(L.hb_eval_tally(C.byref(cfg), n, t % players, t, K.dptr(act), K.dptr(env.reward), K.dptr(env.terminal), K.dptr(env.score),
                                K.dptr(done), K.dptr(fs), K.dptr(ln), K.dptr(counters), K.current_stream()))
    assert torch.equal(res.rows, env.export_state())
    assert torch.equal(res.counters, counters) and torch.equal(res.done, done)
    assert torch.equal(res.final_score, fs) and torch.equal(res.length, ln)
    longer = full["length"] > cap
    assert 0 < longer.sum() and int(res.counters[0]) == longer.sum()
    assert np.array_equal((_np(res.done) & 0x80) == 0, longer)            # games longer than the cap are still running
    assert np.array_equal(_np(res.rows).view(np.uint32), e["rows"])
    assert int(res.max_len) == (full["length"][~longer].max() if (~longer).any() else 0)


def _roots(game, turns, n=64):
    """n games `turns` turns into [Piers, Piers] play: (env, team); seat turns % 2 is to act."""
    import torch

    import hanabi_hip

    team = _agents("piers", 2)
    env = hanabi_hip.HanabiEnv(game, 2, n_games=n, seed=SEED, auto_reset=False, packed=True)
    act = torch.zeros(n, dtype=torch.int32, device="cuda")
    for t in range(turns):
        team[t % 2].eval_moves(env, SEED, t + 1, act)
        env.step(act)
    return env, team


@pytest.mark.parametrize("game,turns", [("Hanabi-Full", 10), ("Hanabi-Full", 11), ("Hanabi-Small", 30), ("Hanabi-Small", 31)])
def test_search_playout_equals_the_loop(game, turns):
    import torch

    from hanabi_hip import RolloutSearch

    from hanabi_hip.search import running

    env, team = _roots(game, turns)
    rows, legal = env.export_state(), env.legal.clone()
    finished = 64 - int(running(rows).sum())
    assert (0 < finished < 64) if game == "Hanabi-Small" else finished == 0   # Small: finished roots among the 64
    base = torch.zeros(64, dtype=torch.int32, device="cuda")
    team[turns % 2].eval_moves(env, SEED, turns + 1, base)
    fast = RolloutSearch(game, 2, replicas=8, seed=3, playout=True)
    slow = RolloutSearch(game, 2, replicas=8, seed=3, playout=False)
    for baseline in (None, base):
        a = fast.run(rows, legal, team, draw=turns, baseline=baseline)
        b = slow.run(rows, legal, team, draw=turns, baseline=baseline)
        assert fast.last_path == "playout" and slow.last_path == "loop"
        for k in ("value", "wsum", "n_live", "best") + (("diff", "se", "n_pair") if baseline is not None else ()):
            x, y = getattr(a, k), getattr(b, k)
            assert torch.equal(torch.nan_to_num(x.double(), nan=-7.0), torch.nan_to_num(y.double(), nan=-7.0)), k
            assert torch.equal(torch.isnan(x.double()), torch.isnan(y.double())), k
        assert a.rollouts == b.rollouts > 0 and a.dead == b.dead and a.turns <= b.turns
    assert torch.equal(rows, env.export_state())
    # a horizon, or a seat that is no rule list, takes the loop
    fast.set_horizon(3, "score")
    fast.run(rows, legal, team, draw=turns)
    assert fast.last_path == "loop"


def test_search_player_with_playout_scores_the_same():
    from hanabi_hip import Evaluator, SearchPlayer

    team = _agents("piers", 2)
    ev = Evaluator("Hanabi-Full", 2, n_games=64, seed=SEED)
    res = [ev.run([SearchPlayer(team, 0, replicas=8, z=2, playout=p), team[1]]) for p in (True, False)]
    assert ev.last_path == "loop"
    assert res[0].as_dict() == res[1].as_dict()
    assert np.array_equal(_np(res[0].scores), _np(res[1].scores))


@pytest.mark.parametrize("variant", ["plain", "log", "preset"])
@pytest.mark.parametrize("players", [2, 5])
@pytest.mark.parametrize("n", [1, 63, 65, 129])
def test_guard_bands(n, players, variant):
    """Every output of hb_rule_playout in a guarded buffer, every input registered: no guard byte and no input changes."""
    import torch

    import hanabi_hip
    from hanabi_hip import _capi as K, evaluate, playout

    game = "Hanabi-Full"
    e = U.expected(game, players, n, "mixed")
    cfg = hanabi_hip.make_config(game, players)
    SW, NC, T = e["rows0"].shape[1], len(e["counters"]), evaluate.max_turns(cfg)
    team = _agents("mixed", players)
    gs = GuardSet("hb_rule_playout")
    tile = 64   # one wavefront's games: the kernel's tile
    preset = variant == "preset"
    done0 = torch.zeros(n, dtype=torch.uint8, device="cuda")
    first = None
    if preset:
        done0[::3] = 0x80                                   # slots that are not played
        first = gs.inp("first_moves", torch.from_numpy(e["actions"][0].copy()).cuda())   # the rule walk's own first moves
    rows = gs.out("rows", (n, SW), torch.int32, tile * SW, init=_dev_rows(e["rows0"]))
    done = gs.out("done", (n,), torch.uint8, 4 * tile, init=done0)
    fs = gs.out("final_score", (n,), torch.int8, 4 * tile, init=torch.zeros(n, dtype=torch.int8, device="cuda"))
    ln = gs.out("length", (n,), torch.int16, 4 * tile, init=torch.zeros(n, dtype=torch.int16, device="cuda"))
    c0 = torch.zeros(NC, dtype=torch.int64, device="cuda")
    c0[0] = int((done0 < 0x80).sum())
    counters = gs.out("counters", (NC,), torch.int64, 64, init=c0)
    log = gs.out("log", (T, n), torch.int32, 4 * tile) if variant != "plain" else None
    illegal = gs.out("illegal", (1,), torch.int64, 64, init=torch.zeros(1, dtype=torch.int64, device="cuda"))
    max_len = gs.out("max_len", (1,), torch.int32, 64, init=torch.zeros(1, dtype=torch.int32, device="cuda"))
    tabs, lens = playout.rule_tables(team)
    K.check(playout._fn()(C.byref(cfg), K.dptr(rows), n, 0, tabs, lens, SEED, 0, K.dptr(first), T, K.dptr(done), K.dptr(fs), K.dptr(ln),
                          K.dptr(counters), K.dptr(log), K.dptr(illegal), K.dptr(max_len), K.current_stream()))
    torch.cuda.synchronize()
    gs.check(f"n={n} players={players} {variant}")
    played = _np(done0) < 0x80
    assert np.array_equal(_np(rows).view(np.uint32)[played], e["rows"][played])
    assert np.array_equal(_np(rows).view(np.uint32)[~played], e["rows0"][~played])       # not played: the row stays
    assert np.array_equal(_np(done)[played], e["done"][played]) and (_np(done)[~played] == 0x80).all()
    assert np.array_equal(_np(fs)[played], e["final_score"][played]) and (_np(fs)[~played] == 0).all()
    assert np.array_equal(_np(ln)[played], e["length"][played]) and (_np(ln)[~played] == 0).all()
    assert int(illegal) == 0 and int(counters[0]) == 0
    assert int(max_len) == (e["length"][played].max() if played.any() else 0)
    if not preset:
        assert np.array_equal(_np(counters), e["counters"])
    if log is not None:
        want = e["actions"].copy()
        want[:, ~played] = -1
        assert np.array_equal(_np(log), want)


def test_session_search_with_playout_leaves_training_untouched(monkeypatch):
    """Session A trains, searches a rule-list blueprint with playout=True, trains on; session B only trains: bit-identical. And
    the search's result is the loop's."""
    import torch

    import hanabi_hip
    from hanabi_agents.rlax_dqn import ActionSpec, DQNAgent, ObservationSpec, RlaxRainbowParams
    from hanabi_hip.selfplay import SelfPlaySession

    def _session_state(sess):
        torch.cuda.synchronize()
        return sess.checkpoint_state(include_replay=True)

    def _assert_same(x, y, path="state"):
        if isinstance(x, dict):
            assert x.keys() == y.keys(), path
            for k in x:
                if k != "params":   # (a repr holding the addresses of the epsilon / beta lambdas)
                    _assert_same(x[k], y[k], f"{path}.{k}")
        elif isinstance(x, (list, tuple)):
            assert len(x) == len(y), path
            for i, (u, v) in enumerate(zip(x, y)):
                _assert_same(u, v, f"{path}[{i}]")
        elif isinstance(x, torch.Tensor):
            assert torch.equal(x, y), path
        else:
            assert x == y, path

    monkeypatch.setenv("HB_ACTOR_FUSED_MIN_ROWS", "0")
    n = 128

    def session():
        torch.manual_seed(0)
        torch.cuda.manual_seed(0)
        flags = hanabi_hip.FLAG_AUTO_RESET | hanabi_hip.FLAG_RESET_START_NEXT
        env = hanabi_hip.HanabiEnv(config=hanabi_hip.make_config("Hanabi-Full", 2, flags), n_games=n, seed=5, packed=True)
        params = RlaxRainbowParams(train_batch_size=128, experience_buffer_size=n * 8, mask_terminal=True, target_update_period=6,
                                   compute_dtype="bfloat16", packed_obs=True, layers=[512], learning_rate=0.01)
        mk = lambda s: DQNAgent(ObservationSpec((n, env.obs_len)), ActionSpec(env.num_actions), params._replace(seed=s), device="cuda")
        return SelfPlaySession(env, [mk(1), mk(2)])

    team = _agents("piers", 2)
    a = session()
    a.run(12)
    before = _session_state(a)
    fast = a.search(blueprint=team, replicas=4, seed=3, playout=True)
    path = a._searches[(4, 3)].last_path
    _assert_same(before, _session_state(a))
    slow = a.search(blueprint=team, replicas=4, seed=3)
    assert path == "playout" and a._searches[(4, 3)].last_path == "loop"
    assert torch.equal(torch.nan_to_num(fast.value, nan=-7.0), torch.nan_to_num(slow.value, nan=-7.0))
    assert torch.equal(fast.best, slow.best) and fast.rollouts == slow.rollouts > 0
    a.run(12)
    b = session()
    b.run(24)
    _assert_same(_session_state(a), _session_state(b))
