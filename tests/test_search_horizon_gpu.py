"""Depth-limited rollouts on the GPU (hanabi_hip.search): a horizon that is never reached is the full
search bit for bit, the quarter-point buffer of a horizon-1 search against `search_leaf_ref` fed from a scratch env, the seat
whose agent values the leaves, leaf="score", `DQNAgent.eval_q` against `eval_moves`, and the horizon through SearchPlayer and
SelfPlaySession.search. tests/test_search_horizon_cpu.py holds the leaf step's arithmetic."""
import numpy as np
import pytest
from search_util import _dqn, _mid_game_env, _team

pytestmark = pytest.mark.gpu

M, R = 5, 3   # five roots: not a multiple of the four rows a workgroup of the search kernels covers


def _bits(t):
    """A tensor as integers: NaNs and infinities compare like every other value."""
    import torch

    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()]) if t.is_floating_point() else t


def _same(a, b, names):
    import torch

    for k in names:
        x, y = getattr(a, k), getattr(b, k)
        assert x.dtype == y.dtype and torch.equal(_bits(x), _bits(y)), k


def _small_roots(turns=3):
    """M Hanabi-Small roots `turns` random moves in, most of them (not all) still running: one life is soon lost to random play,
    so the first seed that leaves M - 1 running is taken (a pure function of the Philox deals: the same roots every time)."""
    for seed in range(6, 70):
        src = _mid_game_env("Hanabi-Small", 2, M, turns, seed=seed)
        rows = src.export_state()
        if int((((rows[:, 0] >> 19) & 3) == 0).sum()) == M - 1:
            src.observe()
            return src, rows, src.legal.clone()
    raise AssertionError("no seed leaves all but one root running")


def test_a_horizon_that_is_never_reached_is_the_full_search():
    import torch

    from hanabi_hip import RolloutSearch
    from hanabi_hip.evaluate import max_turns

    src, rows, legal = _small_roots()
    team = [_dqn(src, seed=5), _dqn(src, seed=6)]
    base = torch.where(legal != 0, torch.arange(legal.shape[1], device="cuda").view(1, -1), 99).amin(1).int()   # lowest legal uid
    names = ("value", "wsum", "n_live", "best", "diff", "se", "n_pair")
    full = RolloutSearch("Hanabi-Small", 2, replicas=R, seed=21).run(rows, legal, team, 13, baseline=base)
    assert full.horizon is None and full.leaves == 0 and full.rollouts > 0
    for H in (max_turns(src.cfg), max_turns(src.cfg) + 7, full.turns):
        rs = RolloutSearch("Hanabi-Small", 2, replicas=R, seed=21, horizon=H)
        res = rs.run(rows, legal, team, 13, baseline=base)
        _same(res, full, names)
        assert res.horizon == H and res.leaves == 0 and res.rollouts == full.rollouts and res.turns == full.turns
        assert "leaf4" not in rs._sized[(M, legal.shape[1], R)]   # no leaf was valued: nothing was allocated for one
    # the second stage honours it too
    chal = torch.where(legal != 0, torch.arange(legal.shape[1], device="cuda").view(1, -1), -1).amax(1).int()   # highest legal uid
    two = [RolloutSearch("Hanabi-Small", 2, replicas=R, seed=21, horizon=H).confirm(rows, legal, team, 13, base, chal, 4)
           for H in (None, max_turns(src.cfg))]
    _same(two[1], two[0], names)
    assert two[1].leaves == 0 and two[0].rollouts > 0


def test_horizon_one_equals_the_leaf_reference():
    import torch

    import hanabi_hip
    from hanabi_hip import RolloutSearch, leaf_dither_ref, search_leaf_ref
    from hanabi_hip.search import search_reduce

    src, rows, legal = _small_roots()
    A = legal.shape[1]
    team = [_dqn(src, seed=5), _dqn(src, seed=6)]
    cp = int((rows[0, 0] >> 13) & 7)
    base = torch.where(legal != 0, torch.arange(A, device="cuda").view(1, -1), 99).amin(1).int()
    rs = RolloutSearch("Hanabi-Small", 2, replicas=R, seed=21, horizon=1, first_game_id=500)
    res = rs.run(rows, legal, team, 13, baseline=base)
    b = rs._sized[(M, A, R)]
    got = b["leaf4"].clone()
    assert got.shape == (M, A, R) and got.dtype == torch.int8
    # the reference: the laid-out rows stepped once by their forced moves in a scratch env, eval_q of the seat then to act
    n = M * A * R
    env = hanabi_hip.HanabiEnv(config=rs.cfg, n_games=n, packed=True)
    env.import_state(b["rows"])
    env.step(b["forced"])
    q = team[(cp + 1) % 2].eval_q((env, (env.net_obs, env.legal))).clone()
    played = ((legal != 0).view(M, A, 1) & (b["weights"].view(M, 1, R) != 0)).cpu().numpy()   # (hb_search_layout's rule)
    ended = (env.terminal.view(M, A, R) != 0).cpu().numpy()
    score = env.score.view(M, A, R).cpu().numpy()
    done = np.where(played & ~ended, 0, 0x80).astype(np.uint8)
    final = np.where(played & ended, score, 0).astype(np.int8)
    u = leaf_dither_ref(21, 13, 0, M, R)
    want = search_leaf_ref(done, final, score, q.view(M, A, R, A).cpu().numpy(), env.legal.view(M, A, R, A).cpu().numpy(), u, 10)
    assert np.array_equal(got.cpu().numpy(), want)
    # ... in which the q values count (the same with v = 0 is another buffer), inside [0, 4 * max_score]
    assert not np.array_equal(want, search_leaf_ref(done, final, score, None, None, u, 10))
    assert want.min() >= 0 and want.max() <= 40
    # the values are the reduce kernel's on that buffer, divided by 4
    value, wsum, n_live, best = search_reduce(got, b["weights"].view(M, R), (legal != 0).to(torch.int8))
    assert torch.equal(_bits(res.value), _bits(value / 4)) and torch.equal(res.best, best) and torch.equal(res.n_live, n_live)
    assert torch.equal(res.wsum, wsum)
    assert res.turns == 1 and res.horizon == 1 and res.leaves == int((played & ~ended).sum()) and res.leaves > 0
    assert res.rollouts == int(played.sum())
    # the paired differences come from the same buffer: in quarter points they are whole multiples of 1 / (4 * sum w)
    ok = ~torch.isnan(res.diff)
    assert bool(ok.any()) and bool((res.diff[ok].abs() <= 10).all())
    # the same search again: the same bits (the dither is a function of seed, draw and row id)
    again = rs.run(rows, legal, team, 13, baseline=base)
    _same(again, res, ("value", "best", "diff", "se", "n_pair"))
    assert torch.equal(b["leaf4"], got)
    for a in team:
        assert a._draws == 0


class _Recording:
    """An agent that counts the eval_q calls it passes on."""

    def __init__(self, agent):
        self.agent, self.calls, self.rows = agent, 0, None

    def requires_vectorized_observation(self):
        return self.agent.requires_vectorized_observation()

    def eval_moves(self, *a, **k):
        return self.agent.eval_moves(*a, **k)

    def eval_q(self, observations, q_out=None, scratch=None):
        self.calls += 1
        self.rows = observations[1][0].shape[0]
        return self.agent.eval_q(observations, q_out=q_out, scratch=scratch)


class _Constant:
    """A leaf agent whose q is one number for every move."""

    def __init__(self, value):
        self.value = value

    def eval_q(self, observations, q_out=None, scratch=None):
        import torch

        return torch.full(observations[1][1].shape, self.value, dtype=torch.float32, device=observations[1][1].device)


@pytest.mark.parametrize("H", [3, 2])
def test_the_leaf_agent_is_the_seat_to_act_after_the_horizon(H):
    import torch

    from hanabi_hip import RolloutSearch

    m = 2
    src = _mid_game_env("Hanabi-Full", 3, m, 5, seed=6)
    src.observe()
    rows, legal = src.export_state(), src.legal.clone()
    assert bool(((((rows[:, 0] >> 19) & 3) == 0)).all())
    cp = int((rows[0, 0] >> 13) & 7)
    team = [_dqn(src, seed=5 + s) for s in range(3)]
    leaf = [_Recording(a) for a in team]
    res = RolloutSearch("Hanabi-Full", 3, replicas=R, seed=21, horizon=H, leaf=leaf).run(rows, legal, team, 13)
    assert res.turns == H and res.leaves > 0
    want = (cp + H) % 3
    assert [w.calls for w in leaf] == [1 if s == want else 0 for s in range(3)]
    assert leaf[want].rows == m * legal.shape[1] * R
    # leaf=None asks the blueprint's own agent of that seat: the same bits
    own = RolloutSearch("Hanabi-Full", 3, replicas=R, seed=21, horizon=H).run(rows, legal, team, 13)
    _same(own, res, ("value", "wsum", "n_live", "best"))
    assert own.leaves == res.leaves
    # ... and it is that seat's q that is added: agents whose q is the constant seat + 1 (whole points: no rounding)
    rs = RolloutSearch("Hanabi-Full", 3, replicas=R, seed=21, horizon=H, leaf=[_Constant(s + 1.0) for s in range(3)])
    const = rs.run(rows, legal, team, 13)
    b = rs._sized[(m, legal.shape[1], R)]
    running = (b["done"] & 0x80) == 0
    assert const.leaves == int(running.sum()) == res.leaves
    assert torch.equal(b["leaf4"].view(-1)[running], (4 * (b["env"].score.long() + want + 1)).to(torch.int8)[running])
    # a blueprint whose agent of that seat has no eval_q is refused before anything is played
    piers = _team("piers_piers", src)[0]
    mixed = [piers if s == want else team[s] for s in range(3)]
    with pytest.raises(TypeError, match="eval_q"):
        RolloutSearch("Hanabi-Full", 3, replicas=R, seed=21, horizon=H).run(rows, legal, mixed, 13)


def test_leaf_score_is_a_truncated_rollout():
    import torch

    from hanabi_hip import RolloutSearch

    src, rows, legal = _small_roots()
    A = legal.shape[1]
    team = _team("piers_piers", src)
    rs = RolloutSearch("Hanabi-Small", 2, replicas=R, seed=21, horizon=2, leaf="score")
    res = rs.run(rows, legal, team, 13)
    b = rs._sized[(M, A, R)]
    running = (b["done"] & 0x80) == 0
    assert res.turns == 2 and res.leaves == int(running.sum()) and res.leaves > 0
    want = torch.where(running, 4 * b["env"].score.long(), 4 * b["final_score"].long()).to(torch.int8)
    assert torch.equal(b["leaf4"].view(-1), want)
    # whole points in, whole points out: every value is a weighted mean of integers
    v = res.value[~torch.isnan(res.value)]
    assert bool((v >= 0).all()) and bool((v <= 10).all())
    with pytest.raises(TypeError, match="eval_q"):   # a rule list has no q of its own
        RolloutSearch("Hanabi-Small", 2, replicas=R, seed=21, horizon=2).run(rows, legal, team, 13)


@pytest.mark.parametrize("game,n", [("Hanabi-Full", 5), ("Hanabi-Full", 129), ("Hanabi-Small", 129)])
def test_eval_q_is_what_eval_moves_selects_from(game, n):
    import torch

    env = _mid_game_env(game, 2, n, 6, seed=4)
    env.observe()
    agent = _dqn(env, seed=9)
    obs = (env, (env.net_obs, env.legal))
    moves = agent.eval_moves(obs, 5, 9, torch.empty(n, dtype=torch.int32, device="cuda"), scratch={})
    scratch = {}
    q = agent.eval_q(obs, scratch=scratch)
    assert q.shape == (n, env.num_actions) and q.dtype == torch.float32 and q.is_cuda
    lg = env.legal != 0
    some = lg.any(1)   # (a finished game has no legal move)
    assert int(some.sum()) > n // 2
    best = torch.where(lg, q, float("-inf")).argmax(1).int()
    assert torch.equal(best[some], moves[some])
    assert bool(torch.isfinite(q[lg]).all())
    # the caller's buffers: scratch is reused, q_out receives a copy, and nothing of the agent moves
    kept = q.clone()
    out = torch.empty_like(q)
    assert agent.eval_q(obs, q_out=out, scratch=scratch) is out and torch.equal(out[lg], kept[lg])
    assert agent._draws == 0


def test_search_player_with_a_horizon_plays_whole_games():
    import torch

    from hanabi_hip import Evaluator, SearchPlayer

    ev = Evaluator("Hanabi-Full", 2, n_games=16, seed=7, record_actions=True)
    shape = _mid_game_env("Hanabi-Full", 2, 1, 0)   # (obs_len and num_actions)
    team = [_dqn(shape, seed=5), _dqn(shape, seed=6)]
    runs = []
    for _ in range(2):
        sp = SearchPlayer(team, 0, replicas=4, seed=2, horizon=2, z=1.0, confirm_replicas=4)
        res = ev.run([sp, team[1]])   # (raises on an illegal move)
        assert res.n_games == 16 and int(res.histogram.sum()) == 16
        assert sp.leaf_games > 0 and sp.moves == int(res.moves[0].sum()) and sp.last_result.horizon == 2
        assert sp.last_result.turns <= 2
        runs.append((res, sp.leaf_games, sp.rollouts, sp.deviations))
    (a, *ra), (b, *rb) = runs
    assert torch.equal(a.scores, b.scores) and torch.equal(a.lengths, b.lengths) and torch.equal(a.actions, b.actions) and ra == rb


def test_session_search_with_a_horizon_leaves_training_untouched(monkeypatch):
    import torch
    from test_search_gpu import _assert_same, _session_state

    import hanabi_hip
    from hanabi_agents.rlax_dqn import ActionSpec, DQNAgent, ObservationSpec, RlaxRainbowParams
    from hanabi_hip.selfplay import SelfPlaySession

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

    a = session()
    a.run(20)
    before = _session_state(a)
    res = a.search(replicas=4, seed=3, horizon=2)
    _assert_same(before, _session_state(a))
    assert res.value.shape == (n, 20) and res.horizon == 2 and res.turns == 2 and 0 < res.leaves <= res.rollouts
    legal = a.env.legal != 0
    assert bool((torch.isnan(res.value) == ~legal).all())
    assert bool((res.best >= 0).all()) and bool(legal.gather(1, res.best.long().view(-1, 1)).all())
    full = a.search(replicas=4, seed=3)   # the kept search goes back to whole rollouts
    assert full.horizon is None and full.leaves == 0 and full.turns > 2
    _assert_same(before, _session_state(a))
    a.run(20)
    b = session()
    b.run(40)
    _assert_same(_session_state(a), _session_state(b))
