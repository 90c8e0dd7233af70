"""The one conditioned-sampling path on the GPU (hanabi_hip.search): ConditionedDeterminizer.sample is sample_history on the
`LastMove`, so it gives what sample_history gives on a depth-1 `PartnerHistory` pushed by hand, field by field of the
`BeliefSample`; the hard filter's depth_used at depth 1 is fallback == 0; `survivors()` is the gather written out root by root;
and RolloutSearch.run with the tuple history keeps its public shapes and equals the run on that depth-1 history.

Hanabi-Small, 2 players, [Piers, an untrained DQN agent] as in tests/test_belief_soft_gpu.py, eight turns in: seat 0 observes,
seat 1 has moved last. The partner model is the DQN agent (`obs_only_eval`: the stateless encode path, padded per slab at m = 6
where a slab of 6 rows is no multiple of 16 bytes, one call at m = 8) and a Piers agent (the scratch env either way). At least
one root has ended (Small has one life), one running root is given valid = 0."""
import pytest

pytestmark = pytest.mark.gpu

R, OV, TURNS, SEAT, EPS = 2, 3, 8, 0, 0.1
_games = {}


def _game(m):
    """m games, TURNS turns in, of the first env seed from 7 on that leaves a finished root and at least three running ones ->
    dict(seed, team, cfg, rows, prev, legal, valid, H1, H2): H2 the depth-2 PartnerHistory seat 0 has kept as SearchPlayer does,
    H1 the depth-1 one pushed by hand with the last entry alone; `valid` is 0 at the first running root, in the tuple, H1 and H2.
    Played once per m and shared; nothing in it is written to afterwards."""
    import torch
    from test_belief_soft_gpu import _dqn

    import hanabi_hip
    from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR
    from hanabi_hip import PartnerHistory, last_move_uid
    from hanabi_hip.search import _ask, running

    if m in _games:
        return _games[m]
    for seed in range(7, 39):
        env = hanabi_hip.HanabiEnv("Hanabi-Small", 2, n_games=m, seed=seed, auto_reset=False, packed=True)
        team = [RulebasedAgent(PR.piers_rules, seed=11), _dqn(env, seed=6)]
        act = torch.empty(m, dtype=torch.int32, device="cuda")
        states, moves, scratch = [env.export_state().clone()], [], {}
        env.observe()
        for t in range(TURNS):
            _ask(team[t % 2], env, seed, t + 1, act, scratch)
            moves.append(act.clone())
            env.step(act)
            states.append(env.export_state().clone())
        live = running(states[-1])
        if int(live.sum()) >= 3 and not bool(live.all()):
            break
    else:
        raise AssertionError("no env seed in 7..38 leaves a finished root and three running ones")
    env.observe()
    rows, prev = states[-1], states[-2]
    valid = torch.ones(m, dtype=torch.uint8, device="cuda")
    valid[int(live.int().argmax())] = 0
    H1 = PartnerHistory(env.cfg, m, 1, "cuda", partner_seed=seed, first_game_id=0)
    H1.push(prev, last_move_uid(env.cfg, rows), TURNS, valid, seat=SEAT)
    H2 = PartnerHistory(env.cfg, m, 2, "cuda", partner_seed=seed, first_game_id=0)
    ones = torch.ones(m, dtype=torch.uint8)
    H2.push(states[TURNS - 3], last_move_uid(env.cfg, states[TURNS - 2]), TURNS - 2, ones, seat=SEAT)
    H2.own_move(moves[TURNS - 2])
    H2.push(prev, last_move_uid(env.cfg, rows), TURNS, valid, seat=SEAT)
    _games[m] = dict(seed=seed, team=team, cfg=env.cfg, rows=rows, prev=prev, legal=env.legal.clone(), live=live, valid=valid, H1=H1, H2=H2)
    return _games[m]


def _partner(g, kind):
    from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR

    return g["team"][1] if kind == "dqn" else RulebasedAgent(PR.piers_rules, seed=12)


def _same(a, b):
    import torch

    assert type(a).__name__ == type(b).__name__ == "BeliefSample" and len(a) == len(b) == 6
    for name, x, y in zip(a._fields, a, b):
        if x is None or y is None:
            assert x is None and y is None, name
        else:
            assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), name


@pytest.mark.parametrize("kind", ["dqn", "piers"])
@pytest.mark.parametrize("m", [6, 8])
def test_sample_is_sample_history_on_the_last_move(m, kind):
    import torch

    from hanabi_hip import BeliefSample, ConditionedDeterminizer

    g = _game(m)
    rows, prev, valid, seed, partner = g["rows"], g["prev"], g["valid"], g["seed"], _partner(g, kind)
    assert getattr(partner, "obs_only_eval", False) is (kind == "dqn")
    SW = rows.shape[1]
    kw = dict(seed=5, draw=TURNS + 1, partner_seed=seed, first_game_id=0, first_row_id=100)
    hard = {}
    for stateless in (True, False):
        one, hist = (ConditionedDeterminizer(config=g["cfg"], stateless=stateless) for _ in range(2))
        for eps in (None, EPS):
            for with_out in (False, True):
                bufs = [(torch.empty((m * R, SW), dtype=torch.int32, device="cuda"), torch.empty(m * R, dtype=torch.int32, device="cuda"))
                        for _ in range(2)] if with_out else [None, None]
                a = one.sample(rows, prev, partner, SEAT, R, OV, partner_draw=TURNS, valid=valid, out=bufs[0], epsilon=eps, **kw)
                b = hist.sample_history(rows, g["H1"], partner, SEAT, R, OV, out=bufs[1], epsilon=eps, **kw)
                assert isinstance(a, BeliefSample)
                _same(a, b)                                                                        # (a)
                assert (a.ess is None) == (eps is None) and a.n_surv.shape == (1, m) and a.depth_used.dtype == torch.int32
                if with_out:
                    assert a.rows is bufs[0][0] and a.weights is bufs[0][1] and b.weights is bufs[1][1]
                else:
                    assert a.weights.dtype == torch.int64
                assert torch.equal(a.depth_used, (a.fallback == 0).int())                          # (b), and the soft filter's L
                assert bool((a.fallback[~g["live"]] == 2).all()) and bool((a.fallback[valid == 0] == 2).all())
                if eps is None and not with_out:
                    hard[stateless] = a
    _same(hard[True], hard[False])
    fb = hard[True].fallback
    print("seed", seed, "live", g["live"].tolist(), "n_surv", hard[True].n_surv.tolist(), "fallback", fb.tolist())
    assert bool((fb != 2).any()) and int((fb == 2).sum()) >= 2   # a filtered root; the finished one and the one with valid = 0


@pytest.mark.parametrize("m", [6, 8])
def test_survivors_is_the_gather_at_the_depth_used(m):
    import torch

    from hanabi_hip import ConditionedDeterminizer

    g = _game(m)
    cd = ConditionedDeterminizer(config=g["cfg"])
    kw = dict(seed=5, draw=TURNS + 1, partner_seed=g["seed"], first_game_id=0, first_row_id=100)
    seen = set()
    for eps in (None, EPS):
        s = cd.sample_history(g["rows"], g["H2"], g["team"][1], SEAT, R, OV, epsilon=eps, **kw)
        assert s.n_surv.shape == (2, m)
        used = s.depth_used.tolist()
        want = [int(s.n_surv[u - 1, i]) if u > 0 else 0 for i, u in enumerate(used)]               # (c)
        got = s.survivors()
        assert got.dtype == torch.int32 and got.tolist() == want
        assert all(u == 0 for u, live, v in zip(used, g["live"].tolist(), g["valid"].tolist()) if not live or v == 0)
        assert bool((got[s.depth_used == 0] == 0).all())
        seen |= set(used)
        print("eps", eps, "n_surv", s.n_surv.tolist(), "depth_used", used, "survivors", want)
    assert 0 in seen and 2 in seen


@pytest.mark.parametrize("kind", ["dqn", "piers"])
@pytest.mark.parametrize("m", [6, 8])
def test_rollout_search_with_the_tuple_history(m, kind):
    import torch

    from hanabi_hip import RolloutSearch

    g = _game(m)
    blueprint = [g["team"][0], _partner(g, kind)]
    for eps in (None, EPS):
        rs = RolloutSearch(config=g["cfg"], replicas=R, seed=5, oversample=OV, epsilon=eps)
        one = rs.run(g["rows"], g["legal"], blueprint, TURNS + 1, seat=SEAT, history=(g["prev"], g["seed"], TURNS, 0, g["valid"]))
        assert one.n_surv.shape == (m,) and one.depth_used is None                                 # (d)
        assert (one.ess is None) == (eps is None) and one.sample.n_surv.shape == (1, m)
        hist = rs.run(g["rows"], g["legal"], blueprint, TURNS + 1, seat=SEAT, history=g["H1"])
        assert hist.n_surv.shape == (1, m) and hist.depth_used.shape == (m,)
        assert torch.equal(one.value.view(torch.int32), hist.value.view(torch.int32))   # (bit for bit: NaN marks an illegal move)
        assert torch.equal(one.best, hist.best) and torch.equal(one.fallback, hist.fallback) and torch.equal(one.n_surv, hist.n_surv[0])
        assert bool(torch.isfinite(one.value).any()) and bool((one.best[g["live"]] >= 0).all())
