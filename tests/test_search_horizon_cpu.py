"""Depth-limited rollouts without a GPU (hanabi_hip.search): the leaf step's specification
(`search_leaf_ref`, `leaf_dither_ref`) on hand-made arrays, its torch forms against it bit for bit, the constructors' checks, and
`DQNAgent.eval_q` on the torch path. tests/test_search_horizon_gpu.py holds the search itself."""
import numpy as np
import pytest

MAX = 25   # Hanabi-Full's top score


def _leaf(done, fs, score, q, legal, u, max_score=MAX):
    """search_leaf_ref on ONE root and slot: the arguments are given per replica ([R], q and legal [R, A])."""
    from hanabi_hip import search_leaf_ref

    a = lambda x, dt: np.asarray(x, dt)[None, None]
    out = search_leaf_ref(a(done, np.uint8), a(fs, np.int8), a(score, np.int8), None if q is None else a(q, np.float32), a(legal, np.int8),
                          np.asarray(u, np.float64)[None], max_score)
    assert out.dtype == np.int8 and out.shape == (1, 1, len(done))
    return out[0, 0].tolist()


def test_leaf_ref_on_hand_made_games():
    nan, inf = float("nan"), float("inf")
    #        finished  unplayed  running                 illegal max   NaN + inf among legal     no legal move
    done = [0x80 | 2, 0x80,     0,                      1,            0,                        0]
    fs = [17,         0,        9,                      9,            9,                        9]       # (read only when finished)
    score = [3,       3,        6,                      6,            6,                        6]
    q = [[9, 9, 9],   [9, 9, 9], [1.25, -3.0, 0.5],     [1.0, 99, 2.5], [nan, inf, 0.75],       [5, 5, 5]]
    legal = [[1, 1, 1], [1, 1, 1], [1, 1, 1],           [1, 0, 1],    [1, 1, 1],                [0, 0, 0]]
    u = [0.9, 0.9, 0.0, 0.0, 0.0, 0.999]
    # finished: 4 * 17; unplayed: final score 0; running: 4 * (6 + 1.25) = 29; the illegal 99 is passed over: 4 * 8.5 = 34; NaN and
    # +inf are passed over: 4 * 6.75 = 27; no legal move: v = 0, 24 exactly, whatever u
    assert _leaf(done, fs, score, q, legal, u) == [68, 0, 29, 34, 27, 24]
    # -inf among the legal entries is passed over like +inf; all entries non-finite: v = 0
    assert _leaf([0, 0], [0, 0], [6, 6], [[-inf, 0.5, -1], [nan, inf, -inf]], [[1, 1, 1]] * 2, [0.0, 0.5]) == [26, 24]
    # leaf="score": q None, v = 0
    assert _leaf(done, fs, score, None, legal, u) == [68, 0, 24, 24, 24, 24]


def test_leaf_ref_clamps_at_both_ends():
    one = lambda score, v, u: _leaf([0], [0], [score], [[v]], [[1]], [u])[0]
    assert one(3, -3.5, 0.99) == 0 and one(3, -1e30, 0.0) == 0            # v < -score
    assert one(24, 1.5, 0.0) == 4 * MAX and one(20, 3e38, 0.5) == 4 * MAX   # score + v > max_score
    assert one(25, 0.0, 0.999) == 100 and one(0, 0.0, 0.0) == 0            # the ends themselves
    assert _leaf([0], [0], [8], [[9.0]], [[1]], [0.3], max_score=10) == [40]


def test_leaf_ref_rounds_stochastically():
    us = (np.arange(1024) + 0.5) / 1024
    ones = np.ones(1024, np.int8)
    for score, v in ((6, 1.0), (0, 0.0), (11, -2.0), (24, 0.25)):   # x a multiple of 1 (quarter points: of 1/4 point): u does nothing
        got = _leaf(0 * ones, 0 * ones, score * ones, [[v]] * 1024, [[1]] * 1024, us)
        assert set(got) == {int(4 * (score + v))}
    for score, v in ((6, 1.3), (2, -0.77), (0, 0.0625), (20, 4.99), (13, np.float32(1e-3))):   # the clamp is inactive
        x = 4 * (score + float(np.float32(v)))
        got = _leaf(0 * ones, 0 * ones, score * ones, [[v]] * 1024, [[1]] * 1024, us)
        assert set(got) <= {int(np.floor(x)), int(np.floor(x)) + 1}
        assert abs(np.mean(got) - x) <= 1 / 1024


def test_leaf_dither_ref():
    from hanabi_hip import leaf_dither_ref

    m, R = 7, 5
    u = leaf_dither_ref(3, 11, 40, m, R)
    assert u.shape == (m, R) and u.dtype == np.float64
    assert (u >= 0).all() and (u < 1).all() and np.array_equal(u * 2 ** 24, np.floor(u * 2 ** 24))
    assert len(np.unique(u)) == m * R                      # differs across replicas (and roots)
    assert not np.array_equal(u, leaf_dither_ref(3, 12, 40, m, R)) and not np.array_equal(u, leaf_dither_ref(4, 11, 40, m, R))
    # a call split by first_row_id: the same numbers
    k = 3
    assert np.array_equal(np.concatenate([leaf_dither_ref(3, 11, 40, k, R), leaf_dither_ref(3, 11, 40 + k * R, m - k, R)]), u)
    # 64-bit seed, draw and row ids
    big = leaf_dither_ref((5 << 40) + 3, (7 << 33) + 1, (1 << 35) + 9, 2, 3)
    assert (big >= 0).all() and (big < 1).all() and len(np.unique(big)) == 6
    assert not np.array_equal(big, leaf_dither_ref(3, (7 << 33) + 1, (1 << 35) + 9, 2, 3))        # the seed's high word counts
    assert not np.array_equal(big, leaf_dither_ref((5 << 40) + 3, 1, (1 << 35) + 9, 2, 3))        # ... and the draw's
    assert not np.array_equal(big, leaf_dither_ref((5 << 40) + 3, (7 << 33) + 1, 9, 2, 3))        # ... and the row id's
    # the mean of many is 1/2: a hash, not a constant
    assert abs(leaf_dither_ref(1, 2, 0, 64, 64).mean() - 0.5) < 0.02


def test_the_dither_is_the_same_for_every_slot():
    """u is [m, R]: slot c of replica r rounds with u[i, r], so equal games of two slots get equal values."""
    from hanabi_hip import leaf_dither_ref, search_leaf_ref

    m, Cn, R = 3, 4, 6
    u = leaf_dither_ref(1, 2, 0, m, R)
    z = np.zeros((m, Cn, R), np.int8)
    q = np.full((m, Cn, R, 1), 1.37, np.float32)
    out = search_leaf_ref(z.astype(np.uint8), z, z + 5, q, np.ones((m, Cn, R, 1), np.int8), u, MAX)
    assert (out == out[:, :1]).all() and len(np.unique(out)) == 2
    assert np.array_equal(out[:, 0], np.floor(4 * (5 + np.float64(np.float32(1.37))) + u).astype(np.int8))


def test_torch_forms_give_the_numpy_forms_bits():
    import torch

    from hanabi_hip import leaf_dither, leaf_dither_ref, search_leaf, search_leaf_ref

    for args in ((3, 11, 40, 7, 5), ((5 << 40) + 3, (7 << 33) + 1, (1 << 35) + 9, 4, 3), (2 ** 64 - 1, 2 ** 64 - 1, 2 ** 40, 1, 9)):
        got = leaf_dither(*args)
        assert got.dtype == torch.float64 and np.array_equal(got.numpy(), leaf_dither_ref(*args))
    rng = np.random.default_rng(5)
    m, Cn, R, A = 5, 3, 7, 11
    done = np.where(rng.random((m, Cn, R)) < 0.3, 0x80, 0).astype(np.uint8) | rng.integers(0, 3, (m, Cn, R)).astype(np.uint8)
    fs = rng.integers(0, MAX + 1, (m, Cn, R)).astype(np.int8)
    score = rng.integers(0, MAX + 1, (m, Cn, R)).astype(np.int8)
    q = (rng.standard_normal((m, Cn, R, A)) * 4).astype(np.float32)
    q[rng.random(q.shape) < 0.05] = np.nan
    q[rng.random(q.shape) < 0.05] = np.inf
    q[rng.random(q.shape) < 0.05] = -np.inf
    q[0, 0, 0], q[0, 0, 1] = 3e38, -3e38
    legal = (rng.random((m, Cn, R, A)) < 0.5).astype(np.int8)
    legal[1, 1] = 0
    u = leaf_dither_ref(9, 4, 0, m, R)
    t = torch.from_numpy
    for qq in (q, None):
        want = search_leaf_ref(done, fs, score, qq, legal, u, MAX)
        got = search_leaf(t(done), t(fs), t(score), None if qq is None else t(qq), t(legal), t(u), MAX)
        assert got.dtype == torch.int8 and np.array_equal(got.numpy(), want)
        out = torch.empty((m, Cn, R), dtype=torch.int8)
        assert search_leaf(t(done), t(fs), t(score), None if qq is None else t(qq), t(legal), t(u), MAX, out=out) is out
        assert np.array_equal(out.numpy(), want)
    assert 0 < (want == 4 * fs).mean() < 1 and want.min() >= 0 and want.max() <= 4 * MAX


class _Q:
    """A stand-in with eval_q (never called here)."""

    def eval_moves(self, *a, **k):
        raise AssertionError("not called")

    def eval_q(self, *a, **k):
        raise AssertionError("not called")

    def requires_vectorized_observation(self):
        return True


def test_constructors_check_horizon_and_leaf():
    from types import SimpleNamespace

    from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR
    from hanabi_hip import RolloutSearch, SearchPlayer
    from hanabi_hip.search import leaf_max_score

    piers = [RulebasedAgent(PR.piers_rules, seed=11), RulebasedAgent(PR.piers_rules, seed=12)]
    for make in (lambda **kw: RolloutSearch(**kw), lambda **kw: SearchPlayer(piers, 0, leaf="score", **kw)):
        with pytest.raises(ValueError, match="horizon"):
            make(horizon=0)
        with pytest.raises(TypeError, match="horizon"):
            make(horizon=1.5)
        with pytest.raises(TypeError, match="horizon"):
            make(horizon=True)
    assert RolloutSearch().horizon is None and RolloutSearch().leaf is None and RolloutSearch(horizon=3).horizon == 3
    with pytest.raises(ValueError, match="one leaf agent per seat"):
        RolloutSearch(horizon=2, leaf=[_Q()])
    with pytest.raises(ValueError, match="one leaf agent per seat"):
        SearchPlayer(piers, 0, horizon=2, leaf=[_Q(), _Q(), _Q()])
    with pytest.raises(ValueError, match="leaf"):
        RolloutSearch(horizon=2, leaf="value")
    with pytest.raises(ValueError, match="needs horizon"):
        RolloutSearch(leaf="score")
    with pytest.raises(ValueError, match="needs horizon"):
        SearchPlayer(piers, 0, leaf="score")
    # a rule list has no q: leaf=None is refused, by name, with the alternatives
    with pytest.raises(TypeError, match="eval_q") as e:
        SearchPlayer(piers, 0, horizon=2)
    assert "RulebasedAgent" in str(e.value) and 'leaf="score"' in str(e.value) and "leaf=[" in str(e.value)
    sp = SearchPlayer(piers, 0, horizon=2, leaf="score")
    assert sp.horizon == 2 and sp.leaf == "score" and sp.leaf_games == 0
    assert SearchPlayer(piers, 0).horizon is None and SearchPlayer(piers, 0).leaf_games == 0
    assert "leaf_games" not in SearchPlayer.COUNTERS
    # only the seat that can be to act at a leaf needs eval_q: seat 0 at horizon 2 comes back to seat 0, at horizon 1 to seat 1
    SearchPlayer([_Q(), piers[1]], 0, horizon=2)
    SearchPlayer(piers, 0, horizon=1, leaf=[piers[0], _Q()])
    with pytest.raises(TypeError, match="eval_q"):
        SearchPlayer([_Q(), piers[1]], 0, horizon=1)
    # quarter points must fit int8
    assert leaf_max_score(SimpleNamespace(colors=5, ranks=5)) == 25 and leaf_max_score(SimpleNamespace(colors=1, ranks=31)) == 31
    with pytest.raises(ValueError, match="127"):
        leaf_max_score(SimpleNamespace(colors=4, ranks=8))
    import hanabi_hip

    with pytest.raises(ValueError):
        RolloutSearch(config=hanabi_hip.HbConfig(2, 6, 6, 5, 8, 3, 0), horizon=2)


@pytest.mark.parametrize("distributional", [True, False])
def test_eval_q_on_the_torch_path(distributional):
    import torch

    from hanabi_agents.rlax_dqn import ActionSpec, DQNAgent, ObservationSpec, RlaxRainbowParams
    from hanabi_agents.rlax_dqn.rlax_rainbow import DQNPolicy

    n, L, A = 33, 40, 7
    params = RlaxRainbowParams(use_priority=False, experience_buffer_size=16, layers=[24], n_atoms=11, distributional=distributional, seed=3)
    agent = DQNAgent(ObservationSpec((n, L)), ActionSpec(A), params, device="cpu")
    rng = np.random.default_rng(1)
    obs = rng.integers(0, 2, (n, L)).astype(np.int8)
    legal = (rng.random((n, A)) < 0.6).astype(np.int8)
    legal[:, 2] = 1
    draws, state = agent._draws, {k: v.clone() for k, v in agent.online.state_dict().items()}
    scratch = {}
    q = agent.eval_q((None, (obs, legal)), scratch=scratch)
    assert q.shape == (n, A) and q.dtype == torch.float32
    want = DQNPolicy.q_values(agent.online, agent.atoms, torch.from_numpy(obs).float(), torch.from_numpy(legal), distributional)
    lg = torch.from_numpy(legal) != 0
    assert torch.equal(q[lg], want.detach().float()[lg])
    # the masked arg-max (lowest uid first) is eval_moves' move, with whatever seed and draw
    moves = agent.eval_moves((None, (torch.from_numpy(obs), torch.from_numpy(legal))), 5, 9, torch.empty(n, dtype=torch.int32), scratch=scratch)
    best = torch.where(lg, q, float("-inf")).argmax(1).int()
    assert torch.equal(best, moves)
    # q_out receives a copy; nothing of the agent moved
    out = torch.empty(n, A)
    assert agent.eval_q((None, (torch.from_numpy(obs), torch.from_numpy(legal))), q_out=out) is out and torch.equal(out[lg], q[lg])
    assert agent._draws == draws and all(torch.equal(v, state[k]) for k, v in agent.online.state_dict().items())
