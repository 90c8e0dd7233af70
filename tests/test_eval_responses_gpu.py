"""Partner-response (convention) statistics on the GPU (csrc/eval.hip: hb_eval_response_tally and its grouped form;
hanabi_hip.evaluate / crossplay / selfplay with responses=True): the kernels against a per-game numpy model at every shape that
takes another path, whole evaluations against `response_counts` over their recorded moves, cross-play teams against their
standalone evaluations, and a training session that an evaluation with the switch on leaves bit-identical."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GAMES = [("Hanabi-Small", 2, 11), ("Hanabi-Full", 2, 20), ("Hanabi-Full", 5, 48)]   # (game, players, A); A = 48: the largest histogram


def _model(actions, done, prev, resp, seat, A):
    """One hb_eval_response_tally call, game by game: returns the new (prev, resp)."""
    prev, resp = prev.copy(), resp.copy()
    for g in range(actions.shape[0]):
        u = int(actions[g])
        if done[g] & 0x80 or u < 0 or u >= A:
            continue
        resp[seat, prev[g] + 1, u] += 1
        prev[g] = u
    return prev, resp


def _call(L, cfg, n, seat, actions, done, prev, resp):
    from hanabi_hip import _capi as K

    K.check(L.hb_eval_response_tally(C.byref(cfg), n, seat, actions.data_ptr(), done.data_ptr(), prev.data_ptr(), resp.data_ptr(),
                                     K.current_stream()))


def _inputs(rng, n, A):
    """A mixed status pattern (bit 7 on some games, lower bits on live and finished ones), prev of -1 and valid uids, and two
    turns of moves with uids outside 0 .. A-1 among them."""
    done = rng.choice(np.array([0, 1, 2, 0x7f, 0x80, 0x81, 0xff], np.uint8), n)
    done[0] = 0x7f                     # live, every lower bit set: only bit 7 counts
    if n > 1:
        done[1] = 0x83                 # finished
    prev = rng.integers(-1, A, n).astype(np.int32)
    prev[0] = -1
    if n > 2:
        prev[2], done[2] = A - 1, 0    # the last row of the slab
    acts = [rng.integers(0, A, n).astype(np.int32) for _ in range(2)]
    acts[1][0] = A                     # (n = 1: the lone lane plays a move in turn 1 and none in turn 2)
    if n > 2:
        acts[0][2], acts[1][2] = A - 1, -1
        acts[0][n - 1], done[n - 1] = A + 7, 0
        acts[0][n // 2], done[n // 2] = -3, 1
    return done, prev, acts


@pytest.mark.parametrize("game,players,A", GAMES)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
def test_kernel_matches_numpy_model(game, players, A, n):
    """n = 1: a lone lane; 63 / 64 / 65: a wavefront boundary; 300: two workgroups, the last one partial. Two consecutive calls
    (the second reads the prev the first wrote, for another seat), then every game finished, then n = 0."""
    _check_kernel(game, players, A, n)


def test_kernel_grid_stride_second_pass():
    """128 workgroups of 256 lanes cover 32 768 games: 70 more take each lane's loop round again (in 1 workgroup of the 128)."""
    _check_kernel("Hanabi-Full", 2, 20, 128 * 256 + 70)


def _check_kernel(game, players, A, n):
    import torch

    import hanabi_hip

    L = hanabi_hip.lib()
    cfg = hanabi_hip.make_config(game, players)
    assert L.hb_num_actions(C.byref(cfg)) == A and L.hb_eval_response_bins(C.byref(cfg)) == (A + 1) * A
    rng = np.random.default_rng(1000 * A + n)
    done, prev, acts = _inputs(rng, n, A)
    # counts so far: just below 2^32, so that the first adds carry into the high word of the int64 bins
    resp = (1 << 32) - 1 - rng.integers(0, 3, (players, A + 1, A)).astype(np.int64)
    d_done, d_prev, d_resp = (torch.from_numpy(x).cuda() for x in (done, prev, resp))
    for seat, a in zip((players - 1, 0), acts):
        prev, resp = _model(a, done, prev, resp, seat, A)
        _call(L, cfg, n, seat, torch.from_numpy(a).cuda(), d_done, d_prev, d_resp)
        assert np.array_equal(d_prev.cpu().numpy(), prev), seat
        assert np.array_equal(d_resp.cpu().numpy(), resp), seat
        assert np.array_equal(d_done.cpu().numpy(), done)            # read only
    live = int(((done & 0x80) == 0).sum())
    assert live >= 1 and (n < 3 or live < n)
    # every game finished: nothing changes
    fin = torch.from_numpy(done | 0x80).cuda()
    a = torch.from_numpy(rng.integers(0, A, n).astype(np.int32)).cuda()
    _call(L, cfg, n, 0, a, fin, d_prev, d_resp)
    assert np.array_equal(d_prev.cpu().numpy(), prev) and np.array_equal(d_resp.cpu().numpy(), resp)
    # n = 0: a no-op
    _call(L, cfg, 0, 0, a, d_done, d_prev, d_resp)
    assert np.array_equal(d_prev.cpu().numpy(), prev) and np.array_equal(d_resp.cpu().numpy(), resp)


@pytest.mark.parametrize("game,players,A", [GAMES[0], GAMES[2]])
def test_grouped_equals_single_calls_on_the_slices(game, players, A):
    """3 blocks of 70 games, two turns: per block, counts and prev equal hb_eval_response_tally on that block's slices; the
    block whose games are all finished stays zero."""
    import torch

    import hanabi_hip
    from hanabi_hip import _capi as K

    L = hanabi_hip.lib()
    cfg = hanabi_hip.make_config(game, players)
    nb, bg = 3, 70
    rng = np.random.default_rng(A)
    done = rng.choice(np.array([0, 3, 0x80, 0x82], np.uint8), nb * bg)
    done[bg:2 * bg] |= 0x80                                   # block 1: every game finished
    done[0], done[2 * bg] = 0, 1
    prev0 = rng.integers(-1, A, nb * bg).astype(np.int32)
    g_done = torch.from_numpy(done).cuda()
    g_prev, s_prev = torch.from_numpy(prev0).cuda(), torch.from_numpy(prev0).cuda()
    g_resp = torch.zeros(nb, players, A + 1, A, dtype=torch.int64, device="cuda")
    s_resp = torch.zeros_like(g_resp)
    prev, resp = prev0, np.zeros((nb, players, A + 1, A), np.int64)
    for seat in (players - 1, 0):
        a = rng.integers(-1, A + 1, nb * bg).astype(np.int32)     # (-1 and A: not moves)
        act = torch.from_numpy(a).cuda()
        K.check(L.hb_eval_response_tally_grouped(C.byref(cfg), nb, bg, seat, act.data_ptr(), g_done.data_ptr(), g_prev.data_ptr(),
                                                 g_resp.data_ptr(), K.current_stream()))
        new_prev = prev.copy()
        for b in range(nb):
            o = b * bg
            K.check(L.hb_eval_response_tally(C.byref(cfg), bg, seat, act.data_ptr() + 4 * o, g_done.data_ptr() + o,
                                             s_prev.data_ptr() + 4 * o, s_resp[b].data_ptr(), K.current_stream()))
            new_prev[o:o + bg], resp[b] = _model(a[o:o + bg], done[o:o + bg], prev[o:o + bg], resp[b], seat, A)
        prev = new_prev
        assert torch.equal(g_resp, s_resp) and torch.equal(g_prev, s_prev), seat
        assert np.array_equal(g_resp.cpu().numpy(), resp) and np.array_equal(g_prev.cpu().numpy(), prev), seat
    assert not g_resp[1].any() and g_resp[0].any() and g_resp[2].any()
    assert np.array_equal(g_prev.cpu().numpy()[bg:2 * bg], prev0[bg:2 * bg])


# ---- whole evaluations -------------------------------------------------------------------------------------------------------

def _piers(k):
    from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR

    return [RulebasedAgent(PR.piers_rules, seed=50 + s) for s in range(k)]


def _assert_same_outcome(got, want):
    import torch

    for name in ("scores", "lengths", "histogram", "moves", "misplays"):
        assert torch.equal(getattr(got, name), getattr(want, name)), name
    assert got.bombouts == want.bombouts and got.turns == want.turns


@pytest.mark.parametrize("game,players,n", [("Hanabi-Small", 2, 200), ("Hanabi-Full", 5, 130)])
def test_evaluator_responses_equal_recorded_moves(game, players, n):
    import torch

    from hanabi_hip import Evaluator
    from hanabi_hip.evaluate import response_counts

    team = _piers(players)
    ev = Evaluator(game, players, n_games=n, seed=17, record_actions=True, responses=True)
    res = ev.run(team)
    A = ev.env.num_actions
    assert res.responses.dtype == np.int64 and res.responses.shape == (players, A + 1, A)
    want = response_counts(res.actions.numpy(), res.lengths.numpy(), players, A)
    assert np.array_equal(res.responses, want)
    for seat in range(players):   # every counted move is one of the seat's four move kinds
        assert int(res.responses[seat].sum()) == int(res.moves[seat].sum())
    assert int(res.responses.sum()) == int(res.lengths.sum()) and int(res.responses[:, 0].sum()) == n
    m = res.response_matrix()
    assert np.allclose(m[~np.isnan(m).any(-1)].sum(-1), 1.0, rtol=0, atol=1e-12)
    assert res.response_matrix(kinds=True).shape == (5, 4) and "responses" in res.as_dict()
    # the switch changes nothing else, bit for bit; a second run gives the same counts (prev and the counts are reset)
    off = Evaluator(game, players, n_games=n, seed=17, record_actions=True).run(team)
    assert off.responses is None and "responses" not in off.as_dict()
    _assert_same_outcome(res, off)
    assert torch.equal(res.actions, off.actions)
    assert np.array_equal(ev.run(team).responses, want)


def test_crossplay_slabs_equal_standalone_evaluations():
    import torch

    from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR
    from hanabi_hip import CrossPlay, Evaluator

    pool = [RulebasedAgent(r, seed=60 + k) for k, r in enumerate((PR.piers_rules, PR.iggi_rules, PR.outer_rules))]
    n, seed = 70, 23
    res = CrossPlay("Hanabi-Full", players=2, n_games=n, seed=seed, responses=True).run(pool)
    assert len(res.teams) == 9 and res.responses.shape == (9, 2, 21, 20)
    for k, (team, got) in enumerate(zip(res.teams, res.results)):
        want = Evaluator("Hanabi-Full", 2, n_games=n, seed=seed, responses=True).run([pool[i] for i in team])
        assert np.array_equal(got.responses, want.responses), team
        assert np.array_equal(res.responses[k], want.responses), team
        _assert_same_outcome(got, want)
    off = CrossPlay("Hanabi-Full", players=2, n_games=n, seed=seed).run(pool)
    assert off.responses is None and all(r.responses is None for r in off.results)
    assert torch.equal(res.mean_matrix(), off.mean_matrix())
    for got, want in zip(res.results, off.results):
        _assert_same_outcome(got, want)
    d = res.convention_distance()
    assert d.shape == (9, 9) and np.array_equal(d, d.T) and np.array_equal(np.diag(d), np.zeros(9))
    assert (d >= 0).all() and (d <= 1).all()
    assert d[0, 4] > 0      # Piers with itself and IGGI with itself do not answer alike


def _dqn(env_like, players, dtype="bfloat16", seed=1, n=None):
    from hanabi_agents.rlax_dqn import ActionSpec, DQNAgent, ObservationSpec, RlaxRainbowParams

    params = RlaxRainbowParams(train_batch_size=128, experience_buffer_size=8192, compute_dtype=dtype, packed_obs=True, layers=[512],
                               seed=seed)
    return DQNAgent(ObservationSpec((n or 1, env_like.obs_len)), ActionSpec(env_like.num_actions), params, device="cuda")


def test_dqn_seat_with_the_switch_on():
    """A bf16 DQN agent in seat 0 (the vectorised-observation path of Evaluator.run), Piers in seat 1."""
    import hanabi_hip
    from hanabi_hip import Evaluator
    from hanabi_hip.evaluate import response_counts

    n = 200
    probe = hanabi_hip.HanabiEnv("Hanabi-Small", 2, n_games=1, auto_reset=False, packed=True)
    team = [_dqn(probe, 2, seed=3), _piers(1)[0]]
    res = Evaluator("Hanabi-Small", 2, n_games=n, seed=5, record_actions=True, responses=True).run(team)
    assert np.array_equal(res.responses, response_counts(res.actions.numpy(), res.lengths.numpy(), 2, probe.num_actions))
    assert [int(res.responses[s].sum()) for s in range(2)] == res.moves.sum(1).tolist()
    off = Evaluator("Hanabi-Small", 2, n_games=n, seed=5, record_actions=True).run(team)
    _assert_same_outcome(res, off)
    assert team[0]._draws == 0


def _session_state(sess):
    import torch

    torch.cuda.synchronize()
    return sess.checkpoint_state(include_replay=True)


def _assert_same(x, y, path="state"):
    import torch

    if isinstance(x, dict):
        assert x.keys() == y.keys(), path
        for k in x:
            if k == "params":   # (a repr holding the addresses of the epsilon / beta lambdas)
                continue
            _assert_same(x[k], y[k], f"{path}.{k}")
    elif isinstance(x, (list, tuple)):
        assert len(x) == len(y), path
        for i, (u, v) in enumerate(zip(x, y)):
            _assert_same(u, v, f"{path}[{i}]")
    elif isinstance(x, torch.Tensor):
        assert torch.equal(x, y), path
    else:
        assert x == y, path


def test_session_evaluate_with_responses_leaves_training_untouched(monkeypatch):
    """Session A trains 20 steps, evaluates and cross-plays with responses=True, trains 20 more; session B trains 40 steps. Both
    end bit-identical, and the switch changes no outcome of the evaluation."""
    import torch

    import hanabi_hip
    from hanabi_agents.rlax_dqn import ActionSpec, DQNAgent, ObservationSpec, RlaxRainbowParams
    from hanabi_hip.selfplay import SelfPlaySession

    monkeypatch.setenv("HB_ACTOR_FUSED_MIN_ROWS", "0")
    n = 1024

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
    r_on = a.evaluate(n_games=300, seed=3, responses=True)
    r_off = a.evaluate(n_games=300, seed=3)
    cp = a.crossplay(a.agents + _piers(1), n_games=70, seed=3, responses=True)
    a.run(20)
    state_a = _session_state(a)
    b = session()
    b.run(40)
    _assert_same(state_a, _session_state(b))
    assert r_on.responses.shape == (2, 21, 20) and int(r_on.responses.sum()) == int(r_on.lengths.sum())
    assert r_off.responses is None
    _assert_same_outcome(r_on, r_off)
    assert cp.responses.shape == (9, 2, 21, 20) and cp.convention_distance().shape == (9, 9)
    assert int(cp.results[1].responses[0].sum()) == int(cp.results[1].moves[0].sum())
