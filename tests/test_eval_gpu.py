"""Greedy evaluation on the GPU (hanabi_hip.evaluate): results against the CPU oracle, repeatability, and a training run that
an evaluation in the middle leaves bit-identical."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _oracle_play(game, players, n, seed, moves_of):
    """Plays n oracle games (auto-reset off) to the end; moves_of(env, t) gives turn t's moves. Returns what EvalResult holds."""
    from oracle import oracle_py as O

    cfg = O.make_config(game, players, 0)
    env = O.OracleEnv(cfg, n, seed=seed)
    H, C = cfg.hand_size, cfg.colors
    done = np.zeros(n, bool)
    lost = np.zeros(n, np.int64)
    score = np.zeros(n, np.int64)
    length = np.zeros(n, np.int64)
    moves = np.zeros((players, 4), np.int64)
    mis = np.zeros(players, np.int64)
    bomb = 0
    t = 0
    while not done.all():
        seat = t % players
        act = np.asarray(moves_of(env, t), np.int32)
        out = env.step(act)
        live = ~done
        kind = np.where(act < H, 0, np.where(act < 2 * H, 1, np.where(act < 2 * H + (players - 1) * C, 2, 3)))
        for k in range(4):
            moves[seat, k] += int(np.sum(live & (kind == k)))
        m = live & (kind == 1) & (out["reward"] <= 0)
        mis[seat] += int(m.sum())
        lost += m
        ended = live & (out["terminal"] != 0)
        score[ended] = out["score"][ended]
        length[ended] = t + 1
        bomb += int(np.sum(ended & (lost >= cfg.max_life)))
        done |= ended
        t += 1
    return dict(scores=score, lengths=length, moves=moves, misplays=mis, bombouts=bomb, illegal=env.illegal_count())


def _assert_matches(res, want, max_score):
    assert np.array_equal(res.scores.numpy(), want["scores"])
    assert np.array_equal(res.lengths.numpy(), want["lengths"])
    assert res.histogram.tolist() == np.bincount(want["scores"], minlength=max_score + 1).tolist()
    assert np.array_equal(res.moves.numpy(), want["moves"])
    assert np.array_equal(res.misplays.numpy(), want["misplays"])
    assert res.bombouts == want["bombouts"]


def _dqn(env_like, players, dtype="bfloat16", seed=1, n=None):
    from hanabi_agents.rlax_dqn import ActionSpec, DQNAgent, ObservationSpec, RlaxRainbowParams

    params = RlaxRainbowParams(train_batch_size=128, experience_buffer_size=8192, compute_dtype=dtype, packed_obs=True, layers=[512],
                               seed=seed)
    return DQNAgent(ObservationSpec((n or 1, env_like.obs_len)), ActionSpec(env_like.num_actions), params, device="cuda")


@pytest.mark.parametrize("players", [2, 4])
@pytest.mark.parametrize("team", ["piers_piers", "iggi_outer"])
def test_rule_teams_match_oracle(players, team):
    from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR
    from hanabi_hip import Evaluator

    lists = dict(piers_piers=(PR.piers_rules, PR.piers_rules), iggi_outer=(PR.iggi_rules, PR.outer_rules))[team]
    seats = [lists[s % 2] for s in range(players)]
    agents = [RulebasedAgent(r, seed=100 + s) for s, r in enumerate(seats)]
    n, seed = 2048, 21
    ev = Evaluator("Hanabi-Full", players, n_games=n, seed=seed)
    res = ev.run(agents)
    rules = [[(r.kind, r.arg, r.threshold) for r in rl] for rl in seats]
    want = _oracle_play("Hanabi-Full", players, n, seed, lambda env, t: env.rule_act(rules[t % players], seed, t + 1)[0])
    _assert_matches(res, want, 25)
    assert want["illegal"] == 0
    assert res.turns <= ev.max_turns and int(ev.counters[0]) == 0
    assert all(a._draws == 0 and a.histogram == [0] * (len(a.rules) + 1) for a in agents)   # nothing of the agents moved
    assert 10 < res.mean < 25


@pytest.mark.parametrize("players", [2, 5])
@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_dqn_actions_replay_through_oracle(players, dtype):
    import torch

    import hanabi_hip
    from hanabi_hip import Evaluator, _capi as K

    n, seed = 1024, 5
    ev = Evaluator("Hanabi-Full", players, n_games=n, seed=seed, record_actions=True)
    probe = hanabi_hip.HanabiEnv("Hanabi-Full", players, n_games=n, seed=seed, auto_reset=False, packed=True)
    agents = [_dqn(probe, players, dtype, seed=s + 1) for s in range(players)]
    res = ev.run(agents)
    assert res.actions.shape == (res.turns, n)
    acts = res.actions.numpy()
    want = _oracle_play("Hanabi-Full", players, n, seed, lambda env, t: acts[t])
    _assert_matches(res, want, 25)
    # the moves are those of a hand loop of the one-kernel actor with epsilon 0 and the evaluator's seed / draw
    L = K.lib()
    q = torch.empty(n, probe.num_actions, dtype=torch.float32, device="cuda")
    out = torch.empty(n, dtype=torch.int32, device="cuda")
    for t in range(res.turns):
        a = agents[t % players]
        act = a._fl.actor
        f = act._fset_ptrs[0]
        K.check(L.hb_actor_fused_act_dt(probe.obs_bits.data_ptr(), probe.legal.data_ptr(), n, probe.obs_len, f[0], f[1], f[2], f[3],
                                        a.atoms[0].contiguous().data_ptr(), act.hidden, act.n_actions, act.n_atoms, q.data_ptr(), 0.0,
                                        seed, t + 1, 0, out.data_ptr(), act._dt, K.current_stream()))
        assert torch.equal(out.cpu(), res.actions[t]), f"turn {t}"
        probe.step(out)
    assert all(a._draws == 0 for a in agents) and agents[0]._fl.actor.q is None   # the actor's own buffers were never allocated


def test_repeatable_and_seeded():
    import torch

    import hanabi_hip
    from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR
    from hanabi_hip import Evaluator

    probe = hanabi_hip.HanabiEnv("Hanabi-Full", 2, n_games=1, auto_reset=False, packed=True)
    agents = [_dqn(probe, 2, seed=3), RulebasedAgent(PR.piers_rules)]
    ev = Evaluator("Hanabi-Full", 2, n_games=4096, seed=9, record_actions=True)
    a, b = ev.run(agents), ev.run(agents)
    for x, y in ((a.scores, b.scores), (a.lengths, b.lengths), (a.histogram, b.histogram), (a.moves, b.moves), (a.actions, b.actions)):
        assert torch.equal(x, y)
    assert a.as_dict() == b.as_dict()
    other = Evaluator("Hanabi-Full", 2, n_games=4096, seed=10)
    c = other.run(agents)
    assert not torch.equal(ev.rows0, other.rows0)
    assert not torch.equal(a.lengths, c.lengths)   # (an untrained agent bombs out: the scores alone may all be 0)


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


@pytest.mark.parametrize("kind", ["rainbow_chain", "vanilla", "rule_partner"])
def test_evaluation_leaves_training_untouched(kind, monkeypatch):
    """Session A trains 20 steps, evaluates on 1000 games (another size than training on purpose), trains 20 more; session B
    trains 40 steps. Both end bit-identical: weights, Adam moments, replay, sum tree, env rows, episode stats, draw counters."""
    import torch

    import hanabi_hip
    from hanabi_agents.rlax_dqn import ActionSpec, DQNAgent, ObservationSpec, RlaxRainbowParams
    from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR
    from hanabi_hip.selfplay import SelfPlaySession

    monkeypatch.setenv("HB_ACTOR_FUSED_MIN_ROWS", "0")
    n = 1024

    def session():
        torch.manual_seed(0)
        torch.cuda.manual_seed(0)
        flags = hanabi_hip.FLAG_AUTO_RESET | hanabi_hip.FLAG_RESET_START_NEXT
        env = hanabi_hip.HanabiEnv(config=hanabi_hip.make_config("Hanabi-Full", 2, flags), n_games=n, seed=5, packed=True)
        if kind == "vanilla":
            params = RlaxRainbowParams(train_batch_size=128, experience_buffer_size=n * 8, compute_dtype="bfloat16", packed_obs=True,
                                       layers=[512], distributional=False, use_priority=False, target_update_period=6)
        else:
            params = RlaxRainbowParams(train_batch_size=128, experience_buffer_size=n * 8, mask_terminal=True, target_update_period=6,
                                       compute_dtype="bfloat16", packed_obs=True, layers=[512], learning_rate=0.01)
        mk = lambda s: DQNAgent(ObservationSpec((n, env.obs_len)), ActionSpec(env.num_actions), params._replace(seed=s), device="cuda")
        agents = [mk(1), RulebasedAgent(PR.piers_rules, seed=4)] if kind == "rule_partner" else [mk(1), mk(2)]
        return SelfPlaySession(env, agents)

    a = session()
    r0 = a.evaluate(n_games=1000, seed=3)    # (fresh agents: the first call builds the FusedLearner as a first act would)
    a.run(20)
    r1 = a.evaluate(n_games=1000, seed=3)
    a.run(20)
    r2 = a.evaluate(n_games=1000, seed=3)    # (the cached evaluator, weights 20 steps later)
    state_a = _session_state(a)
    b = session()
    b.run(40)
    state_b = _session_state(b)
    if kind == "rainbow_chain":
        assert a.native_steps > 10 and b.native_steps > 10
    _assert_same(state_a, state_b)
    assert r0.n_games == r1.n_games == r2.n_games == 1000 and r1.moves.sum() > 0
    if kind == "rule_partner":
        assert a.agents[1].histogram == b.agents[1].histogram and sum(a.agents[1].histogram) == 20 * n
    # the evaluation of B's final weights equals A's second one
    r3 = b.evaluate(n_games=1000, seed=3)
    assert torch.equal(r2.scores, r3.scores) and torch.equal(r2.lengths, r3.lengths)


def test_large_untrained_team_finishes():
    import hanabi_hip
    from hanabi_hip import Evaluator

    n = 32768
    probe = hanabi_hip.HanabiEnv("Hanabi-Full", 2, n_games=1, auto_reset=False, packed=True)
    ev = Evaluator("Hanabi-Full", 2, n_games=n, seed=2)
    res = ev.run([_dqn(probe, 2, seed=1), _dqn(probe, 2, seed=2)])
    # (the run raises if games are still live at the cap; the live count is read every 8 turns, so `turns` may reach it)
    assert res.turns <= ev.max_turns and int(ev.counters[0]) == 0
    assert int(res.lengths.min()) >= 1 and int(res.lengths.max()) <= min(res.turns, ev.max_turns)
    assert int(res.histogram.sum()) == n
    assert int(res.moves.sum()) == int(res.lengths.sum())
    assert ev.env.illegal_count() == 0


def _team_result(ev, agent):
    res = ev.run([agent, agent])
    return res.actions.clone(), res.scores.clone(), res.lengths.clone()


@pytest.mark.parametrize("family", ["c51", "vanilla"])
def test_agents_of_other_shapes_one_after_another(family):
    """One Evaluator, agents of different hidden size / atom count / support evaluated in turn, each dropped before the next is
    made (CPython then tends to hand the next agent the dead one's id): every result equals a fresh Evaluator's."""
    import gc

    import torch

    import hanabi_hip
    from hanabi_agents.rlax_dqn import ActionSpec, DQNAgent, ObservationSpec, RlaxRainbowParams
    from hanabi_hip import Evaluator

    probe = hanabi_hip.HanabiEnv("Hanabi-Full", 2, n_games=1, auto_reset=False, packed=True)
    if family == "c51":   # one-kernel actor (h: one row), then the two-kernel form with 21 atoms, then a wider two-kernel hidden layer
        shapes = [dict(layers=[512]), dict(layers=[256], n_atoms=21, atom_vmax=10), dict(layers=[768], atom_vmax=40)]
    else:
        shapes = [dict(layers=[256]), dict(layers=[768]), dict(layers=[512])]
    extra = dict(distributional=False, use_priority=False) if family == "vanilla" else {}
    shared = Evaluator("Hanabi-Full", 2, n_games=1500, seed=4, record_actions=True)
    for k, shape in enumerate(shapes):
        params = RlaxRainbowParams(compute_dtype="bfloat16", packed_obs=True, experience_buffer_size=1024, seed=10 + k, **extra, **shape)
        agent = DQNAgent(ObservationSpec((1, probe.obs_len)), ActionSpec(probe.num_actions), params, device="cuda")
        got = _team_result(shared, agent)
        want = _team_result(Evaluator("Hanabi-Full", 2, n_games=1500, seed=4, record_actions=True), agent)
        for x, y in zip(got, want):
            assert torch.equal(x, y), shape
        assert len(shared._scratch) == 1
        del agent
        gc.collect()
        assert len(shared._scratch) == 0   # (the dead agent's buffers went with it)


@pytest.mark.parametrize("path", ["library_gemm", "torch"])
def test_fallback_paths_match_exploit(path):
    """Agents off the MFMA kernels: the library-GEMM form (hb_policy_act) and the torch path with its seeded generator. Their
    evaluation moves equal exploit() on the same positions, and neither the agent's generator nor the device's moves."""
    import torch

    import hanabi_hip
    from hanabi_agents.rlax_dqn import ActionSpec, DQNAgent, ObservationSpec, RlaxRainbowParams
    from hanabi_hip import Evaluator

    n, seed = 512, 6
    probe = hanabi_hip.HanabiEnv("Hanabi-Full", 2, n_games=n, seed=seed, auto_reset=False, packed=True)
    if path == "library_gemm":
        params = RlaxRainbowParams(compute_dtype="bfloat16", packed_obs=True, experience_buffer_size=1024)
    else:
        params = RlaxRainbowParams(compute_dtype="float32", distributional=False, use_priority=False, experience_buffer_size=1024)
    agent = DQNAgent(ObservationSpec((n, probe.obs_len)), ActionSpec(probe.num_actions), params, device="cuda")
    if path == "library_gemm":
        agent.use_mfma_actor = False
    else:
        assert not agent._fused and not agent._plain_fast
    gen0, rng0 = agent._gen.get_state().clone(), torch.cuda.get_rng_state().clone()
    res = Evaluator("Hanabi-Full", 2, n_games=n, seed=seed, record_actions=True).run([agent, agent])
    assert agent._draws == 0 and torch.equal(agent._gen.get_state(), gen0) and torch.equal(torch.cuda.get_rng_state(), rng0)
    assert res.turns > 20
    for t in range(res.turns):
        live = res.lengths > t
        want = agent.exploit((probe, (probe.net_obs, probe.legal))).cpu()
        assert torch.equal(want[live], res.actions[t][live]), f"turn {t}"
        probe.step(res.actions[t].cuda())
    assert probe.illegal_count() == 0


@pytest.mark.parametrize("kind", ["rainbow_chain", "vanilla"])
def test_exploit_at_another_size_keeps_training_exact(kind, monkeypatch):
    """exploit() on an env of another size in the middle of training (the hand-rolled evaluation pattern) re-allocates the actor's
    q (one-kernel actor) or the vanilla actor's hidden buffer. The one-call step's command array must not keep the old q address,
    the vanilla actor's captured graph must not keep the old hidden buffer, and training continues exactly as without it."""
    import torch

    import hanabi_hip
    from hanabi_agents.rlax_dqn import ActionSpec, DQNAgent, ObservationSpec, RlaxRainbowParams
    from hanabi_hip import _capi as K
    from hanabi_hip.selfplay import SelfPlaySession

    monkeypatch.setenv("HB_ACTOR_FUSED_MIN_ROWS", "0")
    n = 1024

    def session():
        torch.manual_seed(0)
        torch.cuda.manual_seed(0)
        flags = hanabi_hip.FLAG_AUTO_RESET | hanabi_hip.FLAG_RESET_START_NEXT
        env = hanabi_hip.HanabiEnv(config=hanabi_hip.make_config("Hanabi-Full", 2, flags), n_games=n, seed=5, packed=True)
        extra = dict(distributional=False, use_priority=False) if kind == "vanilla" else dict(mask_terminal=True, learning_rate=0.01)
        params = RlaxRainbowParams(train_batch_size=128, experience_buffer_size=n * 8, target_update_period=6, compute_dtype="bfloat16",
                                   packed_obs=True, layers=[512], **extra)
        mk = lambda s: DQNAgent(ObservationSpec((n, env.obs_len)), ActionSpec(env.num_actions), params._replace(seed=s), device="cuda")
        return SelfPlaySession(env, [mk(1), mk(2)])

    a = session()
    a.run(20)
    agent = a.agents[0]
    other = hanabi_hip.HanabiEnv("Hanabi-Full", 2, n_games=700, seed=9, packed=True)
    if kind == "vanilla":
        assert agent._plain_actor.graph is not None   # (the captured forward the stale buffer would be replayed through)
    else:
        assert a.native_steps > 0 and agent._fl.actor.q.shape[0] == n
    draws = agent._draws
    agent.exploit((other, (other.net_obs, other.legal)))
    torch.cuda.synchronize()
    agent._draws = draws   # (exploit's draw counter step is not what this test is about)
    if kind == "vanilla":
        assert agent._plain_actor.graph is None and agent._plain_actor.h.shape[0] == 700
    else:
        assert agent._fl.actor.q.shape[0] == 700   # (re-allocated: the training-size buffer q_train pointed to is freed)
    del other
    a.run(20)
    if kind == "rainbow_chain":
        q_now = agent._fl.actor.q
        assert q_now.shape[0] == n
        ch = a._chains[(0, 0)]
        acts = [ch.cmds[i] for i in range(ch.count) if ch.cmds[i].op == K.CMD_ACTOR_FUSED_ACT]
        assert len(acts) == 1 and acts[0].p[7] == q_now.data_ptr()   # the command array writes into the live q buffer
    state_a = _session_state(a)
    b = session()
    b.run(40)
    _assert_same(state_a, _session_state(b))
