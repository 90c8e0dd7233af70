"""Cross-play on the GPU (hanabi_hip.crossplay): the three grouped kernels against their single-block counterparts on the same
inputs, every team of a mixed pool against a standalone Evaluator, the generic path, chunking, repeatability, and a training run
that a cross-play in the middle leaves bit-identical."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu


def _dqn(obs_len, n_actions, dtype="bfloat16", seed=1, **extra):
    from hanabi_agents.rlax_dqn import ActionSpec, DQNAgent, ObservationSpec, RlaxRainbowParams

    params = RlaxRainbowParams(train_batch_size=128, experience_buffer_size=1024, compute_dtype=dtype, packed_obs=True, layers=[512],
                               seed=seed, **extra)
    return DQNAgent(ObservationSpec((1, obs_len)), ActionSpec(n_actions), params, device="cuda")


def _played_env(players, n, seed, turns):
    """A packed env (auto-reset off) after `turns` random legal moves: positions of every phase."""
    import hanabi_hip

    env = hanabi_hip.HanabiEnv("Hanabi-Full", players, n_games=n, seed=seed, auto_reset=False, packed=True)
    for t in range(turns):
        env.step(env.random_legal_actions(seed=seed + 1, draw=t))
    return env


def _assert_same_result(got, want, what=""):
    import torch

    assert torch.equal(got.scores, want.scores), what
    assert torch.equal(got.lengths, want.lengths), what
    assert torch.equal(got.histogram, want.histogram), what
    assert got.bombouts == want.bombouts, what
    assert torch.equal(got.moves, want.moves), what
    assert torch.equal(got.misplays, want.misplays), what
    assert got.turns == want.turns, what
    if want.actions is not None:
        assert torch.equal(got.actions, want.actions), what


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


# ---- kernel level ------------------------------------------------------------------------------------------------------------

def test_actor_grouped_matches_single_network_launches():
    """Three networks (two bf16, one fp16) and inactive tiles over 10 tiles: a bf16 and an fp16 launch with complementary active
    tiles. Active rows equal hb_actor_fused_act_dt over the same rows with that tile's weights and game id; inactive rows keep
    the sentinel."""
    import torch

    from hanabi_hip import _capi as K

    L = K.lib()
    n = 10 * 128
    env = _played_env(2, n, 3, 12)
    A, obs_len = env.num_actions, env.obs_len
    nets = [_dqn(obs_len, A, "bfloat16", seed=1), _dqn(obs_len, A, "bfloat16", seed=2), _dqn(obs_len, A, "float16", seed=3)]
    ops = [a.eval_operands() for a in nets]
    assert [o["dtype"] for o in ops] == [1, 1, 2]
    owner = [0, 0, 1, None, 2, 2, 0, None, 1, 2]     # tile -> network (None: inactive in both launches)
    gid0 = [1000 + 37 * t for t in range(10)]          # arbitrary per-tile game ids
    seed, draw, eps = 77, 5, 0.3                       # (eps > 0: the Philox draws of the selection matter)
    tabs = {}
    for dt in (1, 2):
        tab = (K.HbFusedTile * 10)()
        for t, o in enumerate(owner):
            if o is not None and ops[o]["dtype"] == dt:
                d, op = tab[t], ops[o]
                d.w1f, d.b1f, d.w2f, d.b2f, d.support = op["w1f"], op["b1f"], op["w2f"], op["b2f"], op["support"]
                d.first_game_id, d.active = gid0[t], 1
        tabs[dt] = torch.frombuffer(bytearray(tab), dtype=torch.uint8).cuda()
    q = torch.full((n, A), float("nan"), device="cuda")
    acts = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    for dt in (1, 2):
        K.check(L.hb_actor_fused_act_grouped(tabs[dt].data_ptr(), n, env.obs_bits.data_ptr(), env.legal.data_ptr(), obs_len, 512, A, 51,
                                             q.data_ptr(), eps, seed, draw, acts.data_ptr(), dt, K.current_stream()))
    words = env.obs_bits.shape[1]
    for t, o in enumerate(owner):
        rows = slice(128 * t, 128 * t + 128)
        if o is None:
            assert torch.isnan(q[rows]).all() and (acts[rows] == -7).all(), t
            continue
        op = ops[o]
        qr = torch.empty(128, A, device="cuda")
        ar = torch.empty(128, dtype=torch.int32, device="cuda")
        K.check(L.hb_actor_fused_act_dt(env.obs_bits.data_ptr() + 4 * words * 128 * t, env.legal.data_ptr() + A * 128 * t, 128, obs_len,
                                        op["w1f"], op["b1f"], op["w2f"], op["b2f"], op["support"], 512, A, 51, qr.data_ptr(), eps, seed,
                                        draw, gid0[t], ar.data_ptr(), op["dtype"], K.current_stream()))
        assert torch.equal(q[rows], qr), t
        assert torch.equal(acts[rows], ar), t
    assert all(a._draws == 0 for a in nets)


@pytest.mark.parametrize("br,fgid", [(200, 11), (130, 2**32 - 7)])
def test_rule_grouped_matches_single_block_launches(br, fgid):
    """Four rule sets over seven blocks of `br` games (three skipped: two of set -1, one of set n_sets): each block equals
    hb_rule_act on its rows with its rule set. 130 rows: one full workgroup and a 2-lane tail, with game ids that cross 2^32."""
    import torch

    from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR
    from hanabi_hip import _capi as K

    L = K.lib()
    sets_of_block = [0, -1, 1, 2, -1, 3, 4]
    nb = len(sets_of_block)
    env = _played_env(3, nb * br, 8, 9)
    agents = [RulebasedAgent(r) for r in (PR.piers_rules, PR.iggi_rules, PR.outer_rules, PR.flawed_rules)]
    tab = (K.HbRule * (K.MAX_RULES * 4))()
    for s, a in enumerate(agents):
        for i in range(len(a.rules)):
            tab[s * K.MAX_RULES + i] = a._tab[i]
    rules_dev = torch.frombuffer(bytearray(tab), dtype=torch.uint8).cuda()
    n_rules = torch.tensor([len(a.rules) for a in agents], dtype=torch.int32, device="cuda")
    sob = torch.tensor(sets_of_block, dtype=torch.int32, device="cuda")
    acts = torch.full((nb * br,), -7, dtype=torch.int32, device="cuda")
    fired = torch.full((nb * br,), -9, dtype=torch.int32, device="cuda")
    state = L.hb_env_state(env.h)
    cfg = C.byref(env.cfg)
    seed, draw = 123, 4
    K.check(L.hb_rule_act_grouped(cfg, state, nb, br, fgid, sob.data_ptr(), rules_dev.data_ptr(), n_rules.data_ptr(), 4, seed, draw,
                                  acts.data_ptr(), fired.data_ptr(), K.current_stream()))
    for b, s in enumerate(sets_of_block):
        rows = slice(b * br, b * br + br)
        if s < 0 or s >= 4:
            assert (acts[rows] == -7).all() and (fired[rows] == -9).all(), b
            continue
        a = agents[s]
        ar = torch.empty(br, dtype=torch.int32, device="cuda")
        fr = torch.empty(br, dtype=torch.int32, device="cuda")
        K.check(L.hb_rule_act(cfg, state + 4 * env.state_words * b * br, br, fgid, a._tab, len(a.rules), seed, draw, ar.data_ptr(),
                              fr.data_ptr(), K.current_stream()))
        assert torch.equal(acts[rows], ar), b
        assert torch.equal(fired[rows], fr), b
    assert all(a._draws == 0 and a.histogram == [0] * (len(a.rules) + 1) for a in agents)


def test_tally_grouped_matches_per_block_tally():
    """Three blocks of 300 games played to the end with random legal moves: per block, the grouped tally's counters, done,
    final score and length equal hb_eval_tally run on that block alone, after every turn."""
    import torch

    import hanabi_hip
    from hanabi_hip import _capi as K

    L = K.lib()
    nb, n, P = 3, 300, 2
    env = hanabi_hip.HanabiEnv("Hanabi-Full", P, n_games=nb * n, seed=6, auto_reset=False, packed=True)
    nc = L.hb_eval_counters(C.byref(env.cfg))

    def bufs():
        done = torch.zeros(nb * n, dtype=torch.uint8, device="cuda")
        done[n - 20:n] = 0x80   # (finished rows are ignored: as the padding rows of a cross-play block)
        counters = torch.zeros(nb, nc, dtype=torch.int64, device="cuda")
        counters[:, 0] = n
        counters[0, 0] = n - 20
        return dict(done=done, fs=torch.zeros(nb * n, dtype=torch.int8, device="cuda"),
                    ln=torch.zeros(nb * n, dtype=torch.int16, device="cuda"), c=counters)

    g, s = bufs(), bufs()
    cfg = C.byref(env.cfg)
    for t in range(200):
        act = env.random_legal_actions(seed=9, draw=t)
        env.step(act)
        K.check(L.hb_eval_tally_grouped(cfg, nb, n, t % P, t, act.data_ptr(), env.reward.data_ptr(), env.terminal.data_ptr(),
                                        env.score.data_ptr(), g["done"].data_ptr(), g["fs"].data_ptr(), g["ln"].data_ptr(), g["c"].data_ptr(),
                                        K.current_stream()))
        for b in range(nb):
            o = b * n
            K.check(L.hb_eval_tally(cfg, n, t % P, t, act.data_ptr() + 4 * o, env.reward.data_ptr() + 4 * o, env.terminal.data_ptr() + o,
                                    env.score.data_ptr() + o, s["done"].data_ptr() + o, s["fs"].data_ptr() + o, s["ln"].data_ptr() + 2 * o,
                                    s["c"][b].data_ptr(), K.current_stream()))
        for k in g:
            assert torch.equal(g[k], s[k]), (t, k)
        if int(g["c"][:, 0].sum()) == 0:
            break
    assert int(g["c"][:, 0].sum()) == 0 and int(g["c"][:, 1:27].sum()) == nb * n - 20


# ---- CrossPlay against the standalone Evaluator ------------------------------------------------------------------------------

def _pool(players, vanilla=False):
    """Three bf16 DQN agents of different seeds (one keyed by another first_game_id), one fp16 agent, Piers and IGGI."""
    import hanabi_hip
    from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR

    probe = hanabi_hip.HanabiEnv("Hanabi-Full", players, n_games=1, auto_reset=False, packed=True)
    A, obs_len = probe.num_actions, probe.obs_len
    pool = [_dqn(obs_len, A, "bfloat16", seed=s) for s in (1, 2, 3)] + [_dqn(obs_len, A, "float16", seed=4)]
    pool[1].first_game_id = 4096
    pool += [RulebasedAgent(PR.piers_rules, seed=5), RulebasedAgent(PR.iggi_rules, seed=6)]
    if vanilla:
        pool.append(_dqn(obs_len, A, "bfloat16", seed=7, distributional=False, use_priority=False))
    return pool


def _standalone(players, n, seed, fgid, pool, teams, record):
    """Evaluator(game, players, n, seed, first_game_id).run(team) for every team."""
    from hanabi_hip import Evaluator

    return [Evaluator("Hanabi-Full", players, n_games=n, seed=seed, first_game_id=fgid, record_actions=record).run([pool[i] for i in t])
            for t in teams]


@pytest.mark.parametrize("n,record", [(1000, True), (4096, False)])
def test_every_team_matches_its_evaluator_two_players(n, record):
    from hanabi_hip import CrossPlay

    pool = _pool(2)
    seed, fgid = 13, 7
    cp = CrossPlay("Hanabi-Full", players=2, n_games=n, seed=seed, first_game_id=fgid, record_actions=record)
    res = cp.run(pool)
    assert len(res.teams) == 36 and res.teams[7] == (1, 1)
    assert len(cp.last_turns) == 1   # one chunk: every team in one lock-step run
    want = _standalone(2, n, seed, fgid, pool, res.teams, record)
    for t, got, w in zip(res.teams, res.results, want):
        _assert_same_result(got, w, t)
    m = res.mean_matrix()
    assert m[4, 5].item() == want[4 * 6 + 5].mean
    assert cp._chunks[36].env.illegal_count() == 0


def test_generic_path_and_chunking_give_the_same_results():
    """grouped=False (every agent its own eval_moves / hb_rule_act per block) and a max_rows that forces several chunks both
    reproduce the standalone results; a vanilla (scalar-head) agent in the pool takes the generic path either way."""
    from hanabi_hip import CrossPlay

    pool = _pool(2, vanilla=True)
    assert pool[-1].eval_operands() is None   # (the vanilla agent is off the one-kernel actor)
    n, seed, fgid = 1000, 13, 7
    teams = [(6, 0), (0, 6), (6, 6), (3, 4), (4, 3), (1, 2), (5, 6), (2, 2)]
    want = _standalone(2, n, seed, fgid, pool, teams, True)
    grouped = CrossPlay("Hanabi-Full", players=2, n_games=n, seed=seed, first_game_id=fgid, record_actions=True).run(pool, teams=teams)
    generic = CrossPlay("Hanabi-Full", players=2, n_games=n, seed=seed, first_game_id=fgid, record_actions=True).run(pool, teams=teams,
                                                                                                                    grouped=False)
    cp = CrossPlay("Hanabi-Full", players=2, n_games=n, seed=seed, first_game_id=fgid, record_actions=True, max_rows=3 * 1024)
    chunked = cp.run(pool, teams=teams)
    assert len(cp.last_turns) == 3
    for res in (grouped, generic, chunked):
        assert res.teams == teams
        for t, got, w in zip(teams, res.results, want):
            _assert_same_result(got, w, t)
    with pytest.raises(ValueError):
        grouped.mean_matrix()   # (explicit teams: no K x K matrix)


def test_five_players_explicit_teams():
    from hanabi_hip import CrossPlay

    pool = _pool(5)
    n, seed, fgid = 300, 21, 0
    teams = [(0, 4, 4, 4, 4), (4, 0, 0, 0, 0), (3, 1, 5, 2, 0), (5, 5, 5, 5, 5), (2, 3, 3, 4, 4)]
    res = CrossPlay("Hanabi-Full", players=5, n_games=n, seed=seed, record_actions=True).run(pool, teams=teams)
    want = _standalone(5, n, seed, fgid, pool, teams, True)
    for t, got, w in zip(teams, res.results, want):
        _assert_same_result(got, w, t)


def test_repeatable_and_agents_untouched():
    import torch

    from hanabi_hip import CrossPlay

    pool = _pool(2)
    dqn, rules = pool[:4], pool[4:]
    for a in dqn:   # (build the learners first, so that the snapshot below holds the actor's own buffers)
        a.eval_operands()
    snap = [[t.clone() for t in a._fl.actor.state_tensors()] for a in dqn]
    weights = [[p.detach().clone() for p in a.online.parameters()] for a in dqn]
    cp = CrossPlay("Hanabi-Full", players=2, n_games=512, seed=3, record_actions=True)
    x, y = cp.run(pool), cp.run(pool)
    for rx, ry in zip(x.results, y.results):
        _assert_same_result(rx, ry)
    assert x.as_dict() == y.as_dict()
    for a, s, w in zip(dqn, snap, weights):
        assert a._draws == 0 and a._fl.actor.q is None   # the actor's own q was never allocated
        assert all(torch.equal(u, v) for u, v in zip(a._fl.actor.state_tensors(), s))
        assert all(torch.equal(u, v) for u, v in zip(a.online.parameters(), w))
    assert all(a._draws == 0 and a.histogram == [0] * (len(a.rules) + 1) for a in rules)


def test_crossplay_leaves_training_untouched(monkeypatch):
    """Session A trains 20 steps, cross-plays its agents with two rule partners, trains 20 more; session B trains 40 steps.
    Both end bit-identical, and A's second cross-play of the same pool is B's."""
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
        params = RlaxRainbowParams(train_batch_size=128, experience_buffer_size=n * 8, mask_terminal=True, target_update_period=6,
                                   compute_dtype="bfloat16", packed_obs=True, layers=[512], learning_rate=0.01)
        mk = lambda s: DQNAgent(ObservationSpec((n, env.obs_len)), ActionSpec(env.num_actions), params._replace(seed=s), device="cuda")
        return SelfPlaySession(env, [mk(1), mk(2)])

    partners = [RulebasedAgent(PR.piers_rules), RulebasedAgent(PR.outer_rules)]
    a = session()
    a.run(20)
    r1 = a.crossplay(a.agents + partners, n_games=1000, seed=3)
    a.run(20)
    r2 = a.crossplay(a.agents + partners, n_games=1000, seed=3)
    state_a = _session_state(a)
    b = session()
    b.run(40)
    _assert_same(state_a, _session_state(b))
    assert a.native_steps > 10 and len(r1.teams) == 16 and r1.results[0].moves.sum() > 0
    r3 = b.crossplay(b.agents + partners, n_games=1000, seed=3)
    for x, y in zip(r2.results, r3.results):
        _assert_same_result(x, y)
    # and the session's cross-play of its own team is its evaluate()
    ev = b.evaluate(n_games=1000, seed=3)
    _assert_same_result(r3.results[1], ev)   # team (0, 1): the session's own seating
