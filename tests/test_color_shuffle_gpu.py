"""Colour-permuted frames (Other-Play) on the GPU: a shuffled env against a plain one through the host
helpers of hanabi_hip.symmetry, the permutation draw against Philox on the host, the selection-fused step, state round trips,
training and evaluation."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FLAGS = 3   # FLAG_AUTO_RESET | FLAG_RESET_START_NEXT


def _env(game, players, n, seed=7, first_game_id=100, **kw):
    import hanabi_hip

    return hanabi_hip.HanabiEnv(config=hanabi_hip.make_config(game, players, FLAGS), n_games=n, seed=seed, first_game_id=first_game_id,
                                **kw)


def _seat(env):
    return ((env.export_state()[:, 0] >> 13) & 7).cpu().numpy()


def _host_perms(cfg, seed, first_gid, rows, mask):
    """sigma(seed, game id, deal counter, seat) from the oracle's Philox, identity outside `mask` ([n] seat bits)."""
    from hanabi_hip import symmetry as S
    from oracle import oracle_py as O

    n, P, Cc = rows.shape[0], cfg.players, cfg.colors
    out = np.empty((n, P, Cc), np.uint8)
    for g in range(n):
        gid = first_gid + g
        for p in range(P):
            if (int(mask[g]) >> p) & 1:
                r = O.philox([64 + p, int(rows[g, 6]) & 0xFFFFFFFF, gid & 0xFFFFFFFF, gid >> 32], [seed & 0xFFFFFFFF, seed >> 32])
                out[g, p] = S.permutation(S.perm_index(int(r[0]), Cc), Cc)
            else:
                out[g, p] = np.arange(Cc)
    return out


def _lehmer(perm):
    C_ = len(perm)
    rest, idx = list(range(C_)), 0
    for i, v in enumerate(perm):
        d = rest.index(int(v))
        idx += d * math.factorial(C_ - 1 - i)
        rest.pop(d)
    return idx


CASES = [("Hanabi-Full", 2), ("Hanabi-Full", 3), ("Hanabi-Full", 4), ("Hanabi-Full", 5), ("Hanabi-Small", 2), ("Hanabi-Small", 5)]


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("gpw", [16, 64])
@pytest.mark.parametrize("game,players", CASES)
def test_shuffled_env_is_the_plain_env_in_each_seats_frame(game, players, gpw, packed):
    """The core check: a plain env driven by true-frame moves and a shuffled env driven by the same moves in the acting seat's
    frame stay in the same state; at every step the shuffled obs / legal are permute_obs / permute_legal of the plain ones."""
    import torch

    from hanabi_hip import symmetry as S

    n = 200   # (not a multiple of the games per wave: partial wavefronts)
    plain = _env(game, players, n, games_per_wave=gpw, packed=packed)
    shuf = _env(game, players, n, games_per_wave=gpw, packed=packed, color_shuffle=True)
    cfg = plain.cfg
    redeals = 0
    for t in range(151):
        torch.cuda.synchronize()
        perms = shuf.color_perms().cpu().numpy()
        seat = _seat(plain)
        po = (plain.obs_bits if packed else plain.obs).cpu().numpy()
        so = (shuf.obs_bits if packed else shuf.obs).cpu().numpy()
        assert np.array_equal(so, S.permute_obs(po, perms, seat, cfg)), f"step {t}: obs"
        assert np.array_equal(shuf.legal.cpu().numpy(), S.permute_legal(plain.legal.cpu().numpy(), perms, seat, cfg)), f"step {t}: legal"
        assert torch.equal(plain.export_state(), shuf.export_state()), f"step {t}: state rows"
        for x, y in ((plain.reward, shuf.reward), (plain.terminal, shuf.terminal), (plain.score, shuf.score),
                     (plain.agent_reward, shuf.agent_reward), (plain.agent_step_type, shuf.agent_step_type)):
            assert torch.equal(x, y), f"step {t}"
        if t == 150:
            break
        redeals += int(plain.terminal.sum())
        act = plain.random_legal_actions(seed=3, draw=t)
        plain.step(act)
        shuf.step(S.permute_actions(act, perms, seat, cfg))
    assert plain.illegal_count() == 0 and shuf.illegal_count() == 0
    assert plain.stats() == shuf.stats()
    assert redeals > 0
    if cfg.colors > 1:   # the frames really differ
        assert not np.array_equal(shuf.color_perms().cpu().numpy(), np.broadcast_to(np.arange(cfg.colors), (n, players, cfg.colors)))


def test_permutations_are_drawn_per_deal_and_masked_seat():
    """After several re-deals every game's sigma is Philox(seed, game id, deal counter, seat) decoded on the host; seats and
    games outside a per-game mask keep the identity; import and reset recompute them."""
    import torch

    n, seed, fg = 256, 11, 4000
    env = _env("Hanabi-Full", 3, n, seed=seed, first_game_id=fg, packed=True)
    rng = np.random.default_rng(0)
    mask = rng.integers(0, 8, n).astype(np.uint8)
    env.set_color_shuffle(torch.tensor(mask, device="cuda"))
    for t in range(400):
        env.step(env.random_legal_actions(seed=2, draw=t))
    rows = env.export_state().cpu().numpy().astype(np.int64)
    assert rows[:, 6].max() >= 3   # several deals
    want = _host_perms(env.cfg, seed, fg, rows, mask)
    assert np.array_equal(env.color_perms().cpu().numpy(), want)
    env.import_state(env.export_state())
    assert np.array_equal(env.color_perms().cpu().numpy(), want)
    env.reset()
    rows = env.export_state().cpu().numpy().astype(np.int64)
    assert np.array_equal(env.color_perms().cpu().numpy(), _host_perms(env.cfg, seed, fg, rows, mask))
    env.set_color_shuffle((1,))
    assert np.array_equal(env.color_perms().cpu().numpy(), _host_perms(env.cfg, seed, fg, rows, np.full(n, 2)))
    env.set_color_shuffle(False)
    assert not env.color_shuffled and env.color_shuffle == 0
    assert np.array_equal(env.color_perms().cpu().numpy(), np.broadcast_to(np.arange(5), (n, 3, 5)))


def test_permutations_are_uniform_and_seats_independent():
    n = 32768
    env = _env("Hanabi-Full", 2, n, seed=3, packed=True, color_shuffle=True)
    perms = env.color_perms().cpu().numpy()
    idx = np.array([[_lehmer(perms[g, p]) for p in range(2)] for g in range(n)])
    for p in range(2):
        counts = np.bincount(idx[:, p], minlength=120)
        assert (counts > 0).all()
        e = n / 120
        chi2 = float(((counts - e) ** 2 / e).sum())
        assert chi2 < 200, chi2          # 119 degrees of freedom: p < 1e-5 beyond 200
    # independence of the two seats: sigma(0) of seat 0 against sigma(0) of seat 1 (5 x 5 table, 16 degrees of freedom)
    tab = np.zeros((5, 5))
    np.add.at(tab, (perms[:, 0, 0], perms[:, 1, 0]), 1)
    e = tab.sum(1, keepdims=True) * tab.sum(0, keepdims=True) / n
    chi2 = float(((tab - e) ** 2 / e).sum())
    assert chi2 < 50, chi2


def test_selection_fused_step_on_a_shuffled_env():
    """hb_env_step_select_packed on a shuffled env equals hb_policy_select + hb_env_step_packed; actions_out is in the agent's
    frame, and mapped back by sigma^-1 it drives a plain env into the same state."""
    import torch

    from hanabi_hip import _capi as K, symmetry as S

    n, game, players = 300, "Hanabi-Full", 2
    a = _env(game, players, n, packed=True, color_shuffle=True)
    b = _env(game, players, n, packed=True, color_shuffle=True)
    c = _env(game, players, n, packed=True)
    A = a.num_actions
    g = torch.Generator(device="cuda").manual_seed(3)
    L = K.lib()
    for t in range(60):
        q = torch.randn(n, A, device="cuda", generator=g)
        if t % 3 == 0:
            q = torch.round(q * 2) / 2
        eps = (0.0, 0.3, 1.0)[t % 3]
        perms, seat = b.color_perms().cpu().numpy(), _seat(b)
        legal_b = b.legal.clone()
        act_a = torch.empty(n, dtype=torch.int32, device="cuda")
        K.check(L.hb_policy_select(K.dptr(q), K.dptr(a.legal), n, A, eps, 99, 1000 + t, 100, K.dptr(act_a), K.current_stream()))
        a.step(act_a)
        act_b = b.step_select(q, eps, 99, 1000 + t, 100)[0]
        c.step(S.unpermute_actions(act_b, perms, seat, c.cfg))
        torch.cuda.synchronize()
        assert torch.equal(act_a, act_b), f"step {t}"
        assert bool(legal_b.gather(1, act_b.long()[:, None]).all()), f"step {t}: actions_out not legal in the agent's frame"
        assert torch.equal(a.export_state(), b.export_state()) and torch.equal(b.export_state(), c.export_state()), f"step {t}"
        for x, y in ((a.obs_bits, b.obs_bits), (a.legal, b.legal), (a.reward, b.reward), (a.agent_step_type, b.agent_step_type)):
            assert torch.equal(x, y)
    assert a.illegal_count() == 0 and b.illegal_count() == 0 and c.illegal_count() == 0


def test_state_round_trip_restores_obs_and_permutations():
    import torch

    env = _env("Hanabi-Full", 4, 500, packed=True, color_shuffle=True)
    for t in range(30):
        env.step(env.random_legal_actions(seed=4, draw=t))
    rows, perms0 = env.export_state(), env.color_perms()

    def play():
        out = []
        for t in range(120):
            act = env.random_legal_actions(seed=5, draw=t)
            env.step(act)
            out.append((act.clone(), env.obs_bits.clone(), env.legal.clone(), env.color_perms()))
        return out

    first = play()
    env.import_state(rows)
    assert torch.equal(env.color_perms(), perms0)
    env.observe()
    second = play()
    for t, (x, y) in enumerate(zip(first, second)):
        for u, v in zip(x, y):
            assert torch.equal(u, v), f"move {t}"
    assert env.illegal_count() == 0


def _dqn(env, seed, n=None, **extra):
    from hanabi_agents.rlax_dqn import ActionSpec, DQNAgent, ObservationSpec, RlaxRainbowParams

    params = RlaxRainbowParams(train_batch_size=128, experience_buffer_size=8192, packed_obs=True, layers=[512], seed=seed, **extra)
    return DQNAgent(ObservationSpec((n or env.n, env.obs_len)), ActionSpec(env.num_actions), params, device="cuda")


def test_shuffled_env_has_no_fused_actor_step_and_session_falls_back():
    from hanabi_hip import _capi as K
    from hanabi_hip.selfplay import SelfPlaySession

    L = K.lib()
    plain = _env("Hanabi-Full", 2, 256, packed=True)
    shuf = _env("Hanabi-Full", 2, 256, packed=True, color_shuffle=True)
    assert L.hb_actor_fused_step_supported(plain.h) == 1
    assert L.hb_actor_fused_step_supported(shuf.h) == 0
    agents = [_dqn(shuf, 1), _dqn(shuf, 2)]
    sess = SelfPlaySession(shuf, agents, min_replay=256)
    assert not sess.fuse_env_step
    sess.run(40)
    assert shuf.illegal_count() == 0 and sess.grad_steps > 0


def test_rule_agent_in_a_shuffled_seat_is_refused():
    from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR
    from hanabi_hip.selfplay import SelfPlaySession

    env = _env("Hanabi-Full", 2, 128, packed=True, color_shuffle=(0,))
    rule = RulebasedAgent(PR.piers_rules)
    with pytest.raises(ValueError):
        SelfPlaySession(env, [rule, _dqn(env, 1)])
    SelfPlaySession(env, [_dqn(env, 1), rule])   # seat 1 keeps the true colours


def test_replay_holds_shuffled_rows_and_agent_frame_moves():
    import torch

    from hanabi_hip import symmetry as S
    from hanabi_hip.selfplay import SelfPlaySession

    n = 256
    env = _env("Hanabi-Small", 2, n, packed=True, color_shuffle=True)
    agents = [_dqn(env, 1), _dqn(env, 2)]
    sess = SelfPlaySession(env, agents, min_replay=10 ** 9)   # (no updates: the rings only)
    seen = []
    for t in range(3):
        seen.append((env.obs_bits.clone(), env.legal.clone(), env.color_perms().cpu().numpy(), _seat(env)))
        sess.step()
        seen[-1] += (sess.last_actions[t % 2].clone(),)
    torch.cuda.synchronize()
    buf = agents[0].experience
    obs0, legal0, perms0, seat0, act0 = seen[0]
    obs2, legal2 = seen[2][0], seen[2][1]
    assert torch.equal(buf._obs_tm1_buf[:n], obs0) and torch.equal(buf._obs_t_buf[:n], obs2)
    assert torch.equal(buf._lms_t_buf[:n], legal2)
    assert torch.equal(buf._act_tm1_buf[:n, 0].long(), act0.long())
    assert bool(legal0.gather(1, act0.long()[:, None]).all())   # the moves are legal in the agent's own frame
    true = S.unpermute_actions(act0.cpu().numpy(), perms0, seat0, env.cfg)
    assert (true != act0.cpu().numpy()).any() or not (perms0 != np.arange(2)).any()


def test_self_play_learns_hanabi_small_shuffled():
    """As test_self_play_learns_hanabi_small, with every seat colour-shuffled (Other-Play)."""
    import hanabi_hip
    from hanabi_agents.rlax_dqn import ActionSpec, DQNAgent, ObservationSpec, RlaxRainbowParams
    from hanabi_hip.selfplay import SelfPlaySession

    n = 2048
    env = hanabi_hip.HanabiEnv(config=hanabi_hip.make_config("Hanabi-Small", 2, FLAGS), n_games=n, seed=1, packed=True, color_shuffle=True)
    params = RlaxRainbowParams(compute_dtype="bfloat16", mask_terminal=True, experience_buffer_size=2 ** 18, learning_rate=2.5e-4,
                               epsilon=lambda ts: max(0.02, 1.0 - ts / 3000.0), target_update_period=200, atom_vmax=10, packed_obs=True)
    agents = [DQNAgent(ObservationSpec((n, env.obs_len)), ActionSpec(env.num_actions), params._replace(seed=s), device="cuda")
              for s in (1, 2)]
    sess = SelfPlaySession(env, agents, updates_per_step=4)
    sess.run(3500)
    ep0, sc0 = env.stats()
    sess.run(500)
    ep1, sc1 = env.stats()
    mean = (sc1 - sc0) / max(1, ep1 - ep0)
    assert env.illegal_count() == 0
    assert mean > 2.0, mean


def _eval_dqn(players, seed):
    import hanabi_hip

    probe = hanabi_hip.HanabiEnv("Hanabi-Full", players, n_games=1, auto_reset=False, packed=True)
    return _dqn(probe, seed, n=1)


def test_rule_teams_are_not_shuffled():
    import torch

    from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR
    from hanabi_hip import Evaluator

    team = [RulebasedAgent(PR.piers_rules), RulebasedAgent(PR.iggi_rules)]
    a = Evaluator("Hanabi-Full", 2, n_games=1024, seed=3, record_actions=True).run(team)
    b = Evaluator("Hanabi-Full", 2, n_games=1024, seed=3, record_actions=True, color_shuffle=True).run(team)
    assert b.perms is None
    for x, y in ((a.scores, b.scores), (a.lengths, b.lengths), (a.moves, b.moves), (a.actions, b.actions)):
        assert torch.equal(x, y)


@pytest.mark.parametrize("players", [2, 3])
def test_shuffled_dqn_moves_replay_through_oracle(players):
    from hanabi_hip import Evaluator, symmetry as S
    from oracle import oracle_py as O

    n, seed = 512, 5
    agents = [_eval_dqn(players, s + 1) for s in range(players)]
    ev = Evaluator("Hanabi-Full", players, n_games=n, seed=seed, record_actions=True, color_shuffle=True)
    res = ev.run(agents)
    assert res.perms.shape == (n, players, 5)
    perms = res.perms.numpy()
    cfg = O.make_config("Hanabi-Full", players, 0)
    env = O.OracleEnv(cfg, n, seed=seed)
    done = np.zeros(n, bool)
    score = np.zeros(n, np.int64)
    length = np.zeros(n, np.int64)
    for t in range(res.turns):
        act = S.unpermute_actions(res.actions[t].numpy(), perms, t % players, ev.cfg)
        out = env.step(np.asarray(act, np.int32))
        ended = ~done & (out["terminal"] != 0)
        score[ended], length[ended] = out["score"][ended], t + 1
        done |= ended
    assert done.all() and env.illegal_count() == 0
    assert np.array_equal(res.scores.numpy(), score) and np.array_equal(res.lengths.numpy(), length)
    # and the shuffle changed what the agents did
    plain = Evaluator("Hanabi-Full", players, n_games=n, seed=seed, record_actions=True).run(agents)
    assert not (plain.actions.shape == res.actions.shape and bool((plain.actions == res.actions).all()))


def test_crossplay_teams_equal_their_evaluator_runs_shuffled():
    import torch

    from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR
    from hanabi_hip import CrossPlay, Evaluator

    pool = [_eval_dqn(2, 1), _eval_dqn(2, 2), RulebasedAgent(PR.piers_rules)]
    n, seed = 300, 9
    cp = CrossPlay("Hanabi-Full", 2, n_games=n, seed=seed, record_actions=True, color_shuffle=True)
    got = cp.run(pool)
    ev = Evaluator("Hanabi-Full", 2, n_games=n, seed=seed, record_actions=True, color_shuffle=True)
    for team, r in zip(got.teams, got.results):
        want = ev.run([pool[i] for i in team])
        for x, y in ((r.scores, want.scores), (r.lengths, want.lengths), (r.moves, want.moves), (r.actions, want.actions)):
            assert torch.equal(x, y), team
        assert (r.perms is None) == (want.perms is None), team
        if r.perms is not None:
            assert torch.equal(r.perms, want.perms), team
