"""GPU: hb_actor_fused_act_step (csrc/actor_fused.hip + env_api.hip) — the one-kernel actor with the env step as its tail.

The fused launch must compute, bit for bit, what hb_actor_fused_act followed by hb_env_step_packed computes on the same inputs:
q values, moves, every env output, the game state rows and the env's counters, over enough consecutive steps that finished games
are re-dealt and the deck pool is refilled (Hanabi-Full refills every third step). The session test checks that the one-call step
(hb_chain_run) issues the fused launch and trains exactly as the two-launch form does."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STEPS = 45


def _weights(obs_len, n_act, seed, dt):
    import torch

    H, K = 512, 51
    kp, np_ = (obs_len + 63) // 64 * 64, (n_act * K + 63) // 64 * 64
    g = torch.Generator(device="cuda").manual_seed(seed)
    w1 = torch.zeros(kp, H, device="cuda", dtype=dt)
    w1[:obs_len] = (torch.randn(obs_len, H, device="cuda", generator=g) * 0.04).to(dt)
    b1 = (torch.randn(H, device="cuda", generator=g) * 0.05).to(dt)
    w2 = torch.zeros(H, np_, device="cuda", dtype=dt)
    w2[:, :n_act * K] = (torch.randn(H, n_act * K, device="cuda", generator=g) * 0.2).to(dt)
    b2 = torch.zeros(np_, device="cuda", dtype=dt)
    b2[:n_act * K] = (torch.randn(n_act * K, device="cuda", generator=g) * 0.5).to(dt)
    return w1, b1, w2, b2, kp


@pytest.mark.parametrize("players,n,dtype,eps", [(2, 32768, "bfloat16", 0.0), (2, 32768, "bfloat16", 0.1), (2, 1000, "float16", 0.1),
                                                 (5, 32768, "float16", 0.0), (5, 777, "bfloat16", 0.1), (2, 129, "bfloat16", 0.0)])
def test_fused_step_equals_act_then_env_step(players, n, dtype, eps):
    import torch

    import hanabi_hip
    from hanabi_hip import _capi as K
    from hanabi_hip.ops import ActorMFMA

    L = K.lib()
    dt = getattr(torch, dtype)
    envs = [hanabi_hip.HanabiEnv("Hanabi-Full", players, n_games=n, seed=11 + players, packed=True) for _ in range(2)]
    ref, fused = envs
    assert L.hb_actor_fused_step_supported(fused.h) == 1
    w1, b1, w2, b2, kp = _weights(ref.obs_len, ref.num_actions, players * 1000 + n, dt)
    act = ActorMFMA(ref.obs_len, 512, ref.num_actions, 51, kp, "cuda", dtype=dt)
    assert act.fused
    act.fused_min_rows = 0
    act.pack(w1, b1, w2, b2)
    f = act._fset_ptrs[0]
    support = torch.linspace(-25, 25, 51, device="cuda")
    q_f = torch.empty(n, ref.num_actions, device="cuda")
    a_r = torch.empty(n, dtype=torch.int32, device="cuda")
    a_f = torch.empty(n, dtype=torch.int32, device="cuda")
    for e in envs:
        e.observe()
    seed, gid = 99, 4096
    for t in range(STEPS):
        a_r.copy_(act.act(ref.obs_bits, ref.legal, support, eps, seed, t, gid, one_kernel=True))
        q_r = act.q.clone()
        ref.step(a_r)
        K.check(L.hb_actor_fused_act_step(fused.h, fused.obs_bits.data_ptr(), fused.legal.data_ptr(), n, fused.obs_len, f[0], f[1], f[2], f[3],
                                          support.data_ptr(), 512, fused.num_actions, 51, q_f.data_ptr(), eps, seed, t, gid, a_f.data_ptr(),
                                          act._dt, fused.obs_bits.data_ptr(), fused.legal.data_ptr(), fused.reward.data_ptr(),
                                          fused.terminal.data_ptr(), fused.agent_reward.data_ptr(), fused.agent_step_type.data_ptr(),
                                          fused.score.data_ptr(), K.current_stream()))
        torch.cuda.synchronize()
        assert torch.equal(q_f, q_r), f"step {t}: q differs"
        assert torch.equal(a_f, a_r), f"step {t}: {(a_f != a_r).sum().item()} moves differ"
        for name in ("obs_bits", "legal", "reward", "terminal", "agent_reward", "agent_step_type", "score"):
            assert torch.equal(getattr(fused, name), getattr(ref, name)), f"step {t}: {name} differs"
        if t % 9 == 8 or t == STEPS - 1:
            assert torch.equal(fused.export_state(), ref.export_state()), f"step {t}: state rows differ"
    assert fused.illegal_count() == ref.illegal_count() == 0
    episodes, score_sum = fused.stats()
    assert (episodes, score_sum) == ref.stats()
    assert episodes > 0, "no game ended: the re-deal path was not exercised"


def test_fused_step_refuses_other_games():
    import torch

    import hanabi_hip
    from hanabi_hip import _capi as K

    L = K.lib()
    env = hanabi_hip.HanabiEnv("Hanabi-Small", 2, n_games=256, packed=True)
    assert L.hb_actor_fused_step_supported(env.h) == 0
    z = torch.zeros(64, dtype=torch.int32, device="cuda")
    rc = L.hb_actor_fused_act_step(env.h, env.obs_bits.data_ptr(), env.legal.data_ptr(), 256, env.obs_len, z.data_ptr(), z.data_ptr(),
                                   z.data_ptr(), z.data_ptr(), z.data_ptr(), 512, env.num_actions, 51, z.data_ptr(), 0.0, 1, 0, 0,
                                   z.data_ptr(), 1, env.obs_bits.data_ptr(), env.legal.data_ptr(), env.reward.data_ptr(),
                                   env.terminal.data_ptr(), env.agent_reward.data_ptr(), env.agent_step_type.data_ptr(), env.score.data_ptr(),
                                   K.current_stream())
    assert rc != 0 and b"configuration" in L.hb_last_error()


def _session_run(n, steps, fused):
    import os

    import torch

    import hanabi_hip
    from hanabi_agents.rlax_dqn import ActionSpec, DQNAgent, ObservationSpec, RlaxRainbowParams
    from hanabi_hip.selfplay import SelfPlaySession

    os.environ["HB_FUSED_ENV_STEP"] = "1" if fused else "0"
    try:
        flags = hanabi_hip.FLAG_AUTO_RESET | hanabi_hip.FLAG_RESET_START_NEXT
        env = hanabi_hip.HanabiEnv(config=hanabi_hip.make_config("Hanabi-Full", 2, flags), n_games=n, seed=5, packed=True)
        params = RlaxRainbowParams(train_batch_size=256, experience_buffer_size=n * 16, layers=[512], mask_terminal=True,
                                   compute_dtype="bfloat16", packed_obs=True, target_update_period=5)
        agents = [DQNAgent(ObservationSpec((n, env.obs_len)), ActionSpec(env.num_actions), params._replace(seed=s), device="cuda")
                  for s in (1, 2)]
        sess = SelfPlaySession(env, agents)
        for _ in range(steps):
            sess.step()
        sess.flush()
        torch.cuda.synchronize()
    finally:
        del os.environ["HB_FUSED_ENV_STEP"]
    return sess, env, agents


def test_session_chain_issues_the_fused_command(monkeypatch):
    """The benched wiring (one host call per step) issues the policy command with the env step in its tail (HB_CMD_ACTOR_FUSED_ACT
    with the env in p[9]: hb_actor_fused_act_step) and no env command, and trains exactly as the two-launch chain does: same
    observations, same moves, same replay rows, same weights, same sum trees."""
    import torch

    from hanabi_hip import _capi as K

    monkeypatch.setenv("HB_ACTOR_FUSED_MIN_ROWS", "0")
    n, steps = 2048, 20
    runs = {f: _session_run(n, steps, f) for f in (True, False)}
    sess, env, agents = runs[True]
    assert sess.native_steps >= steps - 12, sess.native_steps
    assert sess._chains and all(ch.fused_step for ch in sess._chains.values())
    for ch in sess._chains.values():
        ops = [ch.cmds[k].op for k in range(ch.count)]
        assert K.CMD_ENV_STEP_PACKED not in ops and ops.count(K.CMD_ACTOR_FUSED_ACT) == 1
        pol = ch.cmds[ops.index(K.CMD_ACTOR_FUSED_ACT)]
        assert pol.p[9] == env.h.value and pol.p[0] == env.obs_bits.data_ptr() and pol.p[10] == env.reward.data_ptr()
    sess2, env2, agents2 = runs[False]
    assert not any(ch.fused_step for ch in sess2._chains.values())
    assert torch.equal(env.obs_bits, env2.obs_bits) and torch.equal(env.export_state(), env2.export_state())
    assert env.stats() == env2.stats() and env.illegal_count() == env2.illegal_count() == 0
    for seat in (0, 1):
        assert torch.equal(sess.last_actions[seat], sess2.last_actions[seat])
        b1, b2 = agents[seat].experience, agents2[seat].experience
        assert b1.size == b2.size > 0
        t1, t2 = b1[np.arange(b1.size)], b2[np.arange(b2.size)]
        for name in ("observation_tm1", "observation_t", "action_tm1", "reward_t", "legal_moves_t", "terminal_t"):
            assert np.array_equal(getattr(t1, name), getattr(t2, name)), name
        w1, w2 = (torch.cat([p.detach().reshape(-1) for p in a[seat].online.parameters()]) for a in (agents, agents2))
        assert torch.equal(w1, w2)
        assert torch.equal(b1.sum_tree.nodes(), b2.sum_tree.nodes())
