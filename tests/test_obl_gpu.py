"""Off-belief learning on the GPU (hanabi_hip.obl, csrc/obl.hip): hb_obl_insert against the numpy restatement bit for bit, one
OffBeliefSession step against the CPU branch reference of tests/test_obl_cpu.py, the real game against SelfPlaySession's, a short
training run and the refusals."""
import numpy as np
import pytest

import deep_play as D
from test_obl_cpu import (BELIEF_SEED, FIXTURES, end_steps, expected_rows, fixture, obl_branch_ref, obl_insert_ref, piers_table)

pytestmark = pytest.mark.gpu

CAP = 256


# ---- the kernel ------------------------------------------------------------------------------------------------------------------
def _terminal_patterns(rng, P, n):
    """Rows in turn: never / at step 0 / at the last step / at several steps (the first one counts) / random."""
    term = (rng.random((P, n)) < 0.3).astype(np.int8)
    for g in range(n):
        kind = g % 5
        if kind == 0:
            term[:, g] = 0
        elif kind == 1:
            term[:, g] = 0
            term[0, g] = 1
        elif kind == 2:
            term[:, g] = 0
            term[P - 1, g] = 1
        elif kind == 3:
            term[:, g] = 1
            term[0, g] = P == 1
    return term


@pytest.mark.parametrize("n_steps", [1, 2, 3, 5])
@pytest.mark.parametrize("row_bytes", [24, 84, 171, 658])
def test_obl_insert_equals_the_restatement(n_steps, row_bytes):
    import torch

    from hanabi_hip import _capi as K

    A = 20 if row_bytes != 171 else 11
    rng = np.random.default_rng(1000 * n_steps + row_bytes)
    for n in (1, 63, 64, 65, 200):
        start = CAP - n // 2 - 1          # the batch wraps (n = 1: the last slot)
        host = dict(obs_tm1=rng.integers(-128, 128, (n, row_bytes)).astype(np.int8),
                    actions=rng.integers(0, A, n).astype(np.int32),
                    rewards=rng.integers(-3, 4, (n_steps, n)).astype(np.float32) + rng.random((n_steps, n)).astype(np.float32),
                    terminal=_terminal_patterns(rng, n_steps, n) * rng.integers(1, 3, (n_steps, n)).astype(np.int8),
                    obs_t=rng.integers(-128, 128, (n, row_bytes)).astype(np.int8),
                    legal_t=rng.integers(0, 2, (n, A)).astype(np.int8))
        rings = dict(obs_tm1=np.full((CAP, row_bytes), 0x5A, np.int8), obs_t=np.full((CAP, row_bytes), 0x5A, np.int8),
                     act=np.full(CAP, 0x5A, np.int8), lms=np.full((CAP, A), 0x5A, np.int8), rew=np.full(CAP, -77.0, np.float32),
                     term=np.full(CAP, 0x5A, np.uint8))
        dev = {k: torch.as_tensor(v).cuda() for k, v in host.items()}
        dring = {k: torch.as_tensor(v).cuda() for k, v in rings.items()}
        K.check(K.lib().hb_obl_insert(*(K.dptr(dev[k]) for k in ("obs_tm1", "actions", "rewards", "terminal", "obs_t", "legal_t")),
                                      *(K.dptr(dring[k]) for k in ("obs_tm1", "obs_t", "act", "lms", "rew", "term")),
                                      n, n_steps, row_bytes, A, CAP, start, K.current_stream()))
        want = obl_insert_ref(rings, host["obs_tm1"], host["actions"], host["rewards"], host["terminal"], host["obs_t"], host["legal_t"],
                              start)
        e = end_steps(host["terminal"])
        if n >= 63:
            assert (e == 0).any() and (e == n_steps).any() and (n_steps == 1 or (e == n_steps - 1).any())
        for k in want:   # the written slots bit for bit, and the sentinels everywhere else
            got = dring[k].cpu().numpy()
            assert np.array_equal(got.view(np.uint8 if got.dtype != np.float32 else np.uint32),
                                  want[k].view(np.uint8 if got.dtype != np.float32 else np.uint32)), (k, n)
        untouched = np.setdiff1d(np.arange(CAP), (start + np.arange(n)) % CAP)
        assert (dring["act"].cpu().numpy()[untouched] == 0x5A).all() and (dring["rew"].cpu().numpy()[untouched] == -77.0).all()
        assert (dring["obs_t"].cpu().numpy()[untouched] == 0x5A).all()


# ---- one session step --------------------------------------------------------------------------------------------------------------
def _params(n, **kw):
    from hanabi_agents.rlax_dqn import RlaxRainbowParams

    base = dict(train_batch_size=64, experience_buffer_size=CAP, compute_dtype="bfloat16", packed_obs=True, layers=[512],
                mask_terminal=True)
    base.update(kw)
    return RlaxRainbowParams(**base)


def _dqn(env, seed, **kw):
    from hanabi_agents.rlax_dqn import ActionSpec, DQNAgent, ObservationSpec

    return DQNAgent(ObservationSpec((env.n, env.obs_len)), ActionSpec(env.num_actions), _params(env.n, seed=seed, **kw), device="cuda")


def _env_at_fixture(fx):
    """A HIP env in the fixture's states: the same seed and game ids, stepped with the same moves."""
    import torch

    import hanabi_hip

    env = hanabi_hip.HanabiEnv(fx.game, fx.players, n_games=fx.n, seed=D.SEED, first_game_id=D.FIRST_GAME_ID, packed=True)
    for t in range(fx.turns):
        env.step(torch.as_tensor(fx.moves[t]).cuda())
    assert env.illegal_count() == 0
    assert np.array_equal(env.export_state().cpu().numpy().view(np.uint32), fx.rows)
    return env


def _check_step(fx, partners, partner_moves_from_gpu):
    import torch

    from hanabi_hip import OffBeliefSession

    env = _env_at_fixture(fx)
    learner = _dqn(env, seed=3)
    sess = OffBeliefSession(env, [learner] + partners, train_seats=[0], belief_seed=BELIEF_SEED)
    sess.step(train=False)
    sess.flush()
    torch.cuda.synchronize()
    a_t = sess.last_actions[0].cpu().numpy()
    moves = sess.branch_moves.cpu().numpy()
    assert np.array_equal(moves[0], a_t)
    ref = obl_branch_ref(fx, a_t, 0, partner_moves=moves if partner_moves_from_gpu else None, rules=piers_table())
    if not partner_moves_from_gpu:
        assert np.array_equal(moves, ref["moves"])
    e = end_steps(ref["terminal"])
    # the fixture does its work with the moves the learner really made (tests/test_obl_cpu.py chose it for that)
    assert (e == 0).any() and ((e > 0) & (e < fx.players)).any() and (e == fx.players).any()
    assert np.array_equal(sess._rew.cpu().numpy().view(np.uint32), ref["rewards"].view(np.uint32))
    assert np.array_equal(sess._term.cpu().numpy(), ref["terminal"])
    want = expected_rows(fx, a_t, ref, CAP)
    buf = learner.experience
    got = dict(obs_tm1=buf._obs_tm1_buf, obs_t=buf._obs_t_buf, act=buf._act_tm1_buf[:, 0], lms=buf._lms_t_buf, rew=buf._rew_t_buf[:, 0],
               term=buf._terminal_t_buf[:, 0].to(torch.uint8))
    for k, v in got.items():
        g = v.cpu().numpy()[:fx.n]
        assert np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g, want[k][:fx.n].view(np.uint32) if g.dtype == np.float32
                              else want[k][:fx.n]), k
    assert buf.size == fx.n and buf.oldest_entry == fx.n
    assert sess.dead_rows == 0 and sess.branch_steps == fx.n * fx.players and sess.env_steps == fx.n
    assert learner.last_obs.abs().sum().item() == 0   # never touched
    # the real env made the real move
    assert np.array_equal(env.export_state().cpu().numpy()[:, 0] >> 13 & 7, np.full(fx.n, 1 % fx.players))
    return sess


@pytest.mark.parametrize("game,players", list(FIXTURES))
def test_session_step_equals_the_branch_reference(game, players):
    from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR

    fx = fixture(game, players)
    _check_step(fx, [RulebasedAgent(PR.piers_rules, seed=20 + k) for k in range(1, players)], False)


def test_session_step_with_a_dqn_partner():
    """A bf16 DQN partner: its fictitious moves are read from the GPU and fed to the oracle; everything else is bit-exact."""
    fx = fixture("Hanabi-Full", 2)

    class Shape:   # (the partner is built before the env exists)
        n, obs_len, num_actions = fx.n, fx.obs.shape[1], fx.legal.shape[1]

    sess = _check_step(fx, [_dqn(Shape, seed=4)], True)
    assert sess.agents[1]._draws == 0 and sess.agents[1].experience.size == 0


# ---- the real game -----------------------------------------------------------------------------------------------------------------
def test_the_real_game_is_selfplay_s():
    import torch

    import hanabi_hip
    from hanabi_hip import OffBeliefSession
    from hanabi_hip.selfplay import SelfPlaySession

    def run(cls):
        torch.manual_seed(0)
        env = hanabi_hip.HanabiEnv("Hanabi-Full", 2, n_games=256, seed=7, packed=True)
        agents = [_dqn(env, seed=s, experience_buffer_size=8192) for s in (1, 2)]
        sess = cls(env, agents)
        acts = []
        for _ in range(40):
            sess.step(train=False)
            acts.append(sess.last_actions[(sess.t - 1) % 2].clone())
        sess.flush()
        torch.cuda.synchronize()
        return torch.stack(acts), env.export_state(), [a._draws for a in agents], sess

    a_obl, rows_obl, draws_obl, obl = run(OffBeliefSession)
    a_sp, rows_sp, draws_sp, sp = run(SelfPlaySession)
    assert torch.equal(a_obl, a_sp) and torch.equal(rows_obl, rows_sp)
    assert draws_obl == draws_sp == [20, 20]
    assert obl.env_steps == sp.env_steps == 40 * 256 and obl.branch_steps == 40 * 256 * 2
    assert obl.episodes == sp.episodes and obl.grad_steps == sp.grad_steps == 0


# ---- training ----------------------------------------------------------------------------------------------------------------------
def test_training_smoke():
    import torch

    import hanabi_hip
    from hanabi_hip import OffBeliefSession

    n, steps = 256, 150
    env = hanabi_hip.HanabiEnv("Hanabi-Small", 2, n_games=n, seed=11, packed=True)
    agents = [_dqn(env, seed=s, experience_buffer_size=32768, use_priority=True) for s in (1, 2)]
    w0 = [torch.cat([p.detach().reshape(-1) for p in a.online.parameters()]).clone() for a in agents]
    sess = OffBeliefSession(env, agents)
    sess.run(steps)
    torch.cuda.synchronize()
    assert sess.grad_steps > 0 and sess.env_steps == n * steps and sess.branch_steps == n * steps * 2 and sess.dead_rows == 0
    assert env.illegal_count() == 0 and sess.scratch.illegal_count() == 0
    for a, before in zip(agents, w0):
        w = torch.cat([p.detach().reshape(-1) for p in a.online.parameters()])
        assert torch.isfinite(w).all() and not torch.equal(w, before)
        buf = a.experience
        assert buf.size == n * (steps // 2)
        assert torch.isfinite(buf._rew_t_buf[:buf.size]).all()
        ended = buf._terminal_t_buf[:buf.size, 0]
        assert ended.any() and not ended.all()
        assert not buf._obs_t_buf[:buf.size][ended].any() and not buf._lms_t_buf[:buf.size][ended].any()
        assert buf._lms_t_buf[:buf.size][~ended].any(1).all()
        # every row of the ring has a leaf, and the root is their sum: fp32 pairwise sums over log2(capacity) = 15 levels, each
        # within 2^-24 relative of the exact sum of positive terms
        nodes = buf.sum_tree.nodes().double()
        leaves = nodes[buf.capacity:]
        assert torch.isfinite(leaves).all() and (leaves[:buf.size] > 0).all() and not leaves[buf.size:].any()
        total = float(buf.sum_tree.total_dev().item())
        assert abs(total - float(leaves.sum())) <= 15 * 2.0 ** -24 * float(leaves.sum())
    assert np.isfinite(sess.mean_score()) and sess.episodes > 0


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    import hanabi_hip
    from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR
    from hanabi_hip import OffBeliefSession, PartnerPool

    env = hanabi_hip.HanabiEnv("Hanabi-Small", 2, n_games=128, seed=1, packed=True)
    piers = RulebasedAgent(PR.piers_rules)
    good = _dqn(env, seed=1)
    with pytest.raises(ValueError, match="n_step"):
        OffBeliefSession(env, [_dqn(env, seed=1, n_step=3), piers])
    with pytest.raises(ValueError, match="mask_terminal"):
        OffBeliefSession(env, [_dqn(env, seed=1, mask_terminal=False), piers])
    with pytest.raises(ValueError, match="actor_lag"):
        OffBeliefSession(env, [_dqn(env, seed=1, actor_lag=1), piers])
    with pytest.raises(ValueError, match="partner pool"):
        OffBeliefSession(env, [good, PartnerPool([piers, RulebasedAgent(PR.iggi_rules)])], train_seats=[0])
    shuffled = hanabi_hip.HanabiEnv("Hanabi-Small", 2, n_games=128, seed=1, packed=True, color_shuffle=True)
    with pytest.raises(ValueError, match="colour-shuffled"):
        OffBeliefSession(shuffled, [good, _dqn(env, seed=2)])
    # the same agents outside the trained seats are passive partners: no refusal
    OffBeliefSession(env, [good, _dqn(env, seed=1, mask_terminal=False)], train_seats=[0])
    import torch.distributed as dist

    if dist.is_available() and not dist.is_initialized():
        import unittest.mock as mock

        with mock.patch.object(dist, "is_initialized", return_value=True), mock.patch.object(dist, "get_world_size", return_value=2):
            with pytest.raises(ValueError, match="single-rank"):
                OffBeliefSession(env, [good, piers])
