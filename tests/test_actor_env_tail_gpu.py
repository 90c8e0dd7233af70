"""GPU: the deck-pool refill inside hb_actor_fused_act_step (csrc/actor_fused.hip, env tail).

The fused step launches no refill kernel: the policy kernel's wavefronts that take no part in the move selection regenerate the
pool decks of their workgroup's own games whose flag an earlier launch raised. A refill that comes late, or not at all, re-deals
an old deck and changes the state rows. The tightest timing a refill can meet is a game that dies three steps after every deal,
so the tests drive the games with a constant "play slot 0" policy: all weights zero, b2 = +20 on the top atom of the play-slot-0
action and +20 on the bottom atom of every other action, epsilon 0. On the CPU oracle (n = 300, seed 7, 42 steps, auto-reset +
start-next) that move is legal at every step of every game for 2 and for 5 players, every game is re-dealt 6-12 times and 291-292
of the 300 games have an episode of exactly three steps. The tests assert the precondition (at least 6 deals per game) so they
cannot pass without meeting the path."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED, STEPS = 7, 42
OUTPUTS = ("obs_bits", "legal", "reward", "terminal", "agent_reward", "agent_step_type", "score")


def _flags():
    import hanabi_hip

    return hanabi_hip.FLAG_AUTO_RESET | hanabi_hip.FLAG_RESET_START_NEXT


def _env(players, n, **kw):
    import hanabi_hip

    return hanabi_hip.HanabiEnv(config=hanabi_hip.make_config("Hanabi-Full", players, _flags()), n_games=n, seed=SEED, packed=True, **kw)


class _PlaySlot0:
    """The constant policy as a packed one-kernel actor, and the fused step of an env under it."""

    def __init__(self, env, dtype):
        import torch

        from hanabi_hip import _capi as K
        from hanabi_hip.ops import ActorMFMA

        H, A, NK = 512, env.num_actions, 51
        dt = getattr(torch, dtype)
        kp, np_ = (env.obs_len + 63) // 64 * 64, (A * NK + 63) // 64 * 64
        self.uid = env.cfg.hand_size            # discards are uids 0 .. hand - 1, plays hand .. 2 hand - 1
        b2 = torch.zeros(np_, device="cuda", dtype=dt)
        b2[torch.arange(A, device="cuda") * NK] = 20.0
        b2[self.uid * NK] = 0.0
        b2[self.uid * NK + NK - 1] = 20.0
        self.actor = ActorMFMA(env.obs_len, H, A, NK, kp, "cuda", dtype=dt)
        assert self.actor.fused
        self.actor.fused_min_rows = 0
        self.actor.pack(torch.zeros(kp, H, device="cuda", dtype=dt), torch.zeros(H, device="cuda", dtype=dt),
                        torch.zeros(H, np_, device="cuda", dtype=dt), b2)
        self.support = torch.linspace(-25, 25, NK, device="cuda")
        self.q = torch.empty(env.n, A, device="cuda")
        self.moves = torch.empty(env.n, dtype=torch.int32, device="cuda")
        self.const = torch.full((env.n,), self.uid, dtype=torch.int32, device="cuda")
        self.K, self.L = K, K.lib()

    def fused_step(self, env, t):
        K, f = self.K, self.actor._fset_ptrs[0]
        self.moves.fill_(-1)
        K.check(self.L.hb_actor_fused_act_step(env.h, env.obs_bits.data_ptr(), env.legal.data_ptr(), env.n, env.obs_len, f[0], f[1], f[2], f[3],
                                               self.support.data_ptr(), 512, env.num_actions, 51, self.q.data_ptr(), 0.0, 99, t, 0,
                                               self.moves.data_ptr(), self.actor._dt, env.obs_bits.data_ptr(), env.legal.data_ptr(),
                                               env.reward.data_ptr(), env.terminal.data_ptr(), env.agent_reward.data_ptr(),
                                               env.agent_step_type.data_ptr(), env.score.data_ptr(), K.current_stream()))


def _deals(env):
    """per-game deal counter (state word 6)"""
    return env.export_state().cpu().numpy().view(np.uint32)[:, 6].astype(np.int64)


def _run(env, ref, pol, steps, is_fused, rows_every=6):
    """`env` stepped by the fused launch where is_fused(t), else by hb_env_step_packed on the constant move; `ref` by
    hb_env_step_packed only. Every output equal at every step, the state rows every `rows_every` steps and at the end, the
    counters at the end. Returns the number of deals of each game."""
    import torch

    assert pol.L.hb_actor_fused_step_supported(env.h) == 1
    assert torch.equal(env.export_state(), ref.export_state())
    first = _deals(env)
    for t in range(steps):
        ref.step(pol.const)
        if is_fused(t):
            pol.fused_step(env, t)
            torch.cuda.synchronize()
            assert torch.equal(pol.moves, pol.const), f"step {t}: {(pol.moves != pol.const).sum().item()} moves are not play slot 0"
        else:
            env.step(pol.const)
        for name in OUTPUTS:
            assert torch.equal(getattr(env, name), getattr(ref, name)), f"step {t}: {name} differs"
        if t % rows_every == rows_every - 1 or t == steps - 1:
            assert torch.equal(env.export_state(), ref.export_state()), f"step {t}: state rows differ"
    assert env.stats() == ref.stats()
    assert env.illegal_count() == ref.illegal_count() == 0
    return _deals(env) - first


@pytest.mark.parametrize("n", [300, 129])   # 300: two full workgroups + one of 44 rows (a part-filled and empty wavefronts); 129: one row
@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
@pytest.mark.parametrize("players", [2, 5])
def test_fused_steps_refill_in_time(players, dtype, n):
    env, ref = _env(players, n), _env(players, n)
    deals = _run(env, ref, _PlaySlot0(env, dtype), STEPS, lambda t: True)
    assert deals.min() >= 6, f"a game was dealt only {deals.min()} times: back-to-back three-step episodes were not met"


# blocks of (fused steps, plain steps), repeated
PATTERNS = [(1, 3), (2, 2), (1, 1), (3, 1)]


@pytest.mark.parametrize("switch", [None, "refill_period_1", "async_refill"])
@pytest.mark.parametrize("pattern", PATTERNS, ids=lambda p: f"{p[0]}+{p[1]}")
def test_fused_and_plain_steps_mixed_on_one_env(pattern, switch):
    """The cadence bookkeeping: a plain entry point after fused steps must still refill before a game dealt in a fused step can
    end, whatever the refill period and placement; the twin takes plain steps only, with the default cadence."""
    from hanabi_hip import _capi as K

    n = 300
    env, ref = _env(2, n), _env(2, n)
    if switch == "refill_period_1":
        K.check(K.lib().hb_env_set_refill_period(env.h, 1))
    elif switch == "async_refill":
        K.check(K.lib().hb_env_set_async_refill(env.h, 1))
    nf, npl = pattern
    deals = _run(env, ref, _PlaySlot0(env, "bfloat16"), STEPS, lambda t: t % (nf + npl) < nf)
    assert deals.min() >= 6


@pytest.mark.parametrize("players", [2, 5])
def test_fused_steps_deal_the_callers_decks(players):
    """Caller-set decks: every re-deal deals the caller's deck of that game again (the pool's copy path). The decks are fixed
    permutations of the canonical deck; under them every game is dealt again at least twice within the 24 steps (2-8 times on
    the CPU oracle, 2 and 5 players), so every game meets a re-deal from a regenerated pool entry."""
    import torch

    n, steps = 300, 24
    env, ref = _env(players, n), _env(players, n)
    counts = (3, 2, 2, 2, 1)
    canon = np.array([5 * c + r for c in range(5) for r in range(5) for _ in range(counts[r])], dtype=np.uint8)
    rng = np.random.default_rng(SEED)
    decks = np.stack([rng.permutation(canon) for _ in range(n)])
    for e in (env, ref):
        e.set_decks(decks)
        e.reset()
    deals = _run(env, ref, _PlaySlot0(env, "bfloat16"), steps, lambda t: True)
    assert deals.min() >= 2, "a game was not dealt again twice: the regenerated pool entries were not all met"
    w_deck = 10 + 3 * players
    rows = env.export_state().cpu().numpy().view(np.uint32)
    got = np.ascontiguousarray(rows[:, w_deck:w_deck + 13]).view(np.uint8)[:, :50]
    assert np.array_equal(got, decks), "a game was dealt a deck that is not the caller's"


def test_session_trains_as_the_two_launch_chain(monkeypatch):
    """SelfPlaySession through hb_chain_run: weights, replay rings, sum trees and env rows equal those of the same run with
    HB_FUSED_ENV_STEP=0 (tests/test_actor_env_fused.py's comparison, over more steps than a re-dealt game needs to end again)."""
    import torch

    from test_actor_env_fused import _session_run

    monkeypatch.setenv("HB_ACTOR_FUSED_MIN_ROWS", "0")
    n, steps = 2048, 30
    (sess, env, agents), (sess2, env2, agents2) = (_session_run(n, steps, f) for f in (True, False))
    assert sess._chains and all(ch.fused_step for ch in sess._chains.values())
    assert not any(ch.fused_step for ch in sess2._chains.values())
    assert torch.equal(env.obs_bits, env2.obs_bits) and torch.equal(env.export_state(), env2.export_state())
    assert env.stats() == env2.stats() and env.stats()[0] > 0 and env.illegal_count() == env2.illegal_count() == 0
    for seat in (0, 1):
        b1, b2 = agents[seat].experience, agents2[seat].experience
        assert b1.size == b2.size > 0
        t1, t2 = b1[np.arange(b1.size)], b2[np.arange(b2.size)]
        for name in ("observation_tm1", "observation_t", "action_tm1", "reward_t", "legal_moves_t", "terminal_t"):
            assert np.array_equal(getattr(t1, name), getattr(t2, name)), name
        w1, w2 = (torch.cat([p.detach().reshape(-1) for p in a[seat].online.parameters()]) for a in (agents, agents2))
        assert torch.equal(w1, w2)
        assert torch.equal(b1.sum_tree.nodes(), b2.sum_tree.nodes())
