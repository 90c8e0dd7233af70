"""GPU: the env, encoder and rule kernels on the deep-play corpus (tests/deep_play.py), bit for bit
against the CPU oracle, where the random-legal play of the other differential tests never gets: empty decks, short hands, the
final round with points on the board, completed stacks, the max-score ending and the re-deals out of them
(tests/test_deep_play_cpu.py asserts that the corpus reaches each of these). The driver's moves are computed once, on the
host, and go to both sides."""
import ctypes as C

import numpy as np
import pytest

import deep_play as D
from oracle import oracle_py as O
from test_actor_env_fused import _weights
from test_hip_env import _assert_same

pytestmark = pytest.mark.gpu


def _pair(game, players, packed, gpw=None, **kw):
    import hanabi_hip

    env = hanabi_hip.HanabiEnv(config=hanabi_hip.make_config(game, players, D.FLAGS), n_games=D.N_GAMES, seed=D.SEED,
                               first_game_id=D.FIRST_GAME_ID, games_per_wave=gpw, packed=packed, **kw)
    orc = O.OracleEnv(O.make_config(game, players, D.FLAGS), D.N_GAMES, seed=D.SEED, first_game_id=D.FIRST_GAME_ID)
    return env, orc


def _plain_step(env, act, t):
    import torch

    env.step(torch.as_tensor(act).cuda())


def _play(env, orc, game, players, apply=_plain_step, before_move=None):
    """The corpus run of one variant on both sides: everything the env emits and its state rows equal the oracle's after the
    reset and after every step; at the end so do the episode and score counters."""
    rng = np.random.default_rng(D.SEED)
    out = orc.observe()
    _assert_same(env, orc, out, "after reset")
    episodes = score = 0
    for t in range(D.steps_of(game, players)):
        if before_move is not None:
            before_move(t)
        act = D.open_hand_moves(orc.cfg, orc.export_state(), out["legal"], rng, D.P_RAND)
        apply(env, act, t)
        out = orc.step(act)
        _assert_same(env, orc, out, f"step {t}")
        episodes += int(out["terminal"].sum())
        score += int(out["score"][out["terminal"] != 0].sum())
    assert episodes > D.N_GAMES and env.stats() == (episodes, score)
    assert env.illegal_count() == 0 == orc.illegal_count()


class _RulesAlone:
    """hb_rule_act with every entry of RULES on its own over the env's state rows, against rule_oracle.c; `grouped`: and
    hb_rule_act_grouped with all of them as sets over len(RULES) copies of the rows, against those single calls."""

    def __init__(self, env, orc, grouped):
        import torch

        from hanabi_hip import _capi as K

        self.env, self.orc, self.grouped, self.K = env, orc, grouped, K
        m = len(D.RULES)
        self.tabs = []
        for kind, arg, thr in D.RULES:
            tab = (K.HbRule * 1)()
            tab[0].kind, tab[0].arg, tab[0].threshold = kind, arg, thr
            self.tabs.append(tab)
        self.act = torch.empty((m, env.n), dtype=torch.int32, device="cuda")
        self.fired = torch.empty((m, env.n), dtype=torch.int32, device="cuda")
        sets = (K.HbRule * (K.MAX_RULES * m))()
        for s, (kind, arg, thr) in enumerate(D.RULES):
            r = sets[s * K.MAX_RULES]
            r.kind, r.arg, r.threshold = kind, arg, thr
        self.sets = torch.frombuffer(bytearray(sets), dtype=torch.uint8).cuda()
        self.n_rules = torch.ones(m, dtype=torch.int32, device="cuda")
        self.set_of_block = torch.arange(m, dtype=torch.int32, device="cuda")
        self.gact = torch.empty((m, env.n), dtype=torch.int32, device="cuda")
        self.gfired = torch.empty((m, env.n), dtype=torch.int32, device="cuda")

    def __call__(self, t):
        import torch

        K, env = self.K, self.env
        L, cfg, m = K.lib(), C.byref(env.cfg), len(D.RULES)
        self.act.fill_(-7)
        self.fired.fill_(-9)
        for i, tab in enumerate(self.tabs):
            K.check(L.hb_rule_act(cfg, L.hb_env_state(env.h), env.n, D.FIRST_GAME_ID, tab, 1, D.RULE_SEED, t,
                                  K.dptr(self.act[i]), K.dptr(self.fired[i]), K.current_stream()))
        got_act, got_fired = self.act.cpu().numpy(), self.fired.cpu().numpy()
        for i, rule in enumerate(D.RULES):
            want_act, want_fired = self.orc.rule_act([rule], D.RULE_SEED, t)
            assert np.array_equal(got_fired[i], want_fired), f"step {t}: rule {rule}: fired differs"
            assert np.array_equal(got_act[i], want_act), f"step {t}: rule {rule}: move differs"
        if self.grouped:
            rows = env.export_state().repeat(m, 1).contiguous()
            self.gact.fill_(-7)
            self.gfired.fill_(-9)
            K.check(L.hb_rule_act_grouped(cfg, K.dptr(rows), m, env.n, D.FIRST_GAME_ID, K.dptr(self.set_of_block), K.dptr(self.sets),
                                          K.dptr(self.n_rules), m, D.RULE_SEED, t, K.dptr(self.gact), K.dptr(self.gfired),
                                          K.current_stream()))
            assert torch.equal(self.gact, self.act) and torch.equal(self.gfired, self.fired), f"step {t}: grouped call differs"


GROUPED = {("Hanabi-Full", 5), ("Hanabi-Small", 3)}


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("game,players", D.VARIANTS)
def test_deep_play_bit_exact(game, players, packed):
    """Every variant, int8 and bit-packed output. The int8 runs also hold the rule kernel to the oracle, each rule alone, at
    every state of the run (seed, draw and game ids as on the oracle)."""
    env, orc = _pair(game, players, packed)
    rules = None if packed else _RulesAlone(env, orc, (game, players) in GROUPED)
    _play(env, orc, game, players, before_move=rules)


SWITCHES = [("gpw", 8), ("gpw", 16), ("gpw", 32), ("gpw", 64), ("refill", 1), ("refill", 2), ("async", 1)]
# (Hanabi-Small has one life: a refill period of 1 is the only one there is, and the default)
SWITCH_CASES = [(g, p, s, v) for g, p in (("Hanabi-Full", 2), ("Hanabi-Full", 5), ("Hanabi-Small", 4)) for s, v in SWITCHES
                if not (g == "Hanabi-Small" and (s, v) == ("refill", 2))]


@pytest.mark.parametrize("game,players,switch,value", SWITCH_CASES)
def test_switches_that_must_not_matter(game, players, switch, value):
    """Games per wavefront, the deck pool's refill period and its asynchronous placement: "the results do not depend on it"."""
    from hanabi_hip import _capi as K

    env, orc = _pair(game, players, True, gpw=value if switch == "gpw" else None)
    L = K.lib()
    if switch == "refill":
        for bad in (0, env.cfg.max_life + 1):
            assert L.hb_env_set_refill_period(env.h, bad) == -1       # HB_ERR_INVALID
        K.check(L.hb_env_set_refill_period(env.h, value))
    elif switch == "async":
        K.check(L.hb_env_set_async_refill(env.h, 1))
    _play(env, orc, game, players)


@pytest.mark.parametrize("game,players", [("Hanabi-Full", 2), ("Hanabi-Full", 5), ("Hanabi-Small", 3)])
def test_selection_fused_step_takes_the_drivers_move(game, players):
    """hb_env_step_select_packed, greedy, with q = 0 at the driver's move and -1 elsewhere: it plays that move."""
    import torch

    env, orc = _pair(game, players, True)

    def apply(env, act, t):
        q = torch.full((env.n, env.num_actions), -1.0, device="cuda")
        a = torch.as_tensor(act).cuda()
        q.scatter_(1, a.long()[:, None], 0.0)
        got = env.step_select(q, 0.0, 99, t, D.FIRST_GAME_ID)[0]
        assert torch.equal(got, a), f"step {t}: the selection did not take the driver's move"

    _play(env, orc, game, players, apply=apply)


def _rows(env):
    return env.export_state().cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("turns", [25, 45, 60])
@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
@pytest.mark.parametrize("players", [2, 5])
def test_fused_actor_env_step_on_deep_states(players, dtype, turns):
    """hb_actor_fused_act_step against hb_actor_fused_act_dt + hb_env_step_packed from the states the driver reaches after
    `turns` moves (25: stacks half built; 45: low decks; 60: the final round, endings and re-deals inside the 12 steps)."""
    import torch

    import hanabi_hip
    from hanabi_hip import _capi as K
    from hanabi_hip.ops import ActorMFMA

    L = K.lib()
    n, eps, dt = 300, 0.1, getattr(torch, dtype)
    a, b = (hanabi_hip.HanabiEnv(config=hanabi_hip.make_config("Hanabi-Full", players, D.FLAGS), n_games=n, seed=D.SEED,
                                 first_game_id=D.FIRST_GAME_ID, packed=True) for _ in range(2))
    assert L.hb_actor_fused_step_supported(b.h) == 1
    rng = np.random.default_rng(D.SEED)
    for t in range(turns):
        act = torch.as_tensor(D.open_hand_moves(a.cfg, _rows(a), a.legal.cpu().numpy(), rng, D.P_RAND)).cuda()
        a.step(act)
        b.step(act)
    assert torch.equal(a.export_state(), b.export_state())
    w1, b1, w2, b2, kp = _weights(a.obs_len, a.num_actions, players * 1000 + turns, dt)
    actor = ActorMFMA(a.obs_len, 512, a.num_actions, 51, kp, "cuda", dtype=dt)
    assert actor.fused
    actor.fused_min_rows = 0
    actor.pack(w1, b1, w2, b2)
    f = actor._fset_ptrs[0]
    support = torch.linspace(-25, 25, 51, device="cuda")
    q_b = torch.empty(n, a.num_actions, device="cuda")
    act_a = torch.empty(n, dtype=torch.int32, device="cuda")
    act_b = torch.empty(n, dtype=torch.int32, device="cuda")
    seed = 99
    ended = 0
    for t in range(12):
        act_a.copy_(actor.act(a.obs_bits, a.legal, support, eps, seed, t, D.FIRST_GAME_ID, one_kernel=True))
        q_a = actor.q.clone()
        a.step(act_a)
        K.check(L.hb_actor_fused_act_step(b.h, b.obs_bits.data_ptr(), b.legal.data_ptr(), n, b.obs_len, f[0], f[1], f[2], f[3],
                                          support.data_ptr(), 512, b.num_actions, 51, q_b.data_ptr(), eps, seed, t, D.FIRST_GAME_ID,
                                          act_b.data_ptr(), actor._dt, b.obs_bits.data_ptr(), b.legal.data_ptr(), b.reward.data_ptr(),
                                          b.terminal.data_ptr(), b.agent_reward.data_ptr(), b.agent_step_type.data_ptr(),
                                          b.score.data_ptr(), K.current_stream()))
        torch.cuda.synchronize()
        assert torch.equal(act_b, act_a), f"step {t}: {(act_b != act_a).sum().item()} moves differ"
        assert torch.equal(q_b, q_a), f"step {t}: q differs"
        assert torch.equal(b.export_state(), a.export_state()), f"step {t}: state rows differ"
        for name in ("obs_bits", "legal", "reward", "terminal", "agent_reward", "agent_step_type", "score"):
            assert torch.equal(getattr(b, name), getattr(a, name)), f"step {t}: {name} differs"
        ended += int(a.terminal.sum())
    assert a.illegal_count() == b.illegal_count() == 0 and a.stats() == b.stats()
    if turns == 60:
        assert ended > 0, "no game ended: the terminal + re-deal path of the tail was not met"


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("game,players", [("Hanabi-Full", 2), ("Hanabi-Full", 4), ("Hanabi-Small", 5)])
def test_shuffled_env_is_the_plain_env_on_deep_states(game, players, packed):
    """tests/test_color_shuffle_gpu.py's core comparison with the driver's moves (computed on the plain env's rows)."""
    import torch

    import hanabi_hip
    from hanabi_hip import symmetry as S

    mk = lambda **kw: hanabi_hip.HanabiEnv(config=hanabi_hip.make_config(game, players, D.FLAGS), n_games=D.N_GAMES, seed=D.SEED,
                                           first_game_id=D.FIRST_GAME_ID, packed=packed, **kw)
    plain, shuf = mk(), mk(color_shuffle=True)
    cfg = plain.cfg
    rng = np.random.default_rng(D.SEED)
    steps = D.steps_of(game, players)
    redeals = 0
    for t in range(steps + 1):
        torch.cuda.synchronize()
        perms = shuf.color_perms().cpu().numpy()
        rows = _rows(plain)
        seat = ((rows[:, 0] >> 13) & 7).astype(np.int64)
        po = (plain.obs_bits if packed else plain.obs).cpu().numpy()
        so = (shuf.obs_bits if packed else shuf.obs).cpu().numpy()
        legal = plain.legal.cpu().numpy()
        assert np.array_equal(so, S.permute_obs(po, perms, seat, cfg)), f"step {t}: obs"
        assert np.array_equal(shuf.legal.cpu().numpy(), S.permute_legal(legal, perms, seat, cfg)), f"step {t}: legal"
        assert np.array_equal(_rows(shuf), rows), f"step {t}: state rows"
        for x, y in ((plain.reward, shuf.reward), (plain.terminal, shuf.terminal), (plain.score, shuf.score),
                     (plain.agent_reward, shuf.agent_reward), (plain.agent_step_type, shuf.agent_step_type)):
            assert torch.equal(x, y), f"step {t}"
        if t == steps:
            break
        redeals += int(plain.terminal.sum())
        act = torch.as_tensor(D.open_hand_moves(cfg, rows, legal, rng, D.P_RAND)).cuda()
        plain.step(act)
        shuf.step(S.permute_actions(act, perms, seat, cfg))
    assert plain.illegal_count() == 0 and shuf.illegal_count() == 0
    assert plain.stats() == shuf.stats() and redeals > D.N_GAMES
