"""Training against a partner pool on the GPU (hanabi_hip.partner_pool): the two new kernels against their single-block forms and a
host recount, the pool's moves against each member's standalone launch, one-member equivalence with a plain partner, counts that
add up, evaluate_pool, resume, colour shuffle and five players."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _flags():
    import hanabi_hip

    return hanabi_hip.FLAG_AUTO_RESET | hanabi_hip.FLAG_RESET_START_NEXT


def _env(players, n, seed=5, game="Hanabi-Full", first_game_id=0):
    import hanabi_hip

    return hanabi_hip.HanabiEnv(config=hanabi_hip.make_config(game, players, _flags()), n_games=n, seed=seed, packed=True,
                                first_game_id=first_game_id)


def _frozen(env, dtype="bfloat16", seed=11, **extra):
    from hanabi_agents.rlax_dqn import ActionSpec, DQNAgent, ObservationSpec, RlaxRainbowParams

    params = RlaxRainbowParams(train_batch_size=128, experience_buffer_size=1024, compute_dtype=dtype, packed_obs=True, layers=[512],
                               seed=seed, **extra)
    return DQNAgent(ObservationSpec((1, env.obs_len)), ActionSpec(env.num_actions), params, device="cuda")


def _trainee(env, seed=1):
    from hanabi_agents.rlax_dqn import ActionSpec, DQNAgent, ObservationSpec, RlaxRainbowParams

    params = RlaxRainbowParams(train_batch_size=128, experience_buffer_size=env.n * 8, mask_terminal=True, target_update_period=6,
                               compute_dtype="bfloat16", packed_obs=True, layers=[512], learning_rate=0.01, seed=seed)
    return DQNAgent(ObservationSpec((env.n, env.obs_len)), ActionSpec(env.num_actions), params, device="cuda")


def _rule(name, seed=4321):
    from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR

    return RulebasedAgent(getattr(PR, f"{name}_rules"), seed=seed)


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


def _assert_same_result(got, want, what=""):
    import torch

    assert torch.equal(got.scores, want.scores), what
    assert torch.equal(got.lengths, want.lengths), what
    assert torch.equal(got.histogram, want.histogram), what
    assert got.bombouts == want.bombouts, what
    assert torch.equal(got.moves, want.moves), what
    assert torch.equal(got.misplays, want.misplays), what


# ---- kernel level ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("br,fgid", [(128, None), (130, 2**32 - 300)])
def test_rule_blocks_match_per_block_launches(br, fgid):
    """Six blocks of `br` games (two skipped: set -1 and set n_sets) over the four rule lists: each block equals hb_rule_act on
    its rows with the state pointer and game id offset to the block; the skipped blocks keep the sentinel. fgid None: the env's
    own first game id; 2^32 - 300 with 130-row blocks: first_game_id + b * block_rows + r crosses 2^32 inside the third block."""
    import torch

    import hanabi_hip
    from hanabi_hip import _capi as K

    L = hanabi_hip.lib()
    env = _env(2, 6 * br, seed=3, first_game_id=1000)
    fgid = env.first_game_id if fgid is None else fgid
    for t in range(23):
        env.step(env.random_legal_actions(seed=9, draw=t))
    agents = [_rule(x) for x in ("piers", "iggi", "outer", "flawed")]
    sets = [0, 1, -1, 2, 3, 4]
    tab = (K.HbRule * (K.MAX_RULES * 4))()
    for s, a in enumerate(agents):
        for q in range(len(a.rules)):
            tab[s * K.MAX_RULES + q] = a._tab[q]
    rules = torch.frombuffer(bytearray(tab), dtype=torch.uint8).cuda()
    n_rules = torch.tensor([len(a.rules) for a in agents], dtype=torch.int32, device="cuda")
    sob = torch.tensor(sets, dtype=torch.int32, device="cuda")
    acts = torch.full((env.n,), -7, dtype=torch.int32, device="cuda")
    fired = torch.full((env.n,), -7, dtype=torch.int32, device="cuda")
    state = L.hb_env_state(env.h)
    seed, draw = 77, 5
    K.check(L.hb_rule_act_blocks(C.byref(env.cfg), state, 6, br, fgid, K.dptr(sob), K.dptr(rules), K.dptr(n_rules), 4,
                                 seed, draw, K.dptr(acts), K.dptr(fired), K.current_stream()))
    sw = env.state_words
    for b, s in enumerate(sets):
        lo, hi = br * b, br * (b + 1)
        if s < 0 or s >= 4:
            assert (acts[lo:hi] == -7).all() and (fired[lo:hi] == -7).all()
            continue
        wa = torch.empty(br, dtype=torch.int32, device="cuda")
        wf = torch.empty(br, dtype=torch.int32, device="cuda")
        a = agents[s]
        K.check(L.hb_rule_act(C.byref(env.cfg), C.c_void_p(state + 4 * sw * lo), br, fgid + lo, a._tab, len(a.rules), seed,
                              draw, K.dptr(wa), K.dptr(wf), K.current_stream()))
        assert torch.equal(acts[lo:hi], wa), b
        assert torch.equal(fired[lo:hi], wf), b


def _recount(rows0, logs, tile_member, n_members, P, C_, R, H, INFO, D, max_life, seat0):
    """numpy hb_train_tally_init + hb_train_tally over the logged steps: counters, lost bytes, lengths."""
    n = rows0.shape[0]
    B = C_ * R + 1
    nc = 6 + B + 5 * P
    w0, w1 = rows0[:, 0].astype(np.int64) & 0xFFFFFFFF, rows0[:, 1].astype(np.int64) & 0xFFFFFFFF
    armed = (((w0 & 63) == D - P * H) & (((w0 >> 6) & 15) == INFO) & ((w1 & 0x7FFF) == 0) & (rows0[:, 8] == 0) & (rows0[:, 9] == 0))
    lost = np.zeros(n, np.int64)
    length = np.zeros(n, np.int64)
    cnt = np.zeros((n_members, nc), np.int64)
    mem = np.repeat(tile_member, 128)
    for t, (act, rew, term, score) in enumerate(logs):
        seat = (seat0 + t) % P
        kind = np.where(act < H, 0, np.where(act < 2 * H, 1, np.where(act < 2 * H + (P - 1) * C_, 2, 3)))
        mis = (kind == 1) & (rew <= 0)
        lost_now = lost + mis
        ln = length + 1
        for g in range(n):
            m = mem[g]
            if m < 0:
                continue
            c = cnt[m]
            c[6 + B + 4 * seat + kind[g]] += 1
            c[6 + B + 4 * P + seat] += mis[g]
            if term[g]:
                sc = int(score[g])
                c[0] += 1
                c[1] += sc
                c[2] += sc * sc
                c[3 + min(max(sc, 0), B - 1)] += 1
                if armed[g]:
                    c[5 + B] += 1
                    c[4 + B] += ln[g]
                    c[3 + B] += lost_now[g] >= max_life
                armed[g], lost[g], length[g] = True, 0, 0
            elif armed[g]:
                lost[g], length[g] = lost_now[g], ln[g]
    return cnt, np.where(armed, lost, 0x80), np.where(armed, length, 0), mem >= 0


@pytest.mark.parametrize("players,pre", [(2, 0), (2, 7), (5, 4)])
def test_train_tally_matches_host_recount(players, pre):
    """300 auto-reset steps of random legal moves over 3 members and a tile of nobody's: the counters and per-game state equal a
    numpy recount from the logged actions, rewards, terminals and scores. `pre` random steps before the init leave games mid-deal,
    which are tracked only from their next deal."""
    import torch

    import hanabi_hip
    from hanabi_hip import _capi as K

    L = hanabi_hip.lib()
    n = 8 * 128
    env = _env(players, n, seed=players + pre)
    for t in range(pre):
        env.step(env.random_legal_actions(seed=2, draw=1000 + t))
    tile_member = np.array([0, 0, 1, 2, 2, 2, -1, 1], np.int32)
    tm = torch.tensor(tile_member, device="cuda")
    cfg = env.cfg
    nc = L.hb_train_counters(C.byref(cfg))
    counters = torch.zeros(3, nc, dtype=torch.int64, device="cuda")
    lost = torch.empty(n, dtype=torch.uint8, device="cuda")
    length = torch.empty(n, dtype=torch.int16, device="cuda")
    rows0 = env.export_state().cpu().numpy()
    K.check(L.hb_train_tally_init(C.byref(cfg), L.hb_env_state(env.h), n, K.dptr(lost), K.dptr(length), K.current_stream()))
    logs = []
    for t in range(300):
        act = env.random_legal_actions(seed=4, draw=t + 1)
        env.step(act)
        K.check(L.hb_train_tally(C.byref(cfg), n, (pre + t) % players, K.dptr(act), K.dptr(env.reward), K.dptr(env.terminal),
                                 K.dptr(env.score), K.dptr(tm), 3, K.dptr(lost), K.dptr(length), K.dptr(counters), K.current_stream()))
        logs.append((act.cpu().numpy().astype(np.int64), env.reward.cpu().numpy(), env.terminal.cpu().numpy(),
                     env.score.cpu().numpy().astype(np.int64)))
    want, wlost, wlen, counted = _recount(rows0, logs, tile_member, 3, players, cfg.colors, cfg.ranks, cfg.hand_size, cfg.max_info,
                                          env.deck_size, cfg.max_life, pre % players)
    got = counters.cpu().numpy()
    B = cfg.colors * cfg.ranks + 1
    assert got[:, 0].sum() > 20 and got[:, 5 + B].sum() > 0   # (games ended, some of them tracked from their deal)
    np.testing.assert_array_equal(got, want)
    # (rows of the tile nobody owns are never touched)
    np.testing.assert_array_equal(lost.cpu().numpy()[counted], wlost[counted])
    np.testing.assert_array_equal(length.cpu().numpy().astype(np.int64)[counted], wlen[counted])


# ---- the pool's moves ---------------------------------------------------------------------------------------------------------

def _standalone_moves(pool, env, k, draw):
    import torch

    from hanabi_agents.rule_based import RulebasedAgent
    from hanabi_hip import _capi as K

    m = pool.members[k]
    lo, hi = pool.rows(k)
    out = torch.empty(hi - lo, dtype=torch.int32, device="cuda")
    if isinstance(m, RulebasedAgent):
        L = K.lib()
        K.check(L.hb_rule_act(C.byref(env.cfg), C.c_void_p(L.hb_env_state(env.h) + 4 * env.state_words * lo), hi - lo,
                              env.first_game_id + lo, m._tab, len(m.rules), pool.seed, draw, K.dptr(out), None, K.current_stream()))
        return out
    fgid = m.first_game_id
    m.first_game_id = env.first_game_id + lo
    try:
        m.eval_moves((env, (env.obs_bits[lo:hi], env.legal[lo:hi])), pool.seed, draw, out, scratch={})
    finally:
        m.first_game_id = fgid
    return out


@pytest.mark.parametrize("shuffle", [False, True])
def test_pool_moves_equal_each_members_standalone_launch(monkeypatch, shuffle):
    """Piers, IGGI, a bf16 and an fp16 one-kernel DQN and a vanilla (generic) DQN with uneven weights at 4 096 games: at every pool
    turn each member's rows are its standalone launch on those rows with the pool's seed, draw and global game ids. Shuffled: the
    DQN rows play in colour-permuted frames (shuffle_mask), the rule rows do not. No member's own state moves."""
    import torch

    import hanabi_hip

    monkeypatch.setenv("HB_ACTOR_FUSED_MIN_ROWS", "0")
    env = _env(2, 4096, seed=8, first_game_id=256)
    piers, iggi = _rule("piers", seed=3), _rule("iggi", seed=4)
    members = [piers, _frozen(env, "bfloat16", 21), iggi, _frozen(env, "float16", 22),
               _frozen(env, "bfloat16", 23, distributional=False, use_priority=False)]
    pool = hanabi_hip.PartnerPool(members, weights=[3, 2, 1, 1.5, 0.5], seed=99)
    pool.bind(env, (1,))
    assert pool.tiles == [(0, 12), (12, 8), (20, 4), (24, 6), (30, 2)]
    if shuffle:
        env.set_color_shuffle(pool.shuffle_mask((0, 1)))
        m = env.color_shuffle.cpu()
        for k, want in ((0, 1), (1, 3), (2, 1), (3, 3), (4, 3)):
            lo, hi = pool.rows(k)
            assert (m[lo:hi] == want).all(), k
    dqn = [members[1], members[3], members[4]]
    for a in dqn[:2]:
        assert a.eval_operands() is not None
    assert members[4].eval_operands() is None
    for t in range(24):
        if t % 2 == 0:
            env.step(env.random_legal_actions(seed=5, draw=t + 1))
            continue
        acts = pool.explore((env, (env.net_obs, env.legal))).clone()
        for k in range(len(members)):
            lo, hi = pool.rows(k)
            want = _standalone_moves(pool, env, k, pool._draws)
            assert torch.equal(acts[lo:hi], want), (t, k)
        env.step(acts)
    assert pool._draws == 12 and env.illegal_count() == 0
    assert piers._draws == 0 and iggi._draws == 0 and piers.histogram == [0] * (len(piers.rules) + 1)
    assert all(a._draws == 0 for a in dqn)


def test_rule_member_in_shuffled_rows_is_refused():
    import hanabi_hip
    from hanabi_hip.selfplay import SelfPlaySession

    env = _env(2, 512)
    pool = hanabi_hip.PartnerPool([_rule("piers"), _frozen(env)])
    env.set_color_shuffle(True)
    with pytest.raises(ValueError, match="true state"):
        SelfPlaySession(env, [_trainee(env), pool], train_seats=[0])


# ---- sessions ---------------------------------------------------------------------------------------------------------------

def test_one_member_pool_is_the_plain_partner(monkeypatch):
    """[trainee, PartnerPool([piers], seed=piers.seed)] and [trainee, piers] train identically for 300 steps."""
    import torch

    import hanabi_hip
    from hanabi_hip.selfplay import SelfPlaySession

    monkeypatch.setenv("HB_ACTOR_FUSED_MIN_ROWS", "0")

    def session(use_pool):
        torch.manual_seed(0)
        torch.cuda.manual_seed(0)
        env = _env(2, 1024, seed=6)
        piers = _rule("piers", seed=17)
        partner = hanabi_hip.PartnerPool([piers], seed=piers.seed) if use_pool else piers
        return SelfPlaySession(env, [_trainee(env), partner], train_seats=[0])

    a, b = session(True), session(False)
    for _ in range(6):
        a.run(50)
        b.run(50)
        assert torch.equal(a.env.export_state(), b.env.export_state())
        assert torch.equal(a.last_actions[0], b.last_actions[0])
    for p, q in zip(a.agents[0].online.parameters(), b.agents[0].online.parameters()):
        assert torch.equal(p, q)
    assert a.agents[0].train_step == b.agents[0].train_step > 0
    assert a.native_steps == b.native_steps > 0


def _pool_session(n=1024, players=2, seed=5, shuffle=False):
    import torch

    import hanabi_hip
    from hanabi_hip.selfplay import SelfPlaySession

    torch.manual_seed(0)
    torch.cuda.manual_seed(0)
    env = _env(players, n, seed=seed)
    pool = hanabi_hip.PartnerPool([_rule("piers"), _rule("iggi"), _frozen(env, "bfloat16", 31)], seed=7)
    if shuffle:   # (before the session: its one-call step is chosen for the env as it is then)
        env.set_color_shuffle(pool.shuffle_mask((0, 1), n=n, pool_seats=(1,)))
    return SelfPlaySession(env, [_trainee(env)] + [pool] * (players - 1), train_seats=[0]), pool


def _check_counts(sess, pool, steps):
    import torch

    env = sess.env
    st = pool.stats()
    _, sc = env.stats()
    assert sum(s.episodes for s in st) == sess.episodes > 0
    assert sum(s.score_sum for s in st) == sc - sess._stats0[1]
    P = env.players
    for k, s in enumerate(st):
        lo, hi = pool.rows(k)
        bins = torch.arange(len(s.histogram), dtype=torch.int64)
        assert int(s.histogram.sum()) == s.episodes
        assert int((s.histogram * bins).sum()) == s.score_sum
        assert int((s.histogram * bins * bins).sum()) == s.score_sq_sum
        assert int(s.moves.sum()) == steps * (hi - lo)
        assert s.moves.shape == (P, 4) and s.misplays.shape == (P,)
        assert s.tracked <= s.episodes and s.bombouts <= s.tracked
        assert s.tracked == 0 or s.mean_length > P
        d = s.as_dict()
        assert d["episodes"] == s.episodes and len(d["moves"]) == P


def test_counts_add_up_and_one_call_step_engages(monkeypatch):
    """2 players, 32 768 games, bf16, packed: the pool's per-member episodes and score sums add up to the session's and the env's,
    exactly; the trainee's one-host-call step engages."""
    monkeypatch.setenv("HB_ACTOR_FUSED_MIN_ROWS", "0")
    sess, pool = _pool_session(n=32768)
    sess.run(200)
    _check_counts(sess, pool, 200)
    assert sess.native_steps > 0 and sess.learner_stream is not None
    assert all(s.tracked > 0 for s in pool.stats())
    pool.reset_stats()
    assert all(s.episodes == 0 for s in pool.stats())


def test_evaluate_pool_equals_evaluator_and_leaves_training_untouched(monkeypatch):
    import torch

    from hanabi_hip import Evaluator

    monkeypatch.setenv("HB_ACTOR_FUSED_MIN_ROWS", "0")
    a, pool_a = _pool_session()
    with pytest.raises(ValueError, match="evaluate_pool"):
        a.evaluate()
    a.run(20)
    res = a.evaluate_pool(n_games=1000, seed=3)
    assert len(res) == 3
    for k, r in enumerate(res):
        want = Evaluator(config=a.env.cfg, n_games=1000, seed=3).run([a.agents[0], pool_a.members[k]])
        _assert_same_result(r, want, k)
    a.run(20)
    b, pool_b = _pool_session()
    b.run(40)
    torch.cuda.synchronize()
    _assert_same(a.checkpoint_state(), b.checkpoint_state())
    _check_counts(b, pool_b, 40)


def test_resume_is_bit_identical(monkeypatch, tmp_path):
    import torch

    import hanabi_hip

    monkeypatch.setenv("HB_ACTOR_FUSED_MIN_ROWS", "0")
    a, pool_a = _pool_session()
    a.run(30)
    path = tmp_path / "sess.pt"
    a.save_checkpoint(str(path))
    a.run(30)
    b, pool_b = _pool_session()
    b.load_checkpoint(str(path))
    b.run(30)
    torch.cuda.synchronize()
    for p, q in zip(a.agents[0].online.parameters(), b.agents[0].online.parameters()):
        assert torch.equal(p, q)
    assert torch.equal(pool_a.counters, pool_b.counters)
    assert torch.equal(pool_a._lost, pool_b._lost) and torch.equal(pool_a._length, pool_b._length)
    assert pool_a._draws == pool_b._draws == 30
    other = hanabi_hip.PartnerPool([_rule("outer"), _rule("iggi"), _frozen(a.env)])
    with pytest.raises(ValueError, match="different members"):
        other.load_checkpoint_state(pool_a.checkpoint_state())


def test_shuffle_mask_trains(monkeypatch):
    """Other-Play against a mixed pool: the trainee's seat shuffled everywhere, the pool's seat only on its DQN rows."""
    import torch

    monkeypatch.setenv("HB_ACTOR_FUSED_MIN_ROWS", "0")
    sess, pool = _pool_session(shuffle=True)
    sess.run(60)
    _check_counts(sess, pool, 60)
    assert sess.env.illegal_count() == 0 and sess.agents[0].train_step > 0
    m = sess.env.color_shuffle
    assert isinstance(m, torch.Tensor) and int(m[pool.rows(2)[0]]) == 3 and int(m[0]) == 1
    assert torch.equal(pool.shuffle_mask((0, 1)).cpu(), m.cpu())


def test_five_players(monkeypatch):
    monkeypatch.setenv("HB_ACTOR_FUSED_MIN_ROWS", "0")
    sess, pool = _pool_session(n=1024, players=5)
    assert pool.seats == (1, 2, 3, 4)
    sess.run(100)
    _check_counts(sess, pool, 100)
    assert sess.env.illegal_count() == 0 and sess.agents[0].train_step > 0
    assert pool._draws == 80
