"""The epsilon-aware soft likelihood filter on the GPU (hanabi_hip.search, csrc/belief.hip): hb_belief_select_soft against the
numpy restatement hanabi_hip.belief_select_soft_ref bit for bit (tests/test_belief_soft_cpu.py holds the restatement to
hand-worked figures), ConditionedDeterminizer.sample_history(epsilon=...) against the same steps composed by hand on both of its
paths, the unchanged default, OffBeliefSession(belief_epsilon=...) and SearchPlayer(epsilon=...)."""
import ctypes as C

import numpy as np
import pytest
from search_util import _u32

pytestmark = pytest.mark.gpu

GUARD = 16
FILL = {"int32": 0x5A5A5A5A, "uint8": 0x5A, "float32": 12345.0}


def _guarded(shape, dtype):
    """(buffer, view): a contiguous tensor of `shape` with GUARD sentinel elements before and after it."""
    import torch

    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), FILL[str(dtype).split(".")[1]], dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(shape)


def _inputs(rng, m, K, D, SW, A):
    """Random inputs of one call with every case of the kernel in roots 0 .. 8 (as far as m reaches), rows as uint32."""
    src = rng.integers(0, 2 ** 32, (m, SW), dtype=np.uint64).astype(np.uint32)
    src[:, 0] &= ~np.uint32(3 << 19)                              # running
    det = rng.integers(0, 2 ** 32, (m * K, SW), dtype=np.uint64).astype(np.uint32)
    w = rng.integers(1, 1 << 28, (m, K)).astype(np.uint32)        # (weights stay below 2^28: the product of at most 5 counts <= 45)
    w[rng.random((m, K)) < 0.2] = 0
    actual = rng.integers(0, 3, (D, m))
    hyp = rng.integers(0, 3, (D, K, m))
    nl = rng.integers(1, A + 1, (D, K, m))
    nl[rng.random((D, K, m)) < 0.05] = 0                          # n_legal of 0 ...
    nl[rng.random((D, K, m)) < 0.05] = A                          # ... and of A
    nl[rng.random((D, K, m)) < 0.02] = A + 1                      # out of range on either side: the candidate weighs nothing
    nl[rng.random((D, K, m)) < 0.02] = -1
    valid = (rng.integers(0, 4, (D, m)) != 0).astype(np.uint8)
    case = lambda i: i < m
    if case(0):   # every candidate live and in range, every entry valid; zero weights on both sides of the chunk boundary
        valid[:, 0], w[0] = 1, np.maximum(w[0], 1)
        nl[:, :, 0] = np.clip(nl[:, :, 0], 1, A)
        for k in (63, 64):
            if k < K and K > 2:
                w[0, k] = 0
    if case(1):   # not running, candidates of weight != 0: L = 0, drawn by the weights alone
        src[1, 0] |= 1 << 19
        w[1] = np.maximum(w[1], 1)
    if case(2):   # not running as the determinizer leaves it: every weight 0, T = 0
        src[2, 0] |= 2 << 19
        w[2] = 0
    if case(3):   # an invalid entry in the middle of the chain
        valid[:, 3] = 1
        valid[min(1, D - 1), 3] = 0 if D > 1 else 1
    if case(4):   # running, every weight 0: T = 0
        valid[:, 4], w[4] = 1, 0
    if case(5):   # every n_legal 0 at the newest entry: mx = 0, T = 0
        valid[:, 5], nl[0, :, 5] = 1, 0
    if case(6):   # every n_legal = A, everybody reproduces everything: equal likelihoods
        valid[:, 6], nl[:, :, 6] = 1, A
        hyp[:, :, 6] = actual[:, None, 6]
    if case(7):   # nobody reproduces the newest move: the likelihoods differ by n_legal alone
        valid[:, 7] = 1
        hyp[0, :, 7] = actual[0, 7] + 1
        w[7, 0], nl[:, 0, 7] = max(int(w[7, 0]), 1), 2
    if case(8):   # only the last candidate is live
        valid[:, 8], w[8, :-1] = 1, 0
        w[8, -1], nl[:, -1, 8] = 7, 1
    return src, det, w.reshape(-1), hyp, nl, actual, valid


@pytest.mark.parametrize("game,players", [("Hanabi-Full", 2), ("Hanabi-Small", 2), ("Hanabi-Full", 5)])
@pytest.mark.parametrize("m", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("K", [1, 4, 64, 65, 130])
def test_select_soft_equals_the_restatement(game, players, m, K):
    """R in {1, 3, 32} x depth in {1, 2, 8} per shape; all six outputs between sentinels, compared with the restatement: rows,
    weights, n_surv, depth_used and fallback bit for bit, ess to 1e-6 relative (its f64 sum of squares is added in another
    order)."""
    import torch

    import hanabi_hip
    from hanabi_hip import belief_select_soft, belief_select_soft_ref, soft_table

    cfg = hanabi_hip.make_config(game, players)
    L = hanabi_hip.lib()
    SW, A = L.hb_state_words(C.byref(cfg)), L.hb_num_actions(C.byref(cfg))
    assert SW == (48 if players == 5 else 32)
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a).astype(dt)).cuda()
    seen = {"dead": 0, "drawn": 0, "L0": 0, "cut": 0}
    for R in (1, 3, 32):
        for D in (1, 2, 8):
            rng = np.random.default_rng(((m * 131 + K) * 37 + R) * 11 + D)
            src, det, w, hyp, nl, actual, valid = _inputs(rng, m, K, D, SW, A)
            eps = (0.1, 0.5, 1e-6)[D % 3]
            table = soft_table(eps, A)
            seed, draw, first = 0x1234567800000005 + R, 0x300000007 + D, (1 << 33) - 3 if D == 2 else 100 * R
            shapes = (((m * R, SW), torch.int32), ((m * R,), torch.int32), ((D, m), torch.int32), ((m,), torch.int32),
                      ((m,), torch.uint8), ((m,), torch.float32))
            for use_valid in (True, False):
                bufs, out = zip(*(_guarded(s, dt) for s, dt in shapes))
                got = belief_select_soft(cfg, t(src.view(np.int32), np.int32), t(det.view(np.int32), np.int32), t(w.view(np.int32), np.int32),
                                         t(hyp, np.int32), t(nl, np.int32), t(actual, np.int32), t(valid, np.uint8) if use_valid else None,
                                         table.cuda(), R, seed, draw, first_row_id=first, out=out)
                torch.cuda.synchronize()
                want = belief_select_soft_ref(src, det, w, hyp, nl, actual, valid if use_valid else None, table.numpy(), R, seed, draw,
                                              first_row_id=first, details=True)
                for g, x, name in zip(got, want, ("rows", "weights", "n_surv", "depth_used", "fallback")):
                    assert np.array_equal(_u32(g) if name in ("rows", "weights") else g.cpu().numpy(), x), (name, R, D, use_valid)
                ess = got[5].cpu().numpy()
                assert ess.dtype == np.float32 and np.allclose(ess, want[5], rtol=1e-6, atol=0), (R, D, use_valid)
                for buf, (_, dt) in zip(bufs, shapes):   # the sentinels on both sides
                    fill = FILL[str(dt).split(".")[1]]
                    assert bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all()), (R, D, use_valid)
                x = want[-1]
                seen["dead"] += int((x["T"] == 0).sum())
                seen["drawn"] += int((x["T"] > 0).sum())
                seen["L0"] += int(((want[3] == 0) & (x["T"] > 0)).sum())
                seen["cut"] += int(((want[3] > 0) & (want[3] < D)).sum())
                if m > 8 and use_valid:
                    assert x["T"][2] == 0 and x["T"][4] == 0 and x["T"][5] == 0 and x["T"][1] > 0 and want[3][1] == 0 and want[4][1] == 2
                    assert want[3][0] == D and want[3][3] == min(D, 1) and want[3][6] == D and want[2][D - 1, 6] == np.count_nonzero(x["W"][6])
                    assert x["pick"][8].tolist() == [K - 1] * R and x["T"][7] > 0 and want[2][0, 7] == 0
                    if K > 64:
                        assert x["W"][0, 63] == 0 and x["W"][0, 64] == 0 and (x["pick"][0] != 63).all() and (x["pick"][0] != 64).all()
    assert seen["drawn"] > 0 and (m < 3 or (seen["dead"] > 0 and seen["L0"] > 0 and seen["cut"] > 0))


def test_more_than_64_replicas_and_4096_candidates():
    """The outputs are drawn 64 at a time and the candidates 64 at a time: R = 130 over K = 4096 (the most the host lets in)."""
    import torch

    import hanabi_hip
    from hanabi_hip import belief_select_soft, belief_select_soft_ref, soft_table

    cfg = hanabi_hip.make_config("Hanabi-Full", 2)
    m, K, R, D, SW, A = 3, 4096, 130, 2, 32, 20
    rng = np.random.default_rng(9)
    src, det, w, hyp, nl, actual, valid = _inputs(rng, m, K, D, SW, A)
    w.reshape(m, K)[0] = (1 << 28) - 1   # the largest sum: T just below 2^64 when every likelihood is the largest
    hyp[:, :, 0], nl[:, :, 0], valid[:, 0] = actual[:, None, 0], 4, 1
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a).astype(dt)).cuda()
    table = soft_table(0.1, A)
    got = belief_select_soft(cfg, t(src.view(np.int32), np.int32), t(det.view(np.int32), np.int32), t(w.view(np.int32), np.int32),
                             t(hyp, np.int32), t(nl, np.int32), t(actual, np.int32), t(valid, np.uint8), table.cuda(), R, 3, 4)
    want = belief_select_soft_ref(src, det, w, hyp, nl, actual, valid, table.numpy(), R, 3, 4, details=True)
    assert int(want[-1]["T"][0]) == ((1 << 28) - 1) * (1 << 24) * 4096 and len(set(want[-1]["pick"][0].tolist())) > 100
    for g, x, name in zip(got, want, ("rows", "weights", "n_surv", "depth_used", "fallback")):
        assert np.array_equal(_u32(g) if name in ("rows", "weights") else g.cpu().numpy(), x), name
    assert np.allclose(got[5].cpu().numpy(), want[5], rtol=1e-6, atol=0) and abs(float(want[5][0]) - 4096) < 1e-2


# ---- sample_history ------------------------------------------------------------------------------------------------------------------
def _dqn(env, seed):
    from hanabi_agents.rlax_dqn import ActionSpec, DQNAgent, ObservationSpec, RlaxRainbowParams

    params = RlaxRainbowParams(train_batch_size=64, experience_buffer_size=8192, compute_dtype="bfloat16", packed_obs=True, layers=[512],
                               mask_terminal=True, seed=seed)
    return DQNAgent(ObservationSpec((env.n, env.obs_len)), ActionSpec(env.num_actions), params, device="cuda")


def _small_game(m, turns, seat, depth, seed=7):
    """m games of Small, 2 players, [Piers, an untrained DQN agent], turn by turn as Evaluator.run keys it; `seat` keeps a
    PartnerHistory as SearchPlayer does. -> (team, env, history, rows)."""
    import torch

    import hanabi_hip
    from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR
    from hanabi_hip import PartnerHistory, last_move_uid
    from hanabi_hip.search import _ask

    env = hanabi_hip.HanabiEnv("Hanabi-Small", 2, n_games=m, seed=seed, auto_reset=False, packed=True)
    team = [RulebasedAgent(PR.piers_rules, seed=11), _dqn(env, seed=6)]
    hist = PartnerHistory(env.cfg, m, depth, "cuda", partner_seed=seed, first_game_id=0)
    act = torch.empty(m, dtype=torch.int32, device="cuda")
    states, mine, scratch = [env.export_state()], None, {}
    env.observe()
    for t in range(turns + 1):
        rows = states[-1]
        if t % 2 == seat and t >= 1:
            if mine is not None:
                hist.own_move(mine)
            hist.push(states[-2], last_move_uid(env.cfg, rows), t, torch.ones(m, dtype=torch.uint8), seat=seat)
        if t == turns:
            break
        _ask(team[t % 2], env, seed, t + 1, act, scratch)
        if t % 2 == seat:
            mine = act.clone()
        env.step(act)
        states.append(env.export_state())
    return team, env, hist, states[-1]


def test_sample_history_soft_against_the_steps_by_hand():
    """200 games of Small (a slab of 200 legal rows is no multiple of 16 bytes: the padded slabs), four turns in: the untrained
    agent has moved twice and the history holds both moves; Small has one life, so some games have ended on a misplay: roots
    that are not running, with candidates of weight 0. By hand: determinize, splice with the alive
    masks, one scratch import + observe + eval_moves per (entry, candidate) with the legal moves counted off the env's mask, and
    the restated selection. Both paths of sample_history give those bits; without an epsilon it gives what it gave."""
    import torch
    from test_search_depth_cpu import select_depth_ref

    import hanabi_hip
    from hanabi_hip import ConditionedDeterminizer, Determinizer, belief_select_soft_ref, belief_splice_alive, soft_table
    from hanabi_hip.search import _ask

    m, R, ov, turns, seed, depth, eps = 200, 2, 4, 4, 7, 2, 0.1
    K, seat, partner = R * ov, 0, 1
    team, env, hist, rows = _small_game(m, turns, seat, depth, seed)
    live = (((rows[:, 0] >> 19) & 3) == 0).cpu().numpy()
    assert m // 2 < live.sum() < m and hist.filled == depth and bool((hist.valid != 0).all())
    assert type(team[partner]).obs_only_eval is True
    kw = dict(seed=5, draw=turns + 1, partner_seed=seed, first_game_id=0, first_row_id=1000)
    # by hand
    cand, cw = Determinizer(config=env.cfg).sample(rows, seat=seat, replicas=K, seed=5, draw=turns + 1, first_row_id=1000)
    scratch_env = hanabi_hip.HanabiEnv("Hanabi-Small", 2, n_games=m, seed=99, first_game_id=0, auto_reset=False, packed=True)
    moves, scratch = torch.empty(m, dtype=torch.int32, device="cuda"), {}
    hyp, nl = np.empty((depth, K, m), np.int64), np.empty((depth, K, m), np.int64)
    for d in range(depth):
        spliced = belief_splice_alive(env.cfg, hist.prev_rows[d].contiguous(), hist.alive[d].contiguous(), cand, seat, K)
        for k in range(K):
            scratch_env.import_state(spliced[k])
            scratch_env.observe()
            _ask(team[partner], scratch_env, seed, hist.draws[d], moves, scratch)
            hyp[d, k], nl[d, k] = moves.cpu().numpy(), scratch_env.legal.cpu().numpy().astype(np.int64).sum(1)
    actual = hist.moves.cpu().numpy()
    table = soft_table(eps, env.num_actions).numpy()
    want = belief_select_soft_ref(_u32(rows), _u32(cand), cw.cpu().numpy().astype(np.uint32), hyp, nl, actual, None, table, R, 5, turns + 1,
                                  first_row_id=1000, details=True)
    x = want[-1]
    print("n_surv", want[2].sum(1).tolist(), "mean ess", float(want[5].mean()), "legal moves", int(nl.min()), "..", int(nl.max()))
    assert np.array_equal(want[3], depth * live) and np.array_equal(want[4], 2 * ~live) and np.array_equal(x["T"] > 0, live)
    assert np.array_equal(want[1].reshape(m, R), np.repeat(live[:, None], R, 1))
    assert (want[2][0][live] < K).any() and (x["q"].min(1) < x["q"].max(1)).any()   # the moves told something
    assert nl[:, :, live].min() >= 1 and nl.max() <= env.num_actions and len(np.unique(nl[:, :, live])) > 1
    assert (want[5][live] >= 1 - 1e-6).all() and (want[5] <= K + 1e-3).all() and not want[5][~live].any()
    outs = {}
    for stateless in (True, False):
        cd = ConditionedDeterminizer("Hanabi-Small", 2, stateless=stateless)
        got = cd.sample_history(rows, hist, team[partner], seat, R, ov, epsilon=eps, **kw)
        assert got.ess is not None
        assert np.array_equal(_u32(got.rows), want[0]) and np.array_equal(got.weights.cpu().numpy(), want[1].astype(np.int64))
        assert np.array_equal(got.n_surv.cpu().numpy(), want[2]) and np.array_equal(got.depth_used.cpu().numpy(), want[3])
        assert np.array_equal(got.fallback.cpu().numpy(), want[4]) and np.allclose(got.ess.cpu().numpy(), want[5], rtol=1e-6, atol=0)
        outs[stateless] = [t.clone() for t in got]
        # the out= form: the weights come back as the int32 buffer
        buf = (torch.empty_like(got.rows), torch.empty(m * R, dtype=torch.int32, device="cuda"))
        again = cd.sample_history(rows, hist, team[partner], seat, R, ov, epsilon=eps, out=buf, **kw)
        assert again.rows is buf[0] and again.weights is buf[1] and torch.equal(buf[0], got.rows) and torch.equal(buf[1].long(), got.weights)
        # epsilon=None: the exact-match filter, as it was (the same determinizer object, after a soft call)
        hard = cd.sample_history(rows, hist, team[partner], seat, R, ov, **kw)
        ref = select_depth_ref(_u32(rows), _u32(cand), cw.cpu().numpy().astype(np.uint32), hyp, actual, None, K, R)
        assert hard.ess is None and np.array_equal(_u32(hard.rows), ref[0]) and np.array_equal(hard.weights.cpu().numpy(), ref[1].astype(np.int64))
        assert all(np.array_equal(h.cpu().numpy(), r) for h, r in zip((hard.n_surv, hard.depth_used, hard.fallback), ref[2:]))
    for a, b in zip(outs[True], outs[False]):
        assert a.dtype == b.dtype and torch.equal(a, b)
    # sample(): the last move alone, the same figures as depth 1
    cd = ConditionedDeterminizer("Hanabi-Small", 2)
    one = cd.sample(rows, hist.prev_rows[0], team[partner], seat, R, ov, seed=5, draw=turns + 1, partner_seed=seed, partner_draw=hist.draws[0],
                    first_game_id=0, first_row_id=1000, epsilon=eps)
    want1 = belief_select_soft_ref(_u32(rows), _u32(cand), cw.cpu().numpy().astype(np.uint32), hyp[:1], nl[:1], actual[:1], None, table, R, 5,
                                   turns + 1, first_row_id=1000)
    assert one.ess is not None and np.array_equal(_u32(one.rows), want1[0]) and np.array_equal(one.n_surv[0].cpu().numpy(), want1[2][0])
    assert np.array_equal(one.fallback.cpu().numpy(), want1[4]) and np.allclose(one.ess.cpu().numpy(), want1[5], rtol=1e-6, atol=0)


# ---- OffBeliefSession ----------------------------------------------------------------------------------------------------------------------
def test_off_belief_session_with_a_belief_epsilon():
    """150 steps on 200 games of Small with frozen copies as the belief policy. Acting only (train=False), the real game is
    SelfPlaySession's move for move; no row falls back, every live row is conditioned or has no usable move."""
    import torch

    import hanabi_hip
    from hanabi_hip import OffBeliefSession
    from hanabi_hip.obl import frozen_copy
    from hanabi_hip.selfplay import SelfPlaySession

    n, steps = 200, 150

    def run(make):
        torch.manual_seed(0)
        env = hanabi_hip.HanabiEnv("Hanabi-Small", 2, n_games=n, seed=11, packed=True)
        agents = [_dqn(env, seed=s) for s in (1, 2)]
        sess = make(env, agents)
        acts = []
        for _ in range(steps):
            sess.step(train=False)
            acts.append(sess.last_actions[(sess.t - 1) % 2].clone())
        sess.flush()
        torch.cuda.synchronize()
        return torch.stack(acts), env.export_state(), sess

    soft = lambda e, a: OffBeliefSession(e, a, belief_seed=5, belief_policy=[frozen_copy(x) for x in a], depth=2, oversample=4,
                                         belief_epsilon=0.1)
    a_obl, rows_obl, obl = run(soft)
    a_sp, rows_sp, sp = run(SelfPlaySession)
    assert torch.equal(a_obl, a_sp) and torch.equal(rows_obl, rows_sp) and obl.episodes == sp.episodes > 0
    assert obl.belief_epsilon == 0.1 and obl.env_steps == n * steps and obl.branch_steps == n * steps * 2
    c = {k: getattr(obl, k) for k in OffBeliefSession.LEVEL_COUNTERS + ("ess_sum", "dead_rows")}
    print(c)
    assert c["fallback_rows"] == 0 and c["conditioned_rows"] + c["unconditioned_rows"] == n * steps   # (auto-reset: every row is live)
    assert c["conditioned_rows"] > 0 and c["unconditioned_rows"] > 0 and c["dead_rows"] == 0
    assert c["conditioned_rows"] <= c["depth_used_sum"] <= 2 * c["conditioned_rows"] and c["survivors"] <= 4 * c["conditioned_rows"]
    assert c["conditioned_rows"] * (1 - 1e-6) <= c["ess_sum"] <= 4 * c["conditioned_rows"] * (1 + 1e-6)
    assert obl.env.illegal_count() == 0 and obl.scratch.illegal_count() == 0
    # the same session without the epsilon falls back somewhere: the soft filter is what removed the fallbacks
    hard = run(lambda e, a: OffBeliefSession(e, a, belief_seed=5, belief_policy=[frozen_copy(x) for x in a], depth=2, oversample=4))[2]
    assert hard.ess_sum == 0.0 and hard.conditioned_rows + hard.fallback_rows == c["conditioned_rows"]
    assert hard.unconditioned_rows == c["unconditioned_rows"]


def test_off_belief_training_with_a_belief_epsilon_runs_to_the_end():
    import torch

    import hanabi_hip
    from hanabi_hip import OffBeliefSession
    from hanabi_hip.obl import frozen_copy

    n, steps = 200, 150
    env = hanabi_hip.HanabiEnv("Hanabi-Small", 2, n_games=n, seed=11, packed=True)
    agents = [_dqn(env, seed=s) for s in (1, 2)]
    sess = OffBeliefSession(env, agents, belief_policy=[frozen_copy(a) for a in agents], depth=2, belief_epsilon=0.1)
    sess.run(steps)
    torch.cuda.synchronize()
    assert sess.grad_steps > 0 and sess.env_steps == n * steps and sess.branch_steps == n * steps * 2 and sess.dead_rows == 0
    assert env.illegal_count() == 0 and sess.scratch.illegal_count() == 0
    assert sess.fallback_rows == 0 and sess.conditioned_rows + sess.unconditioned_rows == n * steps and sess.ess_sum > 0
    for a in agents:
        assert all(bool(torch.isfinite(p).all()) for p in a.online.parameters())


# ---- SearchPlayer --------------------------------------------------------------------------------------------------------------------------
def test_search_player_with_an_epsilon():
    import torch

    import hanabi_hip
    from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR
    from hanabi_hip import Determinizer, Evaluator, SearchPlayer, belief_select_soft_ref, soft_table

    n, R, ov, D, eps = 64, 3, 4, 2, 0.1
    K = R * ov
    team = [RulebasedAgent(PR.piers_rules, seed=30), RulebasedAgent(PR.piers_rules, seed=31)]
    make = lambda: SearchPlayer(team, 0, replicas=R, seed=2, condition=True, oversample=ov, depth=D, epsilon=eps)
    # the first turns by hand: nothing to condition on at draw 1 (the draws follow the importance weights), both moves' worth at draw 5
    sp = make()
    env = hanabi_hip.HanabiEnv("Hanabi-Small", 2, n_games=n, seed=7, auto_reset=False, packed=True)
    A = env.num_actions
    act = torch.empty(n, dtype=torch.int32, device="cuda")
    rows = env.export_state().clone()
    sp.eval_moves(env, 7, 1, act)
    b = sp._search._sized[(n, A, R)]
    cand, cw = Determinizer(config=env.cfg).sample(rows, seat=0, replicas=K, seed=2, draw=1, first_row_id=0)
    want = belief_select_soft_ref(_u32(rows), _u32(cand), cw.cpu().numpy().astype(np.uint32), np.zeros((D, K, n)), np.ones((D, K, n)),
                                  np.zeros((D, n)), np.zeros((D, n), np.uint8), soft_table(eps, A).numpy(), R, 2, 1)
    assert np.array_equal(_u32(b["det_rows"]), want[0]) and np.array_equal(_u32(b["weights"]), want[1]) and want[1].all()
    res = sp.last_result
    assert bool((res.fallback == 2).all()) and np.allclose(res.ess.cpu().numpy(), want[5], rtol=1e-6, atol=0) and res.ess.shape == (n,)
    assert sp.conditioned == 0 and sp.unconditioned == n and sp.depth_stats()["ess"] == 0.0
    for t in range(1, 5):
        env.step(act)
        if t % 2 == 0:
            sp.eval_moves(env, 7, t + 1, act)
            live = ((env.export_state()[:, 0] >> 19) & 3) == 0
            res = sp.last_result
            assert bool((res.fallback[live] == 0).all()) and bool((res.depth_used[live] == t // 2).all())
            assert bool((res.ess[live] >= 1 - 1e-6).all()) and bool((res.ess[live] <= K + 1e-3).all())
        else:
            team[1].eval_moves(env, 7, t + 1, act)
    assert sp.conditioned > 0 and sp.fallbacks == 0 and 1.0 <= sp.depth_stats()["ess"] <= K
    # whole games through the Evaluator: two runs agree, nothing falls back, the counters add up
    ev = Evaluator("Hanabi-Small", 2, n_games=n, seed=7, record_actions=True)
    runs = []
    for _ in range(2):
        p = make()
        runs.append((ev.run([p, team[1]]), p))
    (ra, pa), (rb, pb) = runs
    assert torch.equal(ra.scores, rb.scores) and torch.equal(ra.actions, rb.actions)
    assert pa.conditioned + pa.unconditioned == pa.moves == int(ra.moves[0].sum()) and pa.fallbacks == 0 and pa.conditioned > 0
    assert pa.candidates == K * pa.conditioned and pa.conditioned <= pa.depth_used <= D * pa.conditioned
    st = pa.depth_stats()
    print({k: getattr(pa, k) for k in SearchPlayer.COUNTERS}, st)
    assert 1.0 <= st["ess"] <= K and st == pb.depth_stats() and st["reached"][0] == pa.conditioned and sum(st["shallow"]) == 0
    for name in SearchPlayer.COUNTERS:
        assert getattr(pa, name) == getattr(pb, name), name
    # depth 1: the last move alone (ConditionedDeterminizer.sample), with a confirming stage on the same belief
    one = SearchPlayer(team, 0, replicas=R, seed=2, z=1.0, confirm_replicas=4, condition=True, oversample=ov, epsilon=eps)
    r1 = ev.run([one, team[1]])
    assert one.conditioned + one.unconditioned == one.moves == int(r1.moves[0].sum()) and one.fallbacks == 0 and one.conditioned > 0
    assert one.depth_used == one.conditioned and 1.0 <= one.depth_stats()["ess"] <= K
