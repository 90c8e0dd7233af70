"""The search belief conditioned on the partner's last L moves, on the GPU (hanabi_hip.search, csrc/belief.hip):
hb_belief_splice_alive and hb_belief_select_depth against the numpy restatements of tests/test_search_depth_cpu.py byte for byte
and against the depth-1 restatements of tests/test_search_belief_cpu.py, ConditionedDeterminizer.sample_history against a rerun by hand, and the guarantees of
SearchPlayer(condition=True, depth=L) and session.search(history=PartnerHistory)."""
import numpy as np
import pytest
from search_util import _mid_game_env, _u32

pytestmark = pytest.mark.gpu

# (game, players, observer, turns played, roots): more than one workgroup of four roots, an odd count, a 48-word state
SHAPES = [("Hanabi-Full", 2, 1, 14, 256), ("Hanabi-Full", 5, 3, 17, 8), ("Hanabi-Small", 2, 0, 6, 37)]


def _rows_and_candidates(game, players, seat, turns, m, K):
    """(env, earlier rows, rows, candidates of rows, weights): m running games, `earlier` one round of the table before."""
    import torch

    from hanabi_hip import Determinizer

    env = _mid_game_env(game, players, 12 * m, turns)
    earlier = env.export_state()
    for t in range(players):
        env.step(env.random_legal_actions(seed=9, draw=100 + t))
    rows = env.export_state()
    keep = (((rows[:, 0] >> 19) & 3) == 0).nonzero().view(-1)[:m]
    assert keep.numel() == m
    earlier, rows = earlier[keep].contiguous(), rows[keep].contiguous()
    det_rows = torch.empty((m * K, rows.shape[1]), dtype=torch.int32, device="cuda")
    w = torch.empty(m * K, dtype=torch.int32, device="cuda")
    Determinizer(config=env.cfg).sample(rows, seat=seat, replicas=K, seed=9, draw=4, out=(det_rows, w))
    return env, earlier, rows, det_rows, w


@pytest.mark.parametrize("game,players,seat,turns,m", SHAPES)
@pytest.mark.parametrize("K", [5, 70])
def test_splice_alive_equals_the_restatement(game, players, seat, turns, m, K):
    import torch
    from test_search_belief_cpu import splice_ref
    from test_search_depth_cpu import splice_alive_ref

    from hanabi_hip import belief_splice_alive

    env, earlier, rows, det_rows, _ = _rows_and_candidates(game, players, seat, turns, m, K)
    assert env.state_words == (48 if players == 5 else 32)
    earlier[0, 0] |= 2 << 19   # a finished game among the roots: spliced like any other row
    rng = np.random.default_rng(K)
    alive = rng.integers(0, 256, m).astype(np.uint8)   # every mask, the bits of empty slots and bits 5 - 7 among them
    alive[:4] = [0, 0x1F, 0xFF, 1]
    earlier[1, 10 + seat] |= 31 << 20                  # an older hand of four: its fifth slot stays empty under an alive bit
    earlier[3, 10 + seat] |= 1023 << 15                # ... and one of three under a candidate of more
    out = belief_splice_alive(env.cfg, earlier, torch.as_tensor(alive).cuda(), det_rows, seat, K)
    assert out.shape == (K, m, env.state_words)
    want = splice_alive_ref(_u32(earlier), alive, _u32(det_rows), seat, K)
    assert np.array_equal(_u32(out).reshape(K * m, -1), want)
    assert (want[:m, 10 + seat] != _u32(earlier)[:, 10 + seat]).any() and (want[:m, 10 + seat] != _u32(det_rows)[::K, 10 + seat]).any()
    # alive = NULL is every slot alive; on the candidates' own rows (equal hand sizes) that is the whole hand word taken over
    every = belief_splice_alive(env.cfg, earlier, None, det_rows, seat, K)
    assert np.array_equal(_u32(every).reshape(K * m, -1), splice_alive_ref(_u32(earlier), None, _u32(det_rows), seat, K))
    own = belief_splice_alive(env.cfg, rows, None, det_rows, seat, K)
    assert np.array_equal(_u32(own).reshape(K * m, -1), splice_ref(_u32(rows), _u32(det_rows), seat, K))
    buf = torch.empty_like(out)
    assert belief_splice_alive(env.cfg, earlier, torch.as_tensor(alive).cuda(), det_rows, seat, K, out=buf) is buf and torch.equal(buf, out)


def _select_depth_both(cfg, rows, det_rows, w, hyp, actual, valid, K, R):
    import torch
    from test_search_depth_cpu import select_depth_ref

    from hanabi_hip import belief_select_depth

    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a).astype(dt)).cuda()
    got = belief_select_depth(cfg, rows, det_rows, w, t(hyp, np.int32), t(actual, np.int32), None if valid is None else t(valid, np.uint8), R)
    want = select_depth_ref(_u32(rows), _u32(det_rows), _u32(w), hyp, actual, valid, K, R)
    for g, x, name in zip(got, want, ("rows", "weights", "n_surv", "depth_used", "fallback")):
        assert np.array_equal(_u32(g) if name in ("rows", "weights") else g.cpu().numpy(), x), name
    return got, want


def _branches(m, K, D, rng, w):
    """hyp [D, K, m], actual [D, m], valid [D, m] with every branch in roots 0 .. 7 (root 7 is finished by the caller) and
    random moves in the others; `w` [m, K] is edited in place."""
    actual = rng.integers(0, 3, (D, m))
    hyp = rng.integers(0, 3, (D, K, m))
    hyp[:, :, :8] = 9
    valid = np.ones((D, m), np.uint8)
    valid[:, 8:] = rng.integers(0, 4, (D, max(m - 8, 0))) != 0
    every = np.arange(K)
    hyp[:, :, 0] = actual[:, None, 0]                          # root 0: every candidate reproduces every move
    hyp[0, every[every % 3 != 1], 1] = actual[0, 1]            # root 1: the deepest level decides, across the chunk boundaries
    hyp[1:, every[every % 2 == 0], 1] = actual[1:, None, 1]
    hyp[0, [2, K - 1], 2] = actual[0, 2]                       # root 2: fewer survivors than replicas, the last candidate among them
    hyp[1:, :, 2] = actual[1:, None, 2]
    hyp[1:, :, 3] = actual[1:, None, 3]                        # root 3: nobody reproduces the newest move: fallback 1
    valid[:, 4] = 0                                            # root 4: all invalid although every move matches
    hyp[:, :, 4] = actual[:, None, 4]
    hyp[:, :, 5] = actual[:, None, 5]                          # root 5: an invalid middle entry cuts the chain
    valid[min(1, D - 1), 5] = 0 if D > 1 else 1
    hyp[:, :, 6] = actual[:, None, 6]                          # root 6: every second candidate dead, their moves match all the same;
    w[6, ::2] = 0                                              # ... and nobody reproduces the oldest move: depth_used < L
    hyp[D - 1, :, 6] = 9 if D > 1 else actual[0, 6]
    hyp[:, :, 7] = actual[:, None, 7]
    w[7] = 0
    return hyp, actual, valid


@pytest.mark.parametrize("game,players,seat,turns,m", SHAPES)
@pytest.mark.parametrize("K", [5, 70, 130])
@pytest.mark.parametrize("depth", [1, 2, 3, 8])
def test_select_depth_equals_the_restatement(game, players, seat, turns, m, K, depth):
    """Every branch in one call, the survivors on both sides of the 64-candidate chunk boundaries, a finished root (7) and an
    all-invalid root (4) among them; and, at depth 1, the depth-1 restatement of hb_belief_select byte for byte."""
    import torch
    from test_search_belief_cpu import select_ref

    R = 5
    env, _, rows, det_rows, w = _rows_and_candidates(game, players, seat, turns, m, K)
    rows[7, 0] |= 1 << 19
    rng = np.random.default_rng(100 * depth + K)
    wv = w.view(m, K).cpu().numpy().copy()
    hyp, actual, valid = _branches(m, K, depth, rng, wv)
    w = torch.as_tensor(wv).cuda().view(-1)
    got, (_, ow, n_surv, used, fallback) = _select_depth_both(env.cfg, rows, det_rows, w, hyp, actual, valid, K, R)
    last = depth - 1
    assert used[:8].tolist() == [depth, depth, depth, 0, 0, 1, max(depth - 1, 1), 0]
    assert fallback[:8].tolist() == [0, 0, 0, 1, 2, 0, 0, 2]
    assert n_surv[last, 0] == K and n_surv[0, 1] == K - (K + 1) // 3 and n_surv[last, 2] == 2 and n_surv[:, 3].sum() == 0
    assert n_surv[0, 5] == K and (depth == 1 or n_surv[1:, 5].sum() == 0) and n_surv[0, 6] == K // 2
    assert (depth == 1 or n_surv[last, 6] == 0) and (ow.reshape(m, R)[2, 2:] == 0).all() and (ow.reshape(m, R)[2, :2] != 0).all()
    _select_depth_both(env.cfg, rows, det_rows, w, hyp, actual, None, K, R)   # valid = NULL: every entry valid
    if depth == 1:
        one = select_ref(_u32(rows), _u32(det_rows), _u32(w), hyp[0], actual[0], valid[0], K, R)
        assert np.array_equal(_u32(got[0]), one[0]) and np.array_equal(_u32(got[1]), one[1])
        assert np.array_equal(got[2][0].cpu().numpy(), one[2]) and np.array_equal(got[4].cpu().numpy(), one[3])
        assert np.array_equal(got[3].cpu().numpy(), (one[3] == 0).astype(np.int32))


# ---- sample_history -------------------------------------------------------------------------------------------------------------------
def _piers_game(m, turns, seat, depth, seed=7):
    """m games of [Piers, Piers] on Full, turn by turn as Evaluator.run keys it, with `seat` keeping a PartnerHistory as
    SearchPlayer does. -> (team, env, history, rows, the true states the partner moved from [newest first])."""
    import torch

    import hanabi_hip
    from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR
    from hanabi_hip import PartnerHistory, last_move_uid

    team = [RulebasedAgent(PR.piers_rules, seed=11), RulebasedAgent(PR.piers_rules, seed=12)]
    env = hanabi_hip.HanabiEnv("Hanabi-Full", 2, n_games=m, seed=seed, auto_reset=False, packed=True)
    hist = PartnerHistory(env.cfg, m, depth, "cuda", partner_seed=seed, first_game_id=0)
    act = torch.empty(m, dtype=torch.int32, device="cuda")
    states, mine, stored = [env.export_state()], None, []
    for t in range(turns + 1):
        rows = states[-1]
        if t % 2 == seat and t >= 1:   # my turn, draw t + 1: the partner moved from states[-2] with draw t
            if mine is not None:
                hist.own_move(mine)
            hist.push(states[-2], last_move_uid(env.cfg, rows), t, torch.ones(m, dtype=torch.uint8), seat=seat)
            stored = ([states[-2]] + stored)[:depth]
        if t == turns:
            break
        team[t % 2].eval_moves(env, seed, t + 1, act)
        if t % 2 == seat:
            mine = act.clone()
        env.step(act)
        states.append(env.export_state())
    assert turns % 2 == seat
    return team, env, hist, states[-1], stored


def test_sample_history_against_a_rerun_by_hand():
    import torch
    from test_search_depth_cpu import select_depth_ref, splice_alive_ref

    import hanabi_hip
    from hanabi_hip import ConditionedDeterminizer, Determinizer, belief_splice_alive

    m, R, ov, turns, seed, depth = 8, 8, 8, 12, 7, 3
    K, seat, partner = R * ov, 0, 1
    team, env, hist, rows, stored = _piers_game(m, turns, seat, depth, seed)
    assert bool((((rows[:, 0] >> 19) & 3) == 0).all()) and hist.filled == depth and hist.draws == [turns, turns - 2, turns - 4]
    # the true hand, spliced with the tracked masks, reproduces every stored state; some card of the oldest has left the hand
    for d in range(depth):
        assert torch.equal(hist.prev_rows[d], stored[d])
        assert torch.equal(belief_splice_alive(env.cfg, stored[d], hist.alive[d].contiguous(), rows, seat, 1)[0], stored[d])
    occupied = (((stored[-1][:, 10 + seat].view(m, 1) >> (5 * torch.arange(5, device="cuda"))) & 31) != 31).int()
    assert bool((hist.alive[-1].int() != (occupied << torch.arange(5, device="cuda")).sum(1)).any())
    cd = ConditionedDeterminizer("Hanabi-Full", 2)
    smp = cd.sample_history(rows, hist, team[partner], seat, R, ov, seed=5, draw=turns + 1, partner_seed=seed, first_game_id=0,
                            first_row_id=100)
    out, w, n_surv, used, fallback = smp.rows, smp.weights, smp.n_surv, smp.depth_used, smp.fallback
    # by hand: the candidates, the restated splice, one scratch import per (entry, candidate), the real game's keys
    cand, cw = Determinizer("Hanabi-Full", 2).sample(rows, seat=seat, replicas=K, seed=5, draw=turns + 1, first_row_id=100)
    scratch = hanabi_hip.HanabiEnv("Hanabi-Full", 2, n_games=m, seed=99, first_game_id=0, auto_reset=False, packed=True)
    moves = torch.empty(m, dtype=torch.int32, device="cuda")
    actual = hist.moves.cpu().numpy()

    def partner_moves(d, det_rows):
        """The partner's move at entry d with the hands of det_rows [m, SW] carried back."""
        spliced = splice_alive_ref(_u32(stored[d]), hist.alive[d].cpu().numpy(), _u32(det_rows), seat, 1)
        scratch.import_state(torch.as_tensor(spliced.view(np.int32)).cuda())
        return team[partner].eval_moves(scratch, seed, hist.draws[d], moves).cpu().numpy().copy()

    for d in range(depth):   # the true hand gives the real move at every depth
        assert np.array_equal(partner_moves(d, rows), actual[d])
    cand_v = cand.view(m, K, -1)
    hyp = np.stack([np.stack([partner_moves(d, cand_v[:, k].contiguous()) for k in range(K)]) for d in range(depth)])   # [D, K, m]
    want = select_depth_ref(_u32(rows), _u32(cand), cw.cpu().numpy().astype(np.uint32), hyp, actual, None, K, R)
    assert np.array_equal(_u32(out), want[0]) and np.array_equal(w.cpu().numpy(), want[1].astype(np.int64))
    assert np.array_equal(n_surv.cpu().numpy(), want[2]) and np.array_equal(used.cpu().numpy(), want[3])
    assert np.array_equal(fallback.cpu().numpy(), want[4])
    print("n_surv", n_surv.tolist(), "depth_used", used.tolist(), "fallback", fallback.tolist())
    # read off the outputs themselves: every survivor reproduces the partner's move at every depth up to depth_used
    out_v = out.view(m, R, -1)
    for j in range(R):
        for d in range(depth):
            got = partner_moves(d, out_v[:, j].contiguous())
            for i in range(m):
                if d < int(used[i]) and j < int(n_surv[int(used[i]) - 1, i]):
                    assert got[i] == actual[d, i]
    ns = n_surv.cpu().numpy()
    assert (ns[1:] <= ns[:-1]).all() and (ns[0] < K).any() and (ns[-1] < ns[0]).any()   # the older moves filter further
    assert int((used == depth).sum()) >= 1 and int((fallback == 0).sum()) >= 1
    # an invalid middle entry: its root is filtered on the newest move alone; the out= form
    hist.valid[1, 1::2] = 0
    buf = (torch.empty_like(out), torch.empty(m * R, dtype=torch.int32, device="cuda"))
    smp2 = cd.sample_history(rows, hist, team[partner], seat, R, ov, seed=5, draw=turns + 1, partner_seed=seed, first_game_id=0,
                             first_row_id=100, out=buf)
    o2, w2, ns2, du2, fb2 = smp2.rows, smp2.weights, smp2.n_surv, smp2.depth_used, smp2.fallback
    assert o2 is buf[0] and w2 is buf[1]
    assert torch.equal(du2[1::2], (n_surv[0, 1::2] > 0).int()) and bool((ns2[1:, 1::2] == 0).all()) and torch.equal(ns2[:, 0::2], n_surv[:, 0::2])
    assert torch.equal(o2.view(m, R, -1)[0::2], out_v[0::2]) and torch.equal(du2[0::2], used[0::2]) and torch.equal(ns2[0], n_surv[0])


# ---- SearchPlayer ------------------------------------------------------------------------------------------------------------------------
def test_search_player_depth_1_is_the_conditioned_player_as_it_was():
    import torch

    import hanabi_hip
    from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR
    from hanabi_hip import Evaluator, SearchPlayer

    team = [RulebasedAgent(PR.piers_rules, seed=30), RulebasedAgent(PR.piers_rules, seed=31)]
    ev = Evaluator("Hanabi-Full", 2, n_games=16, seed=7, record_actions=True)
    old = SearchPlayer(team, 0, replicas=3, seed=2, z=1.0, condition=True, oversample=4)
    new = SearchPlayer(team, 0, replicas=3, seed=2, z=1.0, condition=True, oversample=4, depth=1)
    a, b = ev.run([old, team[1]]), ev.run([new, team[1]])
    assert torch.equal(a.scores, b.scores) and torch.equal(a.actions, b.actions) and torch.equal(a.lengths, b.lengths)
    for name in SearchPlayer.COUNTERS + ("rollouts", "dead_replicas", "replicas_drawn", "searches"):
        assert getattr(old, name) == getattr(new, name), name
    assert old.conditioned > 0 and old.deviations > 0 and old.depth_used == old.conditioned - old.fallbacks
    # last_result, call by call: both players are asked on the same env at the same draw
    env = hanabi_hip.HanabiEnv("Hanabi-Full", 2, n_games=16, seed=7, auto_reset=False, packed=True)
    act, act2 = (torch.empty(16, dtype=torch.int32, device="cuda") for _ in range(2))
    for t in range(7):
        if t % 2 == 0:
            old.eval_moves(env, 7, t + 1, act)
            new.eval_moves(env, 7, t + 1, act2)
            ra, rb = old.last_result, new.last_result
            assert torch.equal(act, act2) and torch.equal(torch.nan_to_num(ra.value), torch.nan_to_num(rb.value))
            assert torch.equal(ra.n_surv, rb.n_surv) and torch.equal(ra.fallback, rb.fallback) and torch.equal(ra.best, rb.best)
            assert rb.n_surv.shape == (16,) and rb.depth_used is None and new._history is None
            assert bool((rb.fallback == 0).any()) == (t >= 2)
        else:
            team[1].eval_moves(env, 7, t + 1, act)
        env.step(act)


def test_search_player_depth_2():
    import torch

    import hanabi_hip
    from hanabi_agents.rule_based import RulebasedAgent, Ruleset, predefined_rules as PR
    from hanabi_hip import Evaluator, SearchPlayer

    n, Kc = 16, 6
    # A partner whose rule never reads the other hand (tests/test_search_belief_gpu.py: [discard_oldest_first] wherever it
    # fires, i.e. where its move is uid 0): every candidate survives at every depth whose moves were all such moves
    blind = [RulebasedAgent(PR.piers_rules, seed=30), RulebasedAgent([Ruleset.discard_oldest_first], seed=31)]
    sp = SearchPlayer(blind, 0, replicas=2, seed=2, condition=True, oversample=3, depth=2)
    env = hanabi_hip.HanabiEnv("Hanabi-Full", 2, n_games=n, seed=7, auto_reset=False, packed=True)
    act = torch.empty(n, dtype=torch.int32, device="cuda")
    deep_roots = 0
    for t in range(13):
        if t % 2 == 0:
            sp.eval_moves(env, 7, t + 1, act)
            res, h = sp.last_result, sp._history
            assert res.n_surv.shape == (2, n) and res.depth_used.shape == (n,) and h.filled == min(t // 2, 2)
            assert bool((res.depth_used <= 2).all()) and torch.equal(res.depth_used == 0, res.fallback != 0)
            assert bool((res.n_surv <= Kc).all()) and bool((res.n_surv[1] <= res.n_surv[0]).all())
            if t >= 2:
                have = (h.valid != 0).long().cumprod(0).sum(0)   # (every game is still running)
                fired = ((h.moves == 0) & (h.valid != 0)).long().cumprod(0)
                for D in (1, 2):
                    sel = (have >= D) & (fired[D - 1] != 0)
                    assert bool((res.n_surv[D - 1][sel] == Kc).all()) and bool((res.depth_used[sel] >= D).all())
                    deep_roots += int(sel.sum()) if D == 2 else 0
                assert bool((have == 2).any()) == (t >= 4) and bool((res.n_surv[1][have < 2] == 0).all())
        else:
            blind[1].eval_moves(env, 7, t + 1, act)
        env.step(act)
    print("roots whose partner discarded twice in a row:", deep_roots)
    assert deep_roots >= 1
    # [Piers, Piers], both seats searching at depth 2 with a confirming stage: two runs agree move for move, the counters add up
    ev = Evaluator("Hanabi-Full", 2, n_games=n, seed=7, record_actions=True)
    team = [RulebasedAgent(PR.piers_rules, seed=30), RulebasedAgent(PR.piers_rules, seed=31)]
    runs = []
    for _ in range(2):
        pair = [SearchPlayer(team, s, replicas=3, seed=2, z=1.0, confirm_replicas=4, condition=True, oversample=4, depth=2) for s in (0, 1)]
        runs.append((ev.run(pair), pair))
    (ra, pa), (rb, pb) = runs
    assert torch.equal(ra.scores, rb.scores) and torch.equal(ra.actions, rb.actions)
    for s in (0, 1):
        p, st = pa[s], pa[s].depth_stats()
        assert p.conditioned + p.unconditioned == p.moves == int(ra.moves[s].sum())
        assert 0 < p.survivors < p.candidates == 12 * p.conditioned
        assert st["reached"][0] == p.conditioned and 0 < st["reached"][1] < st["reached"][0]
        assert sum(st["used"]) == p.conditioned - p.fallbacks and st["used"][0] + 2 * st["used"][1] == p.depth_used
        assert st["survivors"][1] < st["survivors"][0] and st["used"][1] > 0
        assert st["shallow"][0] <= p.fallbacks <= sum(st["shallow"]) <= p.conditioned - st["used"][1]
        for name in SearchPlayer.COUNTERS:
            assert getattr(p, name) == getattr(pb[s], name), name
        assert st == pb[s].depth_stats()
        p.reset_stats()
        assert p.depth_used == 0 and p.depth_stats()["reached"] == [0, 0]


def test_session_search_with_a_partner_history_leaves_the_session_untouched(monkeypatch):
    import torch
    from test_search_gpu import _assert_same, _session_state

    import hanabi_hip
    from hanabi_agents.rlax_dqn import ActionSpec, DQNAgent, ObservationSpec, RlaxRainbowParams
    from hanabi_hip import PartnerHistory, last_move_uid
    from hanabi_hip.selfplay import SelfPlaySession

    monkeypatch.setenv("HB_ACTOR_FUSED_MIN_ROWS", "0")
    n = 128
    torch.manual_seed(0)
    torch.cuda.manual_seed(0)
    flags = hanabi_hip.FLAG_AUTO_RESET | hanabi_hip.FLAG_RESET_START_NEXT
    env = hanabi_hip.HanabiEnv(config=hanabi_hip.make_config("Hanabi-Full", 2, flags), n_games=n, seed=5, packed=True)
    params = RlaxRainbowParams(train_batch_size=128, experience_buffer_size=n * 8, mask_terminal=True, target_update_period=6,
                               compute_dtype="bfloat16", packed_obs=True, layers=[512], learning_rate=0.01)
    mk = lambda s: DQNAgent(ObservationSpec((n, env.obs_len)), ActionSpec(env.num_actions), params._replace(seed=s), device="cuda")
    sess = SelfPlaySession(env, [mk(1), mk(2)])
    sess.run(19)
    prev = sess.env.export_state()
    sess.run(1)
    rows = sess.env.export_state()
    hist = PartnerHistory(sess.env.cfg, n, 2, "cuda", partner_seed=5, first_game_id=sess.env.first_game_id)
    valid = ((rows[:, 2] & 1) != 0).to(torch.uint8)   # (a game that was just dealt again has no last move)
    hist.push(prev, last_move_uid(sess.env.cfg, rows), 20, valid)
    before = _session_state(sess)
    res = sess.search(replicas=2, seed=3, history=hist, oversample=2)
    _assert_same(before, _session_state(sess))
    assert res.n_surv.shape == (2, n) and res.fallback.shape == (n,) and res.depth_used.shape == (n,) and res.rollouts > 0
    assert bool((res.n_surv <= 4).all()) and bool((res.n_surv[1] == 0).all()) and bool((res.depth_used <= 1).all())
    one = sess.search(replicas=2, seed=3, history=(prev, 5, 20, sess.env.first_game_id, valid), oversample=2)
    assert one.depth_used is None and torch.equal(one.n_surv, res.n_surv[0]) and torch.equal(one.fallback, res.fallback)
    assert torch.equal(torch.nan_to_num(one.value), torch.nan_to_num(res.value))
    _assert_same(before, _session_state(sess))
    with pytest.raises(ValueError, match="roots"):
        sess.search(replicas=2, seed=3, history=PartnerHistory(sess.env.cfg, 5, 2, "cuda"))
