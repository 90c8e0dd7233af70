"""The search belief conditioned on the partner's last move, on the GPU (hanabi_hip.search, csrc/belief.hip): hb_belief_splice
and hb_belief_select against the numpy restatement of tests/test_search_belief_cpu.py byte for byte,
ConditionedDeterminizer.sample against a rerun by hand, the reconstruction of the state the partner moved from, the
guarantees of SearchPlayer(condition=True) and session.search(history=), and the games SearchPlayer(condition=True) plays
against a recording (tests/golden/search_belief_lastmove.json)."""
import json
import os

import numpy as np
import pytest
from search_util import _conditioned_games, _dqn, _u32

pytestmark = pytest.mark.gpu


def _played(game, players, n, turns, seed=3):
    """(env, prev_rows, rows): a non-resetting env after `turns` random legal moves, and n of its rows that are still running,
    before and after the last of them."""
    import hanabi_hip

    env = hanabi_hip.HanabiEnv(game, players, n_games=8 * n, seed=seed, auto_reset=False, packed=True)
    prev = None
    for t in range(turns):
        prev = env.export_state()
        env.step(env.random_legal_actions(seed=seed + 1, draw=t))
    rows = env.export_state()
    keep = (((rows[:, 0] >> 19) & 3) == 0).nonzero().view(-1)[:n]   # the first n games still running
    assert keep.numel() == n
    return env, prev[keep].contiguous(), rows[keep].contiguous()


def _candidates(env, rows, seat, K):
    import torch

    from hanabi_hip import Determinizer

    det_rows = torch.empty((rows.shape[0] * K, rows.shape[1]), dtype=torch.int32, device="cuda")
    w = torch.empty(rows.shape[0] * K, dtype=torch.int32, device="cuda")
    Determinizer(config=env.cfg).sample(rows, seat=seat, replicas=K, seed=9, draw=4, out=(det_rows, w))
    return det_rows, w


SHAPES = [("Hanabi-Full", 2, 1, 14), ("Hanabi-Full", 5, 3, 17), ("Hanabi-Small", 2, 0, 6)]


@pytest.mark.parametrize("game,players,seat,turns", SHAPES)
def test_splice_equals_the_restatement(game, players, seat, turns):
    import torch
    from test_search_belief_cpu import splice_ref

    from hanabi_hip import belief_splice

    m, K = 3, 70
    env, prev, rows = _played(game, players, m, turns)
    assert env.state_words == (48 if players == 5 else 32)
    rows[0, 0] |= 2 << 19   # a finished game among the roots: spliced like any other row
    prev[0, 0] |= 2 << 19
    det_rows, _ = _candidates(env, rows, seat, K)
    out = belief_splice(env.cfg, prev, det_rows, seat, K)
    assert out.shape == (K, m, env.state_words)
    want = splice_ref(_u32(prev), _u32(det_rows), seat, K)
    assert np.array_equal(_u32(out).reshape(K * m, -1), want)
    assert not torch.equal(out[0], out[1])   # (the candidates differ)
    one = belief_splice(env.cfg, prev, det_rows[::K].contiguous(), seat, 1)   # K = 1: candidate-major and root-major coincide
    assert np.array_equal(_u32(one).reshape(m, -1), splice_ref(_u32(prev), _u32(det_rows[::K]), seat, 1))


def _select_both(cfg, rows, det_rows, w, hyp, actual, valid, K, R):
    import torch
    from test_search_belief_cpu import select_ref

    from hanabi_hip import belief_select

    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a).astype(dt)).cuda()
    got = belief_select(cfg, rows, det_rows, w, t(hyp, np.int32), t(actual, np.int32), None if valid is None else t(valid, np.uint8), R)
    want = select_ref(_u32(rows), _u32(det_rows), _u32(w), hyp, actual, valid, K, R)
    assert np.array_equal(_u32(got[0]), want[0]), "rows"
    assert np.array_equal(_u32(got[1]), want[1]), "weights"
    assert np.array_equal(got[2].cpu().numpy(), want[2]), "n_surv"
    assert np.array_equal(got[3].cpu().numpy(), want[3]), "fallback"
    return want


@pytest.mark.parametrize("game,players,seat,turns", SHAPES)
@pytest.mark.parametrize("K", [70, 5, 130])
def test_select_equals_the_restatement(game, players, seat, turns, K):
    m, R = 3, 5
    env, prev, rows = _played(game, players, m, turns)
    rows[0, 0] |= 2 << 19   # a finished game: fallback 2 whatever the moves say
    det_rows, w = _candidates(env, rows, seat, K)
    rng = np.random.default_rng(K)
    hyp = rng.integers(0, 3, (K, m))
    actual = np.array([1, 1, 2])
    _, _, n_surv, fallback = _select_both(env.cfg, rows, det_rows, w, hyp, actual, None, K, R)
    assert fallback[0] == 2 and (K < 70 or (fallback[1:] == 0).all() and (n_surv[1:] > R).all())
    _select_both(env.cfg, rows, det_rows, w, hyp, actual, np.array([1, 0, 1], np.uint8), K, R)


@pytest.mark.parametrize("K", [70, 130])
def test_select_every_branch_in_one_call(K):
    """One call in which every branch of tests/test_search_belief_cpu.py's hand-worked list occurs, the survivors placed on both
    sides of the 64-candidate chunk boundaries."""
    import torch

    m, R, seat = 8, 5, 0
    env, prev, rows = _played("Hanabi-Full", 2, m, 14)
    rows[7, 0] |= 1 << 19                          # root 7: finished
    det_rows, w = _candidates(env, rows, seat, K)
    w = w.clone()
    w.view(m, K)[5, ::2] = 0                       # root 5: every second candidate dead, their moves match all the same
    w.view(m, K)[7] = 0
    hyp = np.full((K, m), 3)
    actual = np.full(m, 7)
    hyp[:, 0] = 7                                  # root 0: all survive
    hyp[[2, 63, 64, 65, K - 1], 1] = 7             # root 1: interleaved, across the chunk boundary, the last candidate among them
    hyp[[63, K - 1], 2] = 7                        # root 2: 0 < n_surv < R
    hyp[:, 4] = 7                                  # root 3: none; root 4: valid = 0 although every move matches
    hyp[:, 5] = 7
    hyp[[66, 67], 6] = 7                           # root 6: the first survivor sits in the second chunk
    hyp[:, 7] = 7
    valid = np.array([1, 1, 1, 1, 0, 1, 1, 1], np.uint8)
    _, ow, n_surv, fallback = _select_both(env.cfg, rows, det_rows, w, hyp, actual, valid, K, R)
    assert n_surv.tolist() == [K, 5, 2, 0, 0, K // 2, 2, 0] and fallback.tolist() == [0, 0, 0, 1, 2, 0, 0, 2]
    assert (ow.reshape(m, R)[2, 2:] == 0).all() and (ow.reshape(m, R)[2, :2] != 0).all()
    assert torch.cuda.is_available()


def _piers_roots(m, turns, seed=7):
    """m games `turns` turns into [Piers, Piers] play, turn by turn as Evaluator.run keys it (seed, draw = turn + 1, game id)."""
    import torch

    import hanabi_hip
    from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR

    team = [RulebasedAgent(PR.piers_rules, seed=11), RulebasedAgent(PR.piers_rules, seed=12)]
    env = hanabi_hip.HanabiEnv("Hanabi-Full", 2, n_games=m, seed=seed, auto_reset=False, packed=True)
    act = torch.empty(m, dtype=torch.int32, device="cuda")
    prev = None
    for t in range(turns):
        team[t % 2].eval_moves(env, seed, t + 1, act)
        prev = env.export_state()
        env.step(act)
    return team, env, prev, env.export_state(), act.clone()


def test_conditioned_determinizer_against_a_rerun_by_hand():
    import torch
    from test_search_belief_cpu import select_ref

    import hanabi_hip
    from hanabi_hip import ConditionedDeterminizer, Determinizer, last_move_uid

    m, R, ov, turns, seed = 8, 8, 8, 10, 7
    K = R * ov
    team, env, prev, rows, played = _piers_roots(m, turns, seed)
    seat, partner = turns % 2, (turns - 1) % 2
    assert bool((((rows[:, 0] >> 19) & 3) == 0).all())
    assert torch.equal(last_move_uid(env.cfg, rows), played)
    cd = ConditionedDeterminizer("Hanabi-Full", 2)
    smp = cd.sample(rows, prev, team[partner], seat, R, ov, seed=5, draw=turns + 1, partner_seed=seed, partner_draw=turns,
                    first_game_id=0, first_row_id=100)
    out, w, n_surv, fallback = smp.rows, smp.weights, smp.n_surv[0], smp.fallback
    # by hand: the candidates, one scratch import per candidate, the partner's eval_moves with the real game's keys
    cand, cw = Determinizer("Hanabi-Full", 2).sample(rows, seat=seat, replicas=K, seed=5, draw=turns + 1, first_row_id=100)
    scratch = hanabi_hip.HanabiEnv("Hanabi-Full", 2, n_games=m, seed=99, first_game_id=0, auto_reset=False, packed=True)
    moves = torch.empty(m, dtype=torch.int32, device="cuda")

    def partner_moves(hand_words):
        spliced = prev.clone()
        spliced[:, 10 + seat] = hand_words
        scratch.import_state(spliced)
        return team[partner].eval_moves(scratch, seed, turns, moves).cpu().numpy().copy()

    # the true hand gives the real move: the previous state and the (seed, draw, game id) keying are the real game's
    assert np.array_equal(partner_moves(rows[:, 10 + seat]), played.cpu().numpy())
    hyp = np.stack([partner_moves(cand.view(m, K, -1)[:, k, 10 + seat]) for k in range(K)])   # [K, m]
    want = select_ref(_u32(rows), _u32(cand), cw.cpu().numpy().astype(np.uint32), hyp, played.cpu().numpy(), None, K, R)
    assert np.array_equal(_u32(out), want[0]) and np.array_equal(w.cpu().numpy(), want[1].astype(np.int64))
    assert np.array_equal(n_surv.cpu().numpy(), want[2]) and np.array_equal(fallback.cpu().numpy(), want[3])
    # ... and read off the outputs themselves: every survivor reproduces the move, every candidate passed over does not
    actual = played.cpu().numpy()
    out_hands = out.view(m, R, -1)[:, :, 10 + seat]
    cand_hands = cand.view(m, K, -1)[:, :, 10 + seat].cpu().numpy()
    some_filtered = False
    for j in range(R):
        got = partner_moves(out_hands[:, j].contiguous())
        for i in range(m):
            if fallback[i] == 0 and j < int(n_surv[i]):
                assert got[i] == actual[i]
    for i in range(m):
        if int(fallback[i]) != 0:
            continue
        taken, k = 0, 0
        while taken < min(R, int(n_surv[i])):
            if hyp[k, i] == actual[i]:
                assert cand_hands[i, k] == int(out_hands[i, taken])
                taken += 1
            else:
                some_filtered = True
            k += 1
    print("n_surv", n_surv.tolist(), "fallback", fallback.tolist())
    assert some_filtered and int((fallback == 0).sum()) >= 1
    assert bool((n_surv <= K).all()) and bool((n_surv[fallback == 0] > 0).all())
    # valid = 0 and the out= form
    buf = (torch.empty_like(out), torch.empty(m * R, dtype=torch.int32, device="cuda"))
    valid = torch.tensor([1, 0] * (m // 2), dtype=torch.uint8, device="cuda")
    smp2 = cd.sample(rows, prev, team[partner], seat, R, ov, seed=5, draw=turns + 1, partner_seed=seed, partner_draw=turns,
                     first_game_id=0, valid=valid, first_row_id=100, out=buf)
    o2, w2, ns2, fb2 = smp2.rows, smp2.weights, smp2.n_surv[0], smp2.fallback
    assert o2 is buf[0] and w2 is buf[1]
    assert bool((fb2[1::2] == 2).all()) and torch.equal(fb2[0::2], fallback[0::2]) and torch.equal(ns2[0::2], n_surv[0::2])
    assert torch.equal(o2.view(m, R, -1)[1::2], cand.view(m, K, -1)[1::2, :R]) and torch.equal(o2.view(m, R, -1)[0::2], out.view(m, R, -1)[0::2])


def test_search_player_rebuilds_the_state_the_partner_moved_from():
    import torch

    import hanabi_hip
    from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR
    from hanabi_hip import SearchPlayer, last_move_uid

    m, seed = 16, 7
    team = [RulebasedAgent(PR.piers_rules, seed=11), RulebasedAgent(PR.piers_rules, seed=12)]
    sp = SearchPlayer(team, 0, replicas=2, seed=3, condition=True, oversample=2)
    env = hanabi_hip.HanabiEnv("Hanabi-Full", 2, n_games=m, seed=seed, auto_reset=False, packed=True)
    scratch = hanabi_hip.HanabiEnv("Hanabi-Full", 2, n_games=m, seed=1, auto_reset=False, packed=True)
    act = torch.empty(m, dtype=torch.int32, device="cuda")
    checked = 0
    for t in range(9):
        if t % 2 == 0:
            rows = env.export_state()
            prev, valid = sp._previous(env, rows, t + 1)
            assert bool(valid.any()) == (t >= 2)   # a seat's first move of a game is never conditioned
            if t >= 2:
                ok = valid != 0
                assert torch.equal(ok, ((rows[:, 0] >> 19) & 3) == 0) and int(ok.sum()) > m // 2   # every game still running
                scratch.import_state(prev)
                scratch.step(last_move_uid(env.cfg, rows))
                assert torch.equal(scratch.export_state()[ok], rows[ok])
                assert bool((((prev[:, 0] >> 13) & 7)[ok] == 1).all())
                checked += 1
            sp.eval_moves(env, seed, t + 1, act)
        else:
            team[1].eval_moves(env, seed, t + 1, act)
        env.step(act)
    assert checked == 4
    # another env object, or a call that is not two draws after the remembered one: nothing is usable
    assert not bool(sp._previous(scratch, scratch.export_state(), 11)[1].any())
    assert not bool(sp._previous(env, env.export_state(), 12)[1].any())


def test_search_player_condition_off_is_the_player_as_it_was():
    import torch

    from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR
    from hanabi_hip import Evaluator, SearchPlayer

    team = [RulebasedAgent(PR.piers_rules, seed=30), RulebasedAgent(PR.piers_rules, seed=31)]
    ev = Evaluator("Hanabi-Full", 2, n_games=16, seed=7, record_actions=True)
    old = SearchPlayer(team, 0, replicas=3, seed=2, z=1.0)
    new = SearchPlayer(team, 0, replicas=3, seed=2, z=1.0, condition=False, oversample=4)
    a, b = ev.run([old, team[1]]), ev.run([new, team[1]])
    assert torch.equal(a.scores, b.scores) and torch.equal(a.actions, b.actions) and torch.equal(a.lengths, b.lengths)
    assert (old.moves, old.deviations, old.rollouts) == (new.moves, new.deviations, new.rollouts) and old.deviations > 0
    assert (new.conditioned, new.unconditioned, new.survivors, new.candidates, new.fallbacks) == (0, 0, 0, 0, 0)


def test_search_player_conditioned():
    import torch

    import hanabi_hip
    from hanabi_agents.rule_based import RulebasedAgent, Ruleset, predefined_rules as PR
    from hanabi_hip import Evaluator, SearchPlayer, last_move_uid

    ev = Evaluator("Hanabi-Full", 2, n_games=16, seed=7, record_actions=True)
    # A partner whose rule list never reads the other hand: every candidate survives. [discard_oldest_first] alone is such a list
    # wherever the rule fires; with every information token in store it does not, the agent falls back to a uniform LEGAL move,
    # and which hints are legal does read the other hand. The rule fired exactly where the partner's move is uid 0 (a discard
    # is illegal where it did not): there n_surv == K and nothing falls back; elsewhere the filter may bite.
    blind = [RulebasedAgent(PR.piers_rules, seed=30), RulebasedAgent([Ruleset.discard_oldest_first], seed=31)]
    sp = SearchPlayer(blind, 0, replicas=2, seed=2, condition=True, oversample=3)
    env = hanabi_hip.HanabiEnv("Hanabi-Full", 2, n_games=16, seed=7, auto_reset=False, packed=True)
    act = torch.empty(16, dtype=torch.int32, device="cuda")
    fired_roots = 0
    for t in range(13):
        if t % 2 == 0:
            rows = env.export_state()
            sp.eval_moves(env, 7, t + 1, act)
            if t >= 2:
                res = sp.last_result
                fired = (last_move_uid(env.cfg, rows) == 0) & (res.fallback != 2)
                assert bool((res.n_surv[fired] == 6).all()) and bool((res.fallback[fired] == 0).all())
                assert bool((res.n_surv <= 6).all())
                fired_roots += int(fired.sum())
        else:
            blind[1].eval_moves(env, 7, t + 1, act)
        env.step(act)
    assert fired_roots >= 16
    sp.reset_stats()
    res = ev.run([sp, blind[1]])
    assert sp.conditioned > 0 and sp.survivors <= sp.candidates == 6 * sp.conditioned
    assert sp.conditioned + sp.unconditioned == sp.moves == int(res.moves[0].sum())
    assert sp.unconditioned >= 16   # every game's first move
    # [Piers, Piers], both seats searching with a confirming stage: the filter bites, two runs agree move for move
    team = [RulebasedAgent(PR.piers_rules, seed=30), RulebasedAgent(PR.piers_rules, seed=31)]
    runs = []
    for _ in range(2):
        pair = [SearchPlayer(team, s, replicas=3, seed=2, z=1.0, confirm_replicas=4, condition=True, oversample=4) for s in (0, 1)]
        runs.append((ev.run(pair), pair))
    (ra, pa), (rb, pb) = runs
    assert torch.equal(ra.scores, rb.scores) and torch.equal(ra.actions, rb.actions)
    for s in (0, 1):
        p = pa[s]
        assert p.conditioned + p.unconditioned == p.moves == int(ra.moves[s].sum())
        assert 0 < p.survivors < p.candidates == 12 * p.conditioned
        assert (p.conditioned, p.survivors, p.fallbacks, p.deviations) == (pb[s].conditioned, pb[s].survivors, pb[s].fallbacks,
                                                                          pb[s].deviations)
        p.reset_stats()
        assert (p.conditioned, p.unconditioned, p.survivors, p.candidates, p.fallbacks) == (0, 0, 0, 0, 0)
    with pytest.raises(ValueError, match="2 players"):
        three = [RulebasedAgent(PR.piers_rules, seed=s) for s in range(3)]
        SearchPlayer(three, 0, condition=True)


def test_search_player_conditioned_reproduces_the_recorded_games():
    """Scores, lengths, every action and every counter of the two runs of search_util._conditioned_games equal the file
    tests/golden/gen_search_belief_golden.py wrote: Philox draws and integer sums only, so the games are the same games."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "search_belief_lastmove.json")) as f:
        want = json.load(f)
    got = _conditioned_games()
    assert sorted(got) == sorted(want) == ["both", "seat0"]
    for name, run in want.items():
        assert len(got[name]["players"]) == len(run["players"]) == (1 if name == "seat0" else 2)
        for field in ("scores", "lengths", "actions"):
            assert got[name][field] == run[field], (name, field)
        for s, (p, q) in enumerate(zip(got[name]["players"], run["players"])):
            assert sorted(p) == sorted(q)
            for k in q:
                assert p[k] == q[k], (name, s, k)
            assert q["conditioned"] > 0 and q["survivors"] < q["candidates"]   # (the filter bites in what was recorded)


def test_search_player_conditions_on_a_dqn_partner():
    """Small, bf16, bit-packed observations: the partner's hypothetical moves come through the vectorized path (observe() on the
    scratch env, eval_moves with its own scratch buffers), and so do the searcher's own."""
    import hanabi_hip
    from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR
    from hanabi_hip import Evaluator, SearchPlayer

    shape = hanabi_hip.HanabiEnv("Hanabi-Small", 2, n_games=1, packed=True)
    team = [_dqn(shape, seed=5), RulebasedAgent(PR.piers_rules, seed=15)]
    ev = Evaluator("Hanabi-Small", 2, n_games=8, seed=7)
    for seat in (1, 0):
        sp = SearchPlayer(team, seat, replicas=2, seed=2, condition=True, oversample=2)
        agents = list(team)
        agents[seat] = sp
        res = ev.run(agents)
        assert res.n_games == 8 and sp.moves == int(res.moves[seat].sum())
        assert sp.conditioned + sp.unconditioned == sp.moves and sp.survivors <= sp.candidates == 4 * sp.conditioned
        assert sp.conditioned > 0 or int(res.lengths.max()) <= 2 + seat


def test_session_search_with_a_history_leaves_the_session_untouched(monkeypatch):
    import torch
    from test_search_gpu import _assert_same, _session_state

    import hanabi_hip
    from hanabi_agents.rlax_dqn import ActionSpec, DQNAgent, ObservationSpec, RlaxRainbowParams
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
    before = _session_state(sess)
    res = sess.search(replicas=2, seed=3, history=(prev, 5, 20, sess.env.first_game_id), oversample=2)
    _assert_same(before, _session_state(sess))
    assert res.n_surv.shape == (n,) and res.fallback.shape == (n,) and res.rollouts > 0
    assert bool((res.n_surv <= 4).all()) and bool((res.fallback <= 2).all())
    plain = sess.search(replicas=2, seed=3)
    assert plain.n_surv is None and plain.fallback is None
    _assert_same(before, _session_state(sess))
    with pytest.raises(ValueError, match="previous rows"):
        sess.search(replicas=2, seed=3, history=(prev[:5], 5, 20, 0))
