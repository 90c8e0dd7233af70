"""Screen-then-confirm search on the GPU (hanabi_hip.search, csrc/belief.hip): hb_search_layout against the torch expressions
RolloutSearch.run used to build its games with and against a numpy gather, hb_search_compare against the restatement of
tests/test_search_confirm_cpu.py, RolloutSearch.confirm against a rerun by hand, and SearchPlayer's z / confirm_replicas."""
import math

import numpy as np
import pytest
from search_util import _mid_game_env, _team, _u32

pytestmark = pytest.mark.gpu


def _roots(game, players, turns, n=37, seed=3):
    """(env, state rows [n, SW], legal [n, A]) of n games `turns` random legal moves in."""
    env = _mid_game_env(game, players, n, turns, seed=seed)
    env.observe()
    return env, env.export_state(), env.legal.clone()


@pytest.mark.parametrize("game,players,turns", [("Hanabi-Full", 2, 14), ("Hanabi-Full", 5, 17), ("Hanabi-Small", 2, 7)])
def test_layout_equals_the_torch_expressions(game, players, turns):
    """C = A with the legal mask as candidates: what RolloutSearch.run built with torch before the kernel existed."""
    import torch

    from hanabi_hip import Determinizer
    from hanabi_hip.search import search_layout

    env, rows_all, legal_all = _roots(game, players, turns)
    A, SW = env.num_actions, env.state_words
    assert SW == (48 if players == 5 else 32)
    det = Determinizer(config=env.cfg)
    uid = torch.arange(A, dtype=torch.int32, device="cuda").view(1, A, 1)
    for m in (1, 5, 37):
        for R in (1, 33):
            src, lg = rows_all[:m], legal_all[:m]
            det_rows, w = det.sample(src, seat=-1, replicas=R, seed=5, draw=2, out=(
                torch.empty((m * R, SW), dtype=torch.int32, device="cuda"), torch.empty(m * R, dtype=torch.int32, device="cuda")))
            w[(m * R) // 2] = 0   # a dead replica
            n = m * A * R
            lgb = lg != 0
            want_rows = det_rows.view(m, 1, R, SW).expand(m, A, R, SW).reshape(n, SW)
            played = lgb.view(m, A, 1) & (w.view(m, 1, R) != 0)
            first_legal = lgb.int().argmax(1).int().view(m, 1, 1)
            want_forced = torch.where(lgb.view(m, A, 1), uid, first_legal).expand(m, A, R).reshape(n)
            want_done = torch.where(played, 0, 0x80).to(torch.uint8).reshape(n)
            cand = torch.where(lgb, uid.view(1, A), -1).int().contiguous()
            got_rows, forced, done, n_played = search_layout(env.cfg, det_rows, w, cand, first_legal.view(m).contiguous(), R)
            assert torch.equal(got_rows, want_rows) and torch.equal(forced, want_forced) and torch.equal(done, want_done)
            assert int(n_played.sum()) == int(played.sum())
            assert torch.equal(n_played.long(), played.view(m, -1).sum(1))


def layout_by_gather(det_rows, weights, cand, filler, R):
    """hb_search_layout as a direct numpy gather (also tests/test_determinize_deep_gpu.py's): det_rows [m * R, SW], weights
    [m * R] uint32, cand [m, C] int32, filler [m] int32 -> (rows [m * C * R, SW], forced [m * C * R], done [m * C * R] uint8,
    n_played [m])."""
    m, Cn = cand.shape
    i, c, r = np.meshgrid(np.arange(m), np.arange(Cn), np.arange(R), indexing="ij")
    played = (cand[i, c] >= 0) & (weights[i * R + r] != 0)
    return (det_rows[(i * R + r).reshape(-1)], np.where(cand[i, c] >= 0, cand[i, c], filler[i]).reshape(-1),
            np.where(played, 0, 0x80).astype(np.uint8).reshape(-1), played.reshape(m, -1).sum(1))


@pytest.mark.parametrize("game,players,turns", [("Hanabi-Full", 2, 14), ("Hanabi-Full", 5, 17), ("Hanabi-Small", 2, 7)])
def test_layout_of_short_candidate_lists(game, players, turns):
    """C = 1 and 2, hand-built lists, against a direct numpy gather."""
    import torch

    from hanabi_hip import Determinizer
    from hanabi_hip.search import search_layout

    env, rows_all, _ = _roots(game, players, turns)
    A, SW = env.num_actions, env.state_words
    rows_all = rows_all.clone()
    rows_all[2, 0] |= 1 << 19   # a finished root: every replica of it weighs nothing
    det = Determinizer(config=env.cfg)
    rng = np.random.default_rng(7)
    for m in (5, 37):
        for R in (1, 33):
            for Cn in (1, 2):
                det_rows, w = det.sample(rows_all[:m], seat=-1, replicas=R, seed=5, draw=2, out=(
                    torch.empty((m * R, SW), dtype=torch.int32, device="cuda"), torch.empty(m * R, dtype=torch.int32, device="cuda")))
                w[R * (m - 1)] = 0   # a dead replica of the last root
                cand = rng.integers(0, A, (m, Cn)).astype(np.int32)
                cand[0] = -1          # a row of all -1
                cand[1, 0] = -1       # -1 in slot 0 only
                filler = rng.integers(0, A, m).astype(np.int32)
                rows, forced, done, n_played = search_layout(env.cfg, det_rows, w, torch.as_tensor(cand).cuda(),
                                                             torch.as_tensor(filler).cuda(), R)
                dn, wn = det_rows.cpu().numpy(), _u32(w)
                assert (wn.reshape(m, R)[2] == 0).all() and wn[R * (m - 1)] == 0 and (wn > 0).any()
                want = layout_by_gather(dn, wn, cand, filler, R)
                for got, exp in zip((rows, forced, done, n_played), want):
                    assert np.array_equal(got.cpu().numpy(), exp)
                assert n_played[0] == 0 and n_played[2] == 0


@pytest.mark.parametrize("kind", ["constant", "random", "zero_roots"])
def test_compare_equals_the_restatement(kind):
    """diff exactly; se within 4 (R + 8) 2^-53 relative: a sum of R non-negative doubles plus the closing operations."""
    import torch
    from test_search_confirm_cpu import compare_ref

    from hanabi_hip.search import search_compare

    rng = np.random.default_rng({"constant": 1, "random": 2, "zero_roots": 3}[kind])
    finite = infinite = nans = 0
    for m in (1, 5, 37):
        for Cn in (1, 2, 20, 48):
            for R in (1, 2, 33, 65, 130):
                scores = rng.integers(0, 26, (m, Cn, R)).astype(np.int8)
                if kind == "constant":
                    w = np.repeat(rng.integers(1, 5 * 10 ** 8, (m, 1), dtype=np.uint64), R, 1)
                else:
                    w = rng.integers(1, 5 * 10 ** 8 + 1, (m, R), dtype=np.uint64)
                    w[rng.random((m, R)) < 0.3] = 0
                if kind == "zero_roots":
                    w[::2] = 0             # roots without a live replica
                    if m > 1:
                        w[1, 1:] = 0       # and one with at most one
                cand = rng.integers(0, 20, (m, Cn)).astype(np.int32)
                cand[rng.random((m, Cn)) < 0.2] = -1
                base = rng.integers(-1, Cn, m).astype(np.int32)
                diff, se, n_pair = search_compare(torch.as_tensor(scores).cuda(), torch.as_tensor(w.astype(np.uint32).view(np.int32)).cuda(),
                                                  torch.as_tensor(cand).cuda(), torch.as_tensor(base).cuda())
                diff, se, n_pair = diff.cpu().numpy(), se.cpu().numpy(), n_pair.cpu().numpy()
                want_diff, want_se, want_n = compare_ref(scores, w, cand, base)
                assert np.array_equal(n_pair, want_n)
                assert np.array_equal(np.isnan(diff), np.isnan(want_diff)) and np.array_equal(np.isnan(se), np.isnan(want_se))
                ok = ~np.isnan(want_diff)
                assert np.array_equal(diff[ok], want_diff[ok])
                inf = np.isinf(want_se)
                assert np.array_equal(np.isinf(se), inf)
                fin = ok & ~inf
                assert (np.abs(se[fin] - want_se[fin]) <= 4 * (R + 8) * 2.0 ** -53 * want_se[fin]).all()
                finite, infinite, nans = finite + int((fin & (want_se > 0)).sum()), infinite + int(inf.sum()), nans + int((~ok).sum())
    assert nans > 0 and (finite > 0 or kind == "zero_roots") and (infinite > 0 or kind == "constant")


def _confirm_by_hand(rows, legal, team, cfg, R0, R1, seed, draw, baseline, challenger, first_game_id=0):
    """RolloutSearch.confirm by hand: the determinizer keyed behind the first stage's rows, an [m, 2, R1] env of its own keyed
    behind the first stage's games, forced first moves, the plain loop, then the restatements."""
    import torch
    from test_search_confirm_cpu import compare_ref

    import hanabi_hip
    from hanabi_hip import Determinizer
    from hanabi_hip.evaluate import max_turns

    m, A, P = rows.shape[0], legal.shape[1], cfg.players
    running = (((rows[:, 0] >> 19) & 3) == 0).cpu().numpy()
    cp = int(((rows[:, 0] >> 13) & 7).cpu().numpy()[running][0])
    det_rows, w = Determinizer(config=cfg).sample(rows, seat=cp, replicas=R1, seed=seed, draw=draw, first_row_id=m * R0)
    n = m * 2 * R1
    env = hanabi_hip.HanabiEnv(config=hanabi_hip.HbConfig(cfg.players, cfg.colors, cfg.ranks, cfg.hand_size, cfg.max_info, cfg.max_life, 0),
                               n_games=n, seed=seed, first_game_id=first_game_id + m * A * R0, packed=True)
    env.import_state(det_rows.view(m, 1, R1, -1).expand(m, 2, R1, det_rows.shape[1]).reshape(n, -1).contiguous())
    lg = legal.cpu().numpy() != 0
    wn = w.cpu().numpy().reshape(m, R1)
    cand = np.full((m, 2), -1, np.int32)
    for i in range(m):
        b, c = int(baseline[i]), int(challenger[i])
        if running[i] and c >= 0 and c != b and 0 <= b < A and c < A and lg[i, b] and lg[i, c]:
            cand[i] = (b, c)
    forced = np.zeros((m, 2, R1), np.int32)
    for i in range(m):
        for c in range(2):
            forced[i, c] = cand[i, c] if cand[i, c] >= 0 else int(np.argmax(lg[i]))
    counted = ((cand >= 0)[:, :, None] & (wn[:, None, :] > 0)).reshape(n)
    final = np.zeros(n, np.int64)
    done = ~counted
    act = torch.as_tensor(forced.reshape(n)).cuda()
    scratch = {}
    for t in range(max_turns(cfg)):
        if t > 0:
            agent = team[(cp + t) % P]
            if agent.requires_vectorized_observation():
                agent.eval_moves((env, (env.net_obs, env.legal)), seed, t + 1, act, scratch=scratch)
            else:
                agent.eval_moves(env, seed, t + 1, act)
        env.step(act)
        term, score = env.terminal.cpu().numpy() != 0, env.score.cpu().numpy()
        ended = ~done & term
        final[ended] = score[ended]
        done |= ended
        if done.all():
            break
    assert done.all() and env.illegal_count() == 0
    final = final.reshape(m, 2, R1)
    value = np.full((m, 2), np.nan, np.float32)
    for i in range(m):
        sw = sum(int(x) for x in wn[i])
        for c in range(2):
            if cand[i, c] >= 0 and sw > 0:
                value[i, c] = np.float32(np.float64(sum(int(wn[i, r]) * int(final[i, c, r]) for r in range(R1))) / np.float64(sw))
    diff, se, n_pair = compare_ref(final, wn, cand, np.zeros(m, np.int32))
    return cand, value, diff, se, n_pair, int(counted.sum()), det_rows


def _same_or_nan(got, want):
    return np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)])


@pytest.mark.parametrize("game,team_name,turns", [("Hanabi-Full", "piers_piers", 8), ("Hanabi-Small", "dqn_piers", 4)])
def test_confirm_equals_a_rerun_by_hand(game, team_name, turns):
    import torch

    from hanabi_hip import RolloutSearch

    m, R0, R1 = 24, 5, 9
    src, rows, legal = _roots(game, 2, turns, n=m, seed=6)
    A = src.num_actions
    running = ((rows[:, 0] >> 19) & 3) == 0
    assert int(running.sum()) > m // 2
    team = _team(team_name, src)
    cp = turns % 2
    baseline = torch.zeros(m, dtype=torch.int32, device="cuda")
    if team[cp].requires_vectorized_observation():
        team[cp].eval_moves((src, (src.net_obs, src.legal)), 21, 13, baseline, scratch={})
    else:
        team[cp].eval_moves(src, 21, 13, baseline)
    rs = RolloutSearch(game, 2, replicas=R0, seed=21, first_game_id=1000)
    first = rs.run(rows, legal, team, draw=13, baseline=baseline)
    challenger = torch.where(running & (first.best != baseline), first.best, -1).int()
    some = torch.nonzero(running & (challenger >= 0) & ((legal != 0).sum(1) < A)).view(-1)
    bad = int(some[-1])   # one root's challenger replaced by a move that is illegal there
    challenger[bad] = int(torch.nonzero(legal[bad] == 0)[0])
    res = rs.confirm(rows, legal, team, 13, baseline, challenger, R1)
    cand, value, diff, se, n_pair, rollouts, det_rows = _confirm_by_hand(rows, legal, team, src.cfg, R0, R1, 21, 13, baseline.cpu().numpy(),
                                                                        challenger.cpu().numpy(), first_game_id=1000)
    with_challenger, without = int((cand[:, 1] >= 0).sum()), int((cand[:, 1] < 0).sum())
    assert with_challenger > 0 and without > 0 and (cand[bad] == -1).all()
    assert bool(((cand[:, 1] != cand[:, 0]) | (cand[:, 1] < 0)).all())
    assert np.array_equal(res.cand.cpu().numpy(), cand)
    assert _same_or_nan(res.value.cpu().numpy(), value)
    got_diff, got_se = res.diff.cpu().numpy(), res.se.cpu().numpy()
    assert _same_or_nan(got_diff, diff)
    assert np.array_equal(np.isnan(got_se), np.isnan(se))
    fin = ~np.isnan(se)
    assert (np.abs(got_se[fin] - se[fin]) <= 4 * (R1 + 8) * 2.0 ** -53 * se[fin]).all()
    assert np.array_equal(res.n_pair.cpu().numpy(), n_pair) and res.rollouts == rollouts == 2 * R1 * with_challenger
    assert (n_pair[cand[:, 1] >= 0] == R1).all()
    # the best slot and its uid
    best, uid = res.best.cpu().numpy(), res.best_uid.cpu().numpy()
    for i in range(m):
        if cand[i, 1] < 0:
            assert best[i] == -1 and uid[i] == -1
        else:
            assert best[i] == (1 if value[i, 1] > value[i, 0] else 0) and uid[i] == cand[i, best[i]]
    # stage 1's paired numbers agree with its values: diff = value[a] - value[baseline] up to the f32 rounding of the values
    v = first.value.double()
    vb = v.gather(1, baseline.long().clamp(0, A - 1).view(-1, 1))
    both = ~torch.isnan(first.diff) & ~torch.isnan(v - vb)
    assert bool(both.any()) and float((first.diff - (v - vb))[both].abs().max()) < 1e-5
    for a in team:
        assert a._draws == 0


def test_confirm_draws_fresh_replicas_and_is_deterministic():
    import torch

    from hanabi_hip import Determinizer, RolloutSearch

    m, R = 16, 6
    src, rows, legal = _roots("Hanabi-Full", 2, 8, n=m, seed=6)
    team = _team("piers_piers", src)
    baseline = torch.zeros(m, dtype=torch.int32, device="cuda")
    team[0].eval_moves(src, 4, 3, baseline)
    rs = RolloutSearch("Hanabi-Full", 2, replicas=R, seed=4)
    first = rs.run(rows, legal, team, draw=3)
    challenger = torch.where(first.best != baseline, first.best, -1).int()
    res = rs.confirm(rows, legal, team, 3, baseline, challenger, R)
    assert res.rollouts > 0
    rows1, rows2 = rs._sized[(m, 20, R)]["det_rows"].view(m, R, -1), rs._sized[(m, 2, R)]["det_rows"].view(m, R, -1)
    running = ((rows[:, 0] >> 19) & 3) == 0
    for i in torch.nonzero(running).view(-1).tolist():   # the same root, the same replica index: another state
        assert not torch.equal(rows1[i], rows2[i])
    det = Determinizer("Hanabi-Full", 2)
    seat = int(((rows[:, 0] >> 13) & 7)[running][0])
    assert torch.equal(rows1.reshape(m * R, -1), det.sample(rows, seat=seat, replicas=R, seed=4, draw=3, first_row_id=0)[0])
    assert torch.equal(rows2.reshape(m * R, -1), det.sample(rows, seat=seat, replicas=R, seed=4, draw=3, first_row_id=m * R)[0])
    assert rs._sized[(m, 20, R)]["env"].first_game_id == 0 and rs._sized[(m, 2, R)]["env"].first_game_id == m * 20 * R
    again = rs.confirm(rows, legal, team, 3, baseline, challenger, R)
    for x, y in ((res.value, again.value), (res.diff, again.diff), (res.se, again.se)):
        assert torch.equal(x.nan_to_num(-77.0), y.nan_to_num(-77.0))
    assert torch.equal(res.n_pair, again.n_pair) and torch.equal(res.best, again.best) and res.rollouts == again.rollouts
    # and the first stage's env and buffers survived the second
    assert torch.equal(rs.run(rows, legal, team, draw=3).value.nan_to_num(-1), first.value.nan_to_num(-1))


@pytest.mark.parametrize("game,players,m,R,turns", [("Hanabi-Small", 2, 5, 3, 4), ("Hanabi-Full", 5, 3, 2, 7)])
def test_run_is_run_candidates_over_the_legal_actions(game, players, m, R, turns):
    """run() against run_candidates() with every legal action in the slot of its uid and the root's lowest legal uid as the
    filler, on a second search with the same seed: the same numbers bit for bit, a finished root among the roots."""
    import torch

    from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR
    from hanabi_hip import RolloutSearch

    src, rows, legal = _roots(game, players, turns, n=m, seed=6)
    A = src.num_actions
    rows = rows.clone()
    rows[1, 0] |= 1 << 19   # a finished root (random play may have ended others): it plays nothing
    live = ((rows[:, 0] >> 19) & 3) == 0
    assert bool(live.any()) and not bool(live[1])
    team = [RulebasedAgent(PR.piers_rules, seed=40 + s) for s in range(players)]
    lgb = legal != 0
    uid = torch.arange(A, dtype=torch.int32, device="cuda").view(1, A)
    first_legal = lgb.int().argmax(1).int()
    b = (A - 1 - lgb.flip(1).int().argmax(1)).int()   # the baseline: each root's highest legal uid
    one = RolloutSearch(game, players, replicas=R, seed=21).run(rows, legal, team, 13, baseline=b)
    two = RolloutSearch(game, players, replicas=R, seed=21).run_candidates(rows, torch.where(lgb, uid, -1), first_legal, team, 13,
                                                                           base_slot=b)
    assert one.cand is None and one.best_uid is None and torch.equal(two.best_uid, two.best)
    for name in ("value", "wsum", "n_live", "best", "diff", "se", "n_pair"):
        assert torch.equal(getattr(one, name).nan_to_num(-77.0), getattr(two, name).nan_to_num(-77.0)), name
    assert (one.rollouts, one.turns, one.dead) == (two.rollouts, two.turns, two.dead)
    assert one.rollouts == R * int(lgb[live].sum()) and one.value.shape == (m, A)   # (no replica dies in a state reached by play)
    assert bool(torch.isnan(one.value[~live]).all()) and bool((one.best[~live] == -1).all()) and bool((one.best[live] >= 0).all())


def _small_eval():
    from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR
    from hanabi_hip import Evaluator

    team = [RulebasedAgent(PR.piers_rules, seed=30), RulebasedAgent(PR.piers_rules, seed=31)]
    return team, Evaluator("Hanabi-Small", 2, n_games=64, seed=7, record_actions=True)


def _same_result(x, y):
    import torch

    return torch.equal(x.scores, y.scores) and torch.equal(x.lengths, y.lengths) and torch.equal(x.actions, y.actions)


def _counters(sp):
    return (sp.moves, sp.deviations, sp.dead_replicas, sp.replicas_drawn, sp.searches, sp.confirmed, sp.rejected, sp.rollouts)


def test_search_player_defaults_are_the_old_rule():
    from hanabi_hip import SearchPlayer

    team, ev = _small_eval()
    old = SearchPlayer(team, 0, replicas=4, threshold=0.0, seed=2)
    res_old = ev.run([old, team[1]])
    new = SearchPlayer(team, 0, replicas=4, threshold=0.0, seed=2, z=None, confirm_replicas=0)
    res_new = ev.run([new, team[1]])
    assert _same_result(res_old, res_new) and _counters(old) == _counters(new)
    assert old.deviations > 0 and old.confirmed == 0 and old.rejected == 0 and old.rollouts > 0


def test_search_player_with_an_infinite_z_is_the_blueprint():
    from hanabi_hip import SearchPlayer

    team, ev = _small_eval()
    base = ev.run(team)
    for confirm in (0, 8):
        sp = SearchPlayer(team, 0, replicas=4, threshold=0.0, seed=2, z=math.inf, confirm_replicas=confirm)
        assert _same_result(ev.run([sp, team[1]]), base)
        assert sp.deviations == 0 and sp.moves == int(base.moves[0].sum())
        assert sp.rejected == sp.confirmed and (sp.confirmed > 0) == (confirm > 0)


def test_search_player_screen_then_confirm(monkeypatch):
    from hanabi_hip import RolloutSearch, SearchPlayer

    played = []
    for name in ("run", "confirm"):
        def counting(self, *a, _f=getattr(RolloutSearch, name), **k):
            res = _f(self, *a, **k)
            played.append(res.rollouts)
            return res
        monkeypatch.setattr(RolloutSearch, name, counting)
    team, ev = _small_eval()
    runs = []
    for _ in range(2):
        del played[:]
        sp = SearchPlayer(team, 0, replicas=4, threshold=0.0, seed=2, z=2, confirm_replicas=16)
        runs.append((ev.run([sp, team[1]]), _counters(sp)))
        assert sp.rollouts == sum(played) and sp.rollouts > 0
        assert sp.confirmed >= sp.rejected >= 0 and sp.confirmed > 0
        assert sp.deviations == sp.confirmed - sp.rejected and sp.deviations <= sp.moves
    assert _same_result(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]
    # a single stage with z: nothing goes to a second stage
    del played[:]
    single = SearchPlayer(team, 0, replicas=4, threshold=0.0, seed=2, z=2)
    ev.run([single, team[1]])
    assert single.confirmed == 0 and single.rejected == 0 and 0 <= single.deviations <= single.moves
    assert single.rollouts == sum(played) and len(played) == single.searches


def test_the_new_paths_leave_a_session_untouched(monkeypatch):
    import torch
    from test_search_gpu import _assert_same, _session_state

    import hanabi_hip
    from hanabi_agents.rlax_dqn import ActionSpec, DQNAgent, ObservationSpec, RlaxRainbowParams
    from hanabi_hip import RolloutSearch, SearchPlayer
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
    sess.run(20)
    sess.flush()
    before = _session_state(sess)
    rows, legal = env.export_state(), env.legal.clone()
    rs = RolloutSearch(config=env.cfg, replicas=2, seed=3)
    baseline = (19 - legal.flip(1).int().argmax(1)).int()   # each root's highest legal uid (an untrained team's best is the lowest)
    first = rs.run(rows, legal, sess.agents, draw=7, baseline=baseline)
    assert first.diff is not None and first.se.shape == (n, 20)
    res = rs.confirm(rows, legal, sess.agents, 7, baseline, first.best, 4)
    assert res.rollouts > 0 and res.diff.shape == (n, 2)
    sp = SearchPlayer(sess.agents, int((rows[0, 0] >> 13) & 7), replicas=2, seed=3, z=1, confirm_replicas=4)
    out = torch.zeros(n, dtype=torch.int32, device="cuda")
    sp.eval_moves((env, (env.net_obs, env.legal)), 1, 7, out, scratch={})
    assert sp.moves > 0 and sp.rollouts > 0
    _assert_same(before, _session_state(sess))
