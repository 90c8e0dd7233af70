"""Belief-sampled rollout search on the GPU (hanabi_hip.search, csrc/belief.hip): the determinize kernel against the numpy
restatement of tests/test_search_cpu.py bit for bit, the reduction against an integer recount, RolloutSearch against a rerun by
hand, and the guarantees of SelfPlaySession.search and SearchPlayer."""
import numpy as np
import pytest
from search_util import _mid_game_env, _team

pytestmark = pytest.mark.gpu


def _ocfg(env):
    from oracle import oracle_py as O

    c = env.cfg
    return O.HbConfig(c.players, c.colors, c.ranks, c.hand_size, c.max_info, c.max_life, 0)


@pytest.mark.parametrize("game,players,m,turns", [("Hanabi-Full", 2, 37, 14), ("Hanabi-Full", 3, 21, 15), ("Hanabi-Full", 5, 70, 17),
                                                  ("Hanabi-Small", 2, 45, 7), ("Hanabi-Very-Small", 2, 33, 5)])
def test_determinize_equals_the_restatement(game, players, m, turns):
    import torch
    from test_search_cpu import determinize_ref

    from hanabi_hip import Determinizer

    env = _mid_game_env(game, players, m, turns)
    rows = env.export_state()
    hinted = rows[:, 10 + players:10 + 3 * players].cpu().numpy().astype(np.uint32)
    assert ((hinted & 0xC00C00) != 0).any(), "no hint has been given in any game"
    det = Determinizer(config=env.cfg)
    ocfg = _ocfg(env)
    rows_np = rows.cpu().numpy().astype(np.uint32)
    some_live = False
    for replicas, seat in ((1, -1), (33, -1), (33, players - 1), (2, 0)):
        out, w = det.sample(rows, seat=seat, replicas=replicas, seed=77, draw=5, first_row_id=1000)
        want, want_w = determinize_ref(ocfg, rows_np, seat, replicas, 77, 5, first_row_id=1000)
        assert np.array_equal(out.cpu().numpy().astype(np.uint32), want)
        assert np.array_equal(w.cpu().numpy(), want_w.astype(np.int64))
        some_live |= bool((w > 0).any())
        if replicas == 33:   # split in two calls (and at a source row that is no multiple of anything)
            k = m // 3
            o1, w1 = det.sample(rows[:k], seat=seat, replicas=replicas, seed=77, draw=5, first_row_id=1000)
            o2, w2 = det.sample(rows[k:], seat=seat, replicas=replicas, seed=77, draw=5, first_row_id=1000 + k * replicas)
            assert torch.equal(torch.cat([o1, o2]), out) and torch.equal(torch.cat([w1, w2]), w)
    assert some_live
    # 64-bit seed, draw and row ids
    big = dict(seed=(5 << 40) + 3, draw=(7 << 33) + 1, first_row_id=(1 << 35) + 9)
    out, w = det.sample(rows, seat=-1, replicas=2, **big)
    want, want_w = determinize_ref(ocfg, rows_np, -1, 2, big["seed"], big["draw"], first_row_id=big["first_row_id"])
    assert np.array_equal(out.cpu().numpy().astype(np.uint32), want) and np.array_equal(w.cpu().numpy(), want_w.astype(np.int64))


def test_determinize_on_crossed_knowledge_and_dead_replicas():
    """Knowledge no play reaches (tests/test_search_cpu.crossed_states): weights differ between replicas and some die."""
    import torch
    from test_search_cpu import crossed_states, determinize_ref

    from hanabi_hip import Determinizer

    states = crossed_states()
    cfg = states[0][0]
    rows_np = np.stack([r for _, r in states]).astype(np.uint32)
    # ... and one whose slot 1 can only be the card slot 0 may take: half of the replicas die
    r = rows_np[0].copy()
    st = (int(r[0]) >> 13) & 7
    c0 = int(r[10 + st]) & 31
    one = (1 << (c0 // 5)) | (1 << (5 + c0 % 5))
    know = (0x3FF) | (one << 12)
    r[10 + 2 + 2 * st], r[10 + 2 + 2 * st + 1] = know & 0xFFFFFFFF, know >> 32
    rows_np = np.concatenate([rows_np, r[None]])
    det = Determinizer("Hanabi-Small", 2)
    out, w = det.sample(torch.as_tensor(rows_np.astype(np.int32)).cuda(), replicas=64, seed=3, draw=9)
    want, want_w = determinize_ref(cfg, rows_np, -1, 64, 3, 9)
    assert np.array_equal(out.cpu().numpy().astype(np.uint32), want) and np.array_equal(w.cpu().numpy(), want_w.astype(np.int64))
    w = w.view(-1, 64)
    assert all(len(torch.unique(w[i][w[i] > 0])) >= 2 for i in range(len(states)))
    assert bool((w[-1] == 0).any()) and bool((w[-1] > 0).any())
    dead = (w.view(-1) == 0).cpu().numpy()
    assert np.array_equal(out.cpu().numpy().astype(np.uint32)[dead], np.repeat(rows_np, 64, 0)[dead])


@pytest.mark.parametrize("game,players,turns", [("Hanabi-Full", 2, 14), ("Hanabi-Full", 5, 17), ("Hanabi-Small", 2, 6)])
def test_the_observer_cannot_tell(game, players, turns):
    import torch

    import hanabi_hip
    from hanabi_hip import Determinizer

    m, R = 50, 6
    src = _mid_game_env(game, players, m, turns)
    rows = src.export_state()
    out, w = Determinizer(config=src.cfg).sample(rows, seat=-1, replicas=R, seed=4, draw=2)
    env = hanabi_hip.HanabiEnv(game, players, n_games=m * R, seed=1, auto_reset=False, packed=True)
    env.import_state(rows.repeat_interleave(R, 0))
    env.observe()
    obs0, legal0 = env.obs_bits.clone(), env.legal.clone()
    env.import_state(out)
    env.observe()
    live = w > 0
    assert int(live.sum()) > m
    assert torch.equal(env.obs_bits[live], obs0[live]) and torch.equal(env.legal[live], legal0[live])
    assert not torch.equal(out[live], rows.repeat_interleave(R, 0)[live])   # (and something did change)


def test_search_reduce_against_integer_recount():
    import torch

    from hanabi_hip.search import search_reduce

    rng = np.random.default_rng(2)
    for m, A, R in ((9, 20, 32), (5, 48, 130), (3, 11, 1)):
        score = rng.integers(0, 26, (m, A, R)).astype(np.int8)
        w = rng.integers(0, 2 ** 32, (m, R), dtype=np.uint64)
        w[rng.random((m, R)) < 0.3] = 0
        legal = (rng.random((m, A)) < 0.6).astype(np.int8)
        legal[0] = 0           # a root without a legal action
        w[1] = 0               # a root without a live replica
        if m > 2:
            score[2] = 7       # ties: the lowest legal uid wins
        value, wsum, n_live, best = search_reduce(torch.as_tensor(score).cuda(), torch.as_tensor(w.astype(np.uint32).view(np.int32)).cuda(),
                                                  torch.as_tensor(legal).cuda())
        value, wsum, n_live, best = (x.cpu().numpy() for x in (value, wsum, n_live, best))
        for i in range(m):
            sw = sum(int(x) for x in w[i])
            top, top_a = None, -1
            for a in range(A):
                if legal[i, a] and sw > 0:
                    num = sum(int(w[i, r]) * int(score[i, a, r]) for r in range(R))
                    want = np.float32(np.float64(num) / np.float64(sw))
                    assert value[i, a] == want and wsum[i, a] == sw and n_live[i, a] == int((w[i] != 0).sum())
                    if top is None or want > top:
                        top, top_a = want, a
                else:
                    assert np.isnan(value[i, a]) and wsum[i, a] == 0 and n_live[i, a] == 0
            assert best[i] == top_a
        assert best[0] == -1 and best[1] == -1
        if m > 2:
            assert best[2] == int(np.argmax(legal[2]))


def _by_hand(src_rows, legal, team, cfg, replicas, seed, draw):
    """RolloutSearch.run by hand: Determinizer, an env of its own, forced first moves, the plain loop, a numpy reduction."""
    import ctypes as C

    import torch

    import hanabi_hip
    from hanabi_hip import Determinizer, _capi as K
    from hanabi_hip.evaluate import max_turns

    m, A, R, P = src_rows.shape[0], legal.shape[1], replicas, cfg.players
    running = ((src_rows[:, 0] >> 19) & 3) == 0
    cp = int(((src_rows[:, 0] >> 13) & 7)[running][0])   # (the seat to move in the games still running)
    det_rows, w = Determinizer(config=cfg).sample(src_rows, seat=cp, replicas=R, seed=seed, draw=draw)
    n = m * A * R
    env = hanabi_hip.HanabiEnv(config=hanabi_hip.HbConfig(cfg.players, cfg.colors, cfg.ranks, cfg.hand_size, cfg.max_info, cfg.max_life, 0),
                               n_games=n, seed=seed, first_game_id=0, packed=True)
    env.import_state(det_rows.view(m, 1, R, -1).expand(m, A, R, det_rows.shape[1]).reshape(n, -1).contiguous())
    lg = legal.cpu().numpy() != 0
    wn = w.cpu().numpy().reshape(m, R)
    forced = np.zeros((m, A, R), np.int32)
    for i in range(m):
        for a in range(A):
            forced[i, a] = a if lg[i, a] else int(np.argmax(lg[i]))
    counted = (lg[:, :, None] & (wn[:, None, :] > 0)).reshape(n)
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
    final = final.reshape(m, A, R)
    value = np.full((m, A), np.nan, np.float32)
    n_live = np.zeros((m, A), np.int32)
    best = np.full(m, -1, np.int32)
    for i in range(m):
        sw = sum(int(x) for x in wn[i])
        top = None
        for a in range(A):
            if lg[i, a] and sw > 0:
                value[i, a] = np.float32(np.float64(sum(int(wn[i, r]) * int(final[i, a, r]) for r in range(R))) / np.float64(sw))
                n_live[i, a] = int((wn[i] > 0).sum())
                if top is None or value[i, a] > top:
                    top, best[i] = value[i, a], a
    return value, n_live, best, int(counted.sum())


@pytest.mark.parametrize("team_name", ["piers_piers", "iggi_flawed", "dqn_piers"])
def test_rollout_search_equals_a_rerun_by_hand(team_name):
    import torch

    from hanabi_hip import RolloutSearch

    m, R = 24, 5
    src = _mid_game_env("Hanabi-Full", 2, m, 8, seed=6)
    src.observe()
    rows, legal = src.export_state(), src.legal.clone()
    assert int((((rows[:, 0] >> 19) & 3) == 0).sum()) > m // 2
    team = _team(team_name, src)
    rs = RolloutSearch("Hanabi-Full", 2, replicas=R, seed=21)
    res = rs.run(rows, legal, team, draw=13)
    value, n_live, best, rollouts = _by_hand(rows, legal, team, src.cfg, R, 21, 13)
    got = res.value.cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(value)) and np.array_equal(got[~np.isnan(got)], value[~np.isnan(value)])
    assert np.array_equal(res.n_live.cpu().numpy(), n_live) and np.array_equal(res.best.cpu().numpy(), best)
    assert res.rollouts == rollouts and rollouts > 0
    if team_name != "dqn_piers":   # (an untrained network bombs out of every game: all of its values are 0)
        assert np.nanmax(got) > np.nanmin(got)
    # determinism: the same (seed, draw) again, then another draw
    again = rs.run(rows, legal, team, draw=13)
    assert torch.equal(again.value.nan_to_num(-1), res.value.nan_to_num(-1)) and torch.equal(again.best, res.best)
    other = rs.run(rows, legal, team, draw=14)
    if team_name != "dqn_piers":
        assert not torch.equal(other.value.nan_to_num(-1), res.value.nan_to_num(-1))
    det = rs.det
    d13, d13b, d14 = (det.sample(rows, seat=-1, replicas=R, seed=21, draw=d)[0] for d in (13, 13, 14))
    assert torch.equal(d13, d13b) and not torch.equal(d13, d14)   # another draw: other replicas
    # nothing of the agents moved
    for a in team:
        assert a._draws == 0


def test_search_refuses_mixed_seats_and_shuffled_envs():
    import hanabi_hip
    from hanabi_hip import RolloutSearch, SearchPlayer

    src = _mid_game_env("Hanabi-Full", 2, 8, 4)
    rows = src.export_state()
    rows[3, 0] ^= 1 << 13   # seat 1 to move in one game
    team = _team("piers_piers", src)
    with pytest.raises(ValueError, match="same current player"):
        RolloutSearch("Hanabi-Full", 2, replicas=2).run(rows, src.legal, team, draw=1)
    with pytest.raises(ValueError, match="one blueprint agent per seat"):
        RolloutSearch("Hanabi-Full", 2, replicas=2).run(src.export_state(), src.legal, team[:1], draw=1)
    shuf = hanabi_hip.HanabiEnv("Hanabi-Full", 2, n_games=8, auto_reset=False, packed=True, color_shuffle=True)
    import torch

    with pytest.raises(ValueError, match="colour-shuffled"):
        SearchPlayer(team, 0, replicas=2).eval_moves(shuf, 1, 1, torch.zeros(8, dtype=torch.int32, device="cuda"))


def _session_state(sess):
    import torch

    torch.cuda.synchronize()
    return sess.checkpoint_state(include_replay=True)


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


def test_session_search_leaves_training_untouched(monkeypatch):
    """Session A trains 20 steps, searches, trains 20 more; session B trains 40 steps: bit-identical (weights, Adam moments,
    replay, sum tree, env rows, draw counters). And the state right before and right after the search is the same."""
    import torch

    import hanabi_hip
    from hanabi_agents.rlax_dqn import ActionSpec, DQNAgent, ObservationSpec, RlaxRainbowParams
    from hanabi_hip.selfplay import SelfPlaySession

    monkeypatch.setenv("HB_ACTOR_FUSED_MIN_ROWS", "0")
    n = 128

    def session():
        torch.manual_seed(0)
        torch.cuda.manual_seed(0)
        flags = hanabi_hip.FLAG_AUTO_RESET | hanabi_hip.FLAG_RESET_START_NEXT
        env = hanabi_hip.HanabiEnv(config=hanabi_hip.make_config("Hanabi-Full", 2, flags), n_games=n, seed=5, packed=True)
        params = RlaxRainbowParams(train_batch_size=128, experience_buffer_size=n * 8, mask_terminal=True, target_update_period=6,
                                   compute_dtype="bfloat16", packed_obs=True, layers=[512], learning_rate=0.01)
        mk = lambda s: DQNAgent(ObservationSpec((n, env.obs_len)), ActionSpec(env.num_actions), params._replace(seed=s), device="cuda")
        return SelfPlaySession(env, [mk(1), mk(2)])

    a = session()
    a.run(20)
    before = _session_state(a)
    res = a.search(replicas=4, seed=3)
    _assert_same(before, _session_state(a))
    assert res.value.shape == (n, 20) and res.rollouts > 0
    legal = a.env.legal != 0
    assert bool((torch.isnan(res.value) == ~legal).all())
    assert bool((res.best >= 0).all()) and bool(legal.gather(1, res.best.long().view(-1, 1)).all())
    a.run(20)
    b = session()
    b.run(40)
    _assert_same(_session_state(a), _session_state(b))
    shuffled = hanabi_hip.HanabiEnv("Hanabi-Full", 2, n_games=n, packed=True, color_shuffle=True)
    with pytest.raises(ValueError, match="colour-shuffled"):
        SelfPlaySession(shuffled, a.agents).search()


@pytest.mark.parametrize("players", [2, 3])
def test_search_player_in_an_evaluation(players):
    import math

    import torch

    from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR
    from hanabi_hip import Evaluator, SearchPlayer

    team = [RulebasedAgent(PR.piers_rules, seed=30 + s) for s in range(players)]
    ev = Evaluator("Hanabi-Full", players, n_games=16, seed=7, record_actions=True)
    base = ev.run(team)
    # never deviating: the evaluation of the blueprint itself
    sp = SearchPlayer(team, 0, replicas=3, threshold=math.inf, seed=2)
    same = ev.run([sp] + team[1:])
    assert torch.equal(same.scores, base.scores) and torch.equal(same.lengths, base.lengths) and torch.equal(same.actions, base.actions)
    assert sp.deviations == 0 and sp.moves == int(base.moves[0].sum())
    # SPARTA's rule: completes with no illegal move (Evaluator.run raises on one)
    sp = SearchPlayer(team, 0, replicas=3, threshold=0.0, seed=2)
    res = ev.run([sp] + team[1:])
    assert res.n_games == 16 and int(res.histogram.sum()) == 16
    assert sp.moves == int(res.moves[0].sum()) and 0 < sp.deviations <= sp.moves
    assert sp.dead_replicas == 0 and sp.replicas_drawn == 3 * sp.moves
    again = SearchPlayer(team, 0, replicas=3, threshold=0.0, seed=2)
    res2 = ev.run([again] + team[1:])
    assert torch.equal(res2.scores, res.scores) and torch.equal(res2.actions, res.actions)
