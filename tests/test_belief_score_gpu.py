"""Scoring a belief against the true hand on the GPU (hanabi_hip.search, csrc/belief.hip): hb_belief_score against the numpy
restatement hanabi_hip.belief_score_ref bit for bit (tests/test_belief_score_cpu.py holds the restatement to a brute-force tally,
an independent card count and the exact enumeration), the V0 belief against the prior on fresh deals, and the switch in
SearchPlayer and OffBeliefSession, which must change nothing but the figures it adds."""
import math

import numpy as np
import pytest
from search_util import _mid_game_env, _u32

pytestmark = pytest.mark.gpu

GUARD = 16
FILL = {"int8": 0x5A, "int32": 0x5A5A5A5A, "int64": 0x5A5A5A5A5A5A5A5A}


def _guarded(shape, dtype):
    """(buffer, view): a contiguous tensor of `shape` with GUARD sentinel elements before and after it."""
    import torch

    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), FILL[str(dtype).split(".")[1]], dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(shape)


_ROWS = {}


def _late_rows(game, players):
    """Rows of the open-handed driver of tests/deep_play.py (the oracle's env) from the turn a deck runs out: 12 running rows in
    which the seat to act or the last seat holds a short hand (few games get there: the ones there are, repeated) and 12 finished
    ones, alternating."""
    from deep_play import open_hand_moves
    from oracle import oracle_py as O

    cfg = O.make_config(game, players, 0)
    env = O.OracleEnv(cfg, 48, seed=9)
    legal, rng, late = env.observe()["legal"], np.random.default_rng(4), []
    for t in range(76):
        rows = np.asarray(env.export_state()).astype(np.uint32)
        if (rows[:, 0] & 63).min() == 0:
            late.append(rows.copy())
        legal = env.step(open_hand_moves(cfg, rows, legal, rng, 0.05))["legal"]
    late = np.concatenate(late)
    run = ((late[:, 0] >> 19) & 3) == 0
    sizes = np.stack([(late[:, 1] >> (15 + 3 * p)) & 7 for p in range(players)], 1)
    short = run & ((sizes[np.arange(len(late)), (late[:, 0] >> 13) & 7] < cfg.hand_size) | (sizes[:, players - 1] < cfg.hand_size))
    assert short.sum() >= 4 and (~run).sum() >= 12
    few = late[short][:12]
    return np.stack([x for pair in zip(few[np.arange(12) % len(few)], late[~run][:12]) for x in pair])


def _true_rows(game, players):
    """State rows [72, SW] uint32 in a fixed order: a running row a few random moves into a game, a late one with a short hand and a
    finished one, then the rest of _late_rows and more rows of the first kind (some of them lost already) in turn."""
    if (game, players) not in _ROWS:
        mid = _u32(_mid_game_env(game, players, 48, turns=14 if game == "Hanabi-Full" else 4).export_state())
        mid = mid[np.argsort(((mid[:, 0] >> 19) & 3) != 0, kind="stable")]   # (a running row first: m = 1 scores something)
        assert ((mid[0, 0] >> 19) & 3) == 0
        late = _late_rows(game, players)
        mixed = [mid[0], late[0], late[1]] + [x for pair in zip(late[2:], mid[1:23]) for x in pair] + list(mid[23:])
        _ROWS[(game, players)] = np.stack(mixed)
    return _ROWS[(game, players)]


@pytest.mark.parametrize("game,players", [("Hanabi-Full", 2), ("Hanabi-Small", 2), ("Hanabi-Full", 5)])
@pytest.mark.parametrize("m", [1, 3, 4, 5, 65])
def test_kernel_equals_the_restatement(game, players, m):
    """R in {1, 63, 64, 65, 130} x seat in {-1, the last seat} x counts on and off per shape: replicas from Determinizer.sample
    with a third of the weights zeroed and a few hand words overwritten by random 5-bit fields (31 and ids >= NC among them);
    every output between sentinels, compared with the restatement bit for bit."""
    import torch

    import hanabi_hip
    from hanabi_hip import Determinizer, belief_score, belief_score_ref

    cfg = hanabi_hip.make_config(game, players)
    H, NC = cfg.hand_size, cfg.colors * cfg.ranks
    pool = _true_rows(game, players)
    true = pool[np.arange(m) % len(pool)]
    SW = true.shape[1]
    assert SW == (48 if players == 5 else 32)
    det_of = Determinizer(config=cfg)
    rows_dev = torch.as_tensor(true.view(np.int32)).cuda()
    seen = dict.fromkeys(("short", "finished", "junk", "dead", "joint", "miss"), 0)
    for R in (1, 63, 64, 65, 130):
        for seat in (-1, players - 1):
            rng = np.random.default_rng((m * 131 + R) * 7 + seat + 1)
            det, w = det_of.sample(rows_dev, seat=seat, replicas=R, seed=3, draw=R, out=(
                torch.empty((m * R, SW), dtype=torch.int32, device="cuda"), torch.empty(m * R, dtype=torch.int32, device="cuda")))
            det, w = _u32(det).copy(), _u32(w).copy()
            w[rng.random(m * R) < 1 / 3] = 0
            for o in rng.choice(m * R, size=max(1, m * R // 8), replace=False):   # random 5-bit fields in some slot of some seat's hand
                s, word = int(rng.integers(0, 5)), 10 + int(rng.integers(0, players))
                det[o, word] = (int(det[o, word]) & ~(31 << (5 * s))) | (int(rng.choice([31, NC, 30, rng.integers(0, 32)])) << (5 * s))
            want = belief_score_ref(cfg, true, det, w, seat, R)
            det_dev, w_dev = torch.as_tensor(det.view(np.int32)).cuda(), torch.as_tensor(w.view(np.int32)).cuda()
            for counts in (True, False):
                shapes = [((m, H), torch.int8), ((m, H), torch.int64), ((m,), torch.int64), ((m,), torch.int64), ((m,), torch.int32),
                          ((m, H, NC), torch.int8)] + ([((m, H, NC), torch.int64)] if counts else [])
                bufs, out = zip(*(_guarded(s, dt) for s, dt in shapes))
                got = belief_score(cfg, rows_dev, det_dev, w_dev, seat, R, counts=counts, out=out)
                torch.cuda.synchronize()
                for name in ("truth", "hit", "joint", "wsum", "n_live", "prior") + (("counts",) if counts else ()):
                    g = getattr(got, name).cpu().numpy()
                    assert g.dtype == want[name].dtype and np.array_equal(g, want[name]), (name, R, seat, counts)
                assert counts or got.counts is None
                for buf, (_, dt) in zip(bufs, shapes):   # the sentinels on both sides
                    fill = FILL[str(dt).split(".")[1]]
                    assert bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all()), (R, seat, counts)
            n_slots = (want["truth"] >= 0).sum(1)
            seen["short"] += int(((n_slots > 0) & (n_slots < H)).sum())
            seen["finished"] += int((n_slots == 0).sum())
            seen["junk"] += int(((want["counts"].sum(2) < want["wsum"][:, None]) & (want["truth"] >= 0)).sum())
            seen["dead"] += int(((want["n_live"] < R) & (n_slots > 0)).sum())
            seen["joint"] += int((want["joint"] > 0).sum())
            seen["miss"] += int(((want["hit"] == 0) & (want["truth"] >= 0) & (want["wsum"][:, None] > 0)).sum())
    assert seen["junk"] and seen["dead"] and seen["joint"] and seen["miss"]
    assert m < 3 or (seen["short"] and seen["finished"])


def test_fresh_deals_give_the_prior():
    """At turn 0 nobody has been told anything: the V0 marginal of a slot IS the card count. 4096 replicas of 64 fresh deals of
    Full, 2 players (constant weights: uniform draws): hit / wsum within 6 binomial standard errors of prior[truth] / sum prior."""
    import torch

    import hanabi_hip
    from hanabi_hip import Determinizer, belief_score

    m, R = 64, 4096
    env = hanabi_hip.HanabiEnv("Hanabi-Full", 2, n_games=m, seed=5, auto_reset=False, packed=True)
    rows = env.export_state()
    det, w = Determinizer(config=env.cfg).sample(rows, seat=-1, replicas=R, seed=9, draw=0, out=(
        torch.empty((m * R, rows.shape[1]), dtype=torch.int32, device="cuda"), torch.empty(m * R, dtype=torch.int32, device="cuda")))
    b = belief_score(env.cfg, rows, det, w, -1, R, counts=True)
    assert bool((b.n_live == R).all()) and bool(b.scored.all()) and bool((b.truth >= 0).all())
    wsum = b.wsum.double().view(m, 1)
    assert bool((b.wsum == R * (w.view(m, R)[:, 0].long() & 0xFFFFFFFF)).all())   # one weight per root
    prior = b.prior.double()
    assert bool((prior.sum(2) == 45).all())                                      # 5 own cards + 40 to draw, nothing excluded
    p = prior.gather(2, b.truth.long().unsqueeze(2)).squeeze(2) / 45
    assert bool((p > 0).all())
    est = b.hit.double() / wsum
    print("largest deviation in standard errors:", float(((est - p).abs() / (p * (1 - p) / R).sqrt()).max()))
    assert bool(((est - p).abs() <= 6 * (p * (1 - p) / R).sqrt()).all())
    # ... and so does every other card of every slot
    pc, ec = prior / 45, b.counts.double() / wsum.unsqueeze(2)
    assert bool(((ec - pc).abs() <= 6 * (pc * (1 - pc) / R).sqrt() + 1e-12).all())
    assert 0.0 <= b.joint_rate() < b.hit_rate() < 0.1 and b.hit_rate() == pytest.approx(b.prior_rate(), abs=2e-3)
    assert b.cross_entropy() == pytest.approx(b.prior_cross_entropy(), rel=2e-2)


@pytest.mark.parametrize("kw", [{}, {"condition": True, "depth": 2, "oversample": 4}], ids=["v0", "depth2"])
def test_search_player_scores_without_changing_a_move(kw):
    import torch

    from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR
    from hanabi_hip import Evaluator, SearchPlayer

    class Counting(SearchPlayer):
        """SearchPlayer that also adds up, by itself, the hand sizes of its seat over the live roots it is asked about."""
        cards_seen = roots_seen = 0

        def eval_moves(self, observations, seed, draw, actions_out, scratch=None):
            env = observations[0] if isinstance(observations, (tuple, list)) else observations
            rows = env.export_state()
            live = ((rows[:, 0] >> 19) & 3) == 0
            self.cards_seen += int((((rows[:, 1] >> (15 + 3 * self.seat)) & 7) * live).sum())
            self.roots_seen += int(live.sum())
            return super().eval_moves(observations, seed, draw, actions_out, scratch=scratch)

    n = 64
    team = [RulebasedAgent(PR.piers_rules, seed=30), RulebasedAgent(PR.piers_rules, seed=31)]
    ev = Evaluator("Hanabi-Small", 2, n_games=n, seed=7, record_actions=True)
    off = SearchPlayer(team, 0, replicas=4, seed=2, **kw)
    on = Counting(team, 0, replicas=4, seed=2, score_belief=True, **kw)
    r_off, r_on = ev.run([off, team[1]]), ev.run([on, team[1]])
    assert torch.equal(r_off.scores, r_on.scores) and torch.equal(r_off.moves, r_on.moves) and torch.equal(r_off.actions, r_on.actions)
    for name in SearchPlayer.COUNTERS + ("rollouts", "dead_replicas", "replicas_drawn", "searches"):
        assert getattr(off, name) == getattr(on, name), name
    assert off._belief is None and off.last_result.belief is None and off.belief_stats()["cards"] == 0
    st = on.belief_stats()
    print(st)
    # (the exact filter hands out dead copies of the root where it runs short of survivors: they weigh, and count, nothing)
    assert (on.dead_replicas > 0 if kw else on.dead_replicas == 0) and st["roots"] == on.roots_seen == on.moves and st["cards"] == on.cards_seen > st["roots"]
    assert sum(st["by_slot"]["cards"]) == st["cards"] and len(st["by_slot"]["cards"]) == 2
    for k in ("hit_rate", "prior_rate", "joint_rate"):
        assert 0.0 <= st[k] <= 1.0 and all(0.0 <= v <= 1.0 for v in st["by_slot"].get(k, []))
    assert st["joint_rate"] <= st["hit_rate"] and 0.0 < st["prior_rate"] and 0.0 < st["hit_rate"]
    assert 0.0 < st["cross_entropy"] < math.inf and 0.0 < st["prior_cross_entropy"] < math.log(20)   # (Small: 20 cards)
    if kw:
        c, u = st["conditioned"], st["unconditioned"]
        assert c["roots"] == on.conditioned > 0 and u["roots"] == on.unconditioned > 0
        assert c["cards"] + u["cards"] == st["cards"] and c["roots"] + u["roots"] == st["roots"]
        for k, count in (("hit_rate", "cards"), ("prior_rate", "cards"), ("cross_entropy", "cards"), ("joint_rate", "roots")):
            assert (c[k] * c[count] + u[k] * u[count]) / st[count] == pytest.approx(st[k], rel=1e-9)
    else:
        assert "conditioned" not in st
    on.reset_stats()
    assert on.belief_stats()["cards"] == 0


def _dqn(env, seed):
    from hanabi_agents.rlax_dqn import ActionSpec, DQNAgent, ObservationSpec, RlaxRainbowParams

    params = RlaxRainbowParams(train_batch_size=64, experience_buffer_size=8192, compute_dtype="bfloat16", packed_obs=True, layers=[512],
                               mask_terminal=True, seed=seed)
    return DQNAgent(ObservationSpec((env.n, env.obs_len)), ActionSpec(env.num_actions), params, device="cuda")


@pytest.mark.parametrize("level", [1, 2])
def test_off_belief_session_scores_without_changing_the_training(level):
    import torch

    import hanabi_hip
    from hanabi_hip import OffBeliefSession
    from hanabi_hip.obl import frozen_copy

    n, steps = 128, 12

    def run(score):
        torch.manual_seed(0)
        env = hanabi_hip.HanabiEnv("Hanabi-Small", 2, n_games=n, seed=11, packed=True)
        agents = [_dqn(env, seed=s) for s in (1, 2)]
        kw = dict(belief_policy=[frozen_copy(a) for a in agents], depth=2, oversample=4) if level == 2 else {}
        sess = OffBeliefSession(env, agents, belief_seed=5, score_belief=score, **kw)
        sess.run(steps)
        sess.flush()
        torch.cuda.synchronize()
        return sess, [torch.cat([p.detach().reshape(-1) for p in a.online.parameters()]).clone() for a in agents], env.export_state()

    off, w_off, rows_off = run(False)
    on, w_on, rows_on = run(True)
    assert off.grad_steps == on.grad_steps > 0 and torch.equal(rows_off, rows_on)
    for a, b in zip(w_off, w_on):
        assert torch.equal(a, b)
    assert [getattr(off, k) for k in OffBeliefSession.BELIEF_COUNTERS] == [0, 0.0, 0.0, 0.0, 0] and off._belief is None
    c = {k: getattr(on, k) for k in OffBeliefSession.BELIEF_COUNTERS}
    print(c)
    assert on.dead_rows == 0 and c["belief_roots"] == n * steps and c["belief_cards"] == 2 * n * steps   # (auto-reset: every row is live)
    assert 0.0 < c["belief_joint_sum"] <= c["belief_hit_sum"] <= c["belief_cards"]
    assert c["belief_hit_sum"] == float(int(c["belief_hit_sum"]))   # one replica per game: a slot is right or it is not
    assert 0.0 < c["belief_prior_sum"] < c["belief_cards"]
    if level == 2:
        assert on.conditioned_rows == off.conditioned_rows > 0
