"""The tracked belief on the GPU (hanabi_hip.search, csrc/belief.hip): hb_belief_carry against the numpy restatement
hanabi_hip.belief_carry_ref byte for byte on rows and weights (tests/test_belief_carry_cpu.py holds the restatement to hand-worked
cases and to the enumerated posterior), TrackedBelief.step against the same pipeline called by hand, and SearchPlayer(track=...)
on 64 games of Hanabi-Full against [Piers, Piers]."""
import numpy as np
import pytest
from search_util import _u32

pytestmark = pytest.mark.gpu

GUARD = 16
FILL = 0x5A5A5A5A
SEED, DRAW = (0x9E37 << 40) | 77, (3 << 33) | 5   # 64-bit Philox keys: the high words count


def _guarded(n_words, shift):
    """(buffer, view): n_words int32 between GUARD + shift sentinels before and GUARD after; shift = 1 leaves the view 4 bytes off
    a 16-byte boundary."""
    import torch

    buf = torch.full((n_words + 2 * GUARD + shift,), FILL, dtype=torch.int32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf, buf[GUARD + shift:GUARD + shift + n_words]


def _intact(buf, n_words, shift):
    b = _u32(buf)
    return (b[:GUARD + shift] == FILL).all() and (b[GUARD + shift + n_words:] == FILL).all()


_TRIPLES = {}


def _triples(game):
    """Transitions of real play, by the open-handed driver of tests/deep_play.py on the oracle's env: seat -> a list of (then, prev,
    now, my move, kind) with `then` my turn (running), `prev` the state the partner moved from, `now` two moves on; kind is
    "early" (the first four turns), "late" (the deck is empty now, the partner's hand short among them), "over" (the game has ended by now), "middle", or
    "short" (see below). The list interleaves the kinds, late first, so that every m >= 5 takes one of each."""
    if game in _TRIPLES:
        return _TRIPLES[game]
    from deep_play import open_hand_moves
    from oracle import oracle_py as O

    cfg = O.make_config(game, 2, 0)
    env = O.OracleEnv(cfg, 48, seed=9)
    legal, rng = env.observe()["legal"], np.random.default_rng(4)
    hist, moves = [np.asarray(env.export_state()).astype(np.uint32).copy()], []
    for t in range(76 if game == "Hanabi-Full" else 40):
        act = open_hand_moves(cfg, hist[-1], legal, rng, 0.05)
        moves.append(np.asarray(act).copy())
        legal = env.step(act)["legal"]
        hist.append(np.asarray(env.export_state()).astype(np.uint32).copy())
    kinds = {0: {}, 1: {}}
    for t in range(len(moves) - 1):
        then, prev, now = hist[t], hist[t + 1], hist[t + 2]
        for i in range(then.shape[0]):
            if (then[i, 0] >> 19) & 3:
                continue
            over = (now[i, 0] >> 19) & 3 != 0
            kind = "over" if over else "early" if t < 4 else "late" if now[i, 0] & 63 == 0 else "middle"
            kinds[t % 2].setdefault(kind, []).append((then[i], prev[i], now[i], int(moves[t][i]), kind))
    out = {}
    for seat, by in kinds.items():
        assert all(len(by.get(k, [])) >= 4 for k in ("early", "middle", "late", "over")), {k: len(v) for k, v in by.items()}
        H = cfg.hand_size
        # with 2 players the seat to act never holds a short hand in a running game (the game ends with its own last move), so the
        # "no card to draw" branch comes from late transitions edited by hand: my newest card, drawn as the deck's last, taken out
        # again (hand size, hand word), as if the deck had run out one card earlier
        card_move = [x for x in by["late"] if x[3] < 2 * H and (x[2][1] >> (15 + 3 * seat)) & 7 == H]
        assert card_move and any((x[2][1] >> (15 + 3 * (1 - seat))) & 7 < H for x in by["late"])   # (the partner's hand is short)
        short = []
        for then, prev, now, mv, _ in card_move[:4]:
            now = now.copy()
            now[1] = (int(now[1]) & ~(7 << (15 + 3 * seat))) | ((H - 1) << (15 + 3 * seat))
            now[10 + seat] = int(now[10 + seat]) | (31 << (5 * (H - 1)))
            short.append((then, prev, now, mv, "short"))
        n = max(len(v) for v in by.values())
        out[seat] = [v[j % len(v)] for j in range(n) for v in (by["late"], by["early"], by["middle"], by["over"], short)]
    _TRIPLES[game] = (cfg, out)
    return _TRIPLES[game]


def _inputs(game, m, Kn, seat, rng):
    """cur [m, SW], old [m * K, SW], old weights, own_slot, revealed, drew (numpy) for m roots of _triples: per root the particles
    are, in turn, the true old hand, V0-like shuffles of the cards I could not see then, the true hand with one card swapped for
    another of the pool, and hand words of random 5-bit fields (31 and ids >= NC among them); a third of the weights zeroed."""
    import torch

    from hanabi_hip import TrackedBelief

    cfg, by_seat = _triples(game)
    tri = [by_seat[seat][j % len(by_seat[seat])] for j in range(m)]
    then, prev, now = (np.stack([x[k] for x in tri]) for k in range(3))
    mv = np.array([x[3] for x in tri], np.int32)
    as_t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32).copy())
    slot, rev, drew = (t.numpy() for t in TrackedBelief(game, 2).observed(as_t(now), as_t(then), torch.from_numpy(mv), as_t(prev), seat))
    H, D, P = cfg.hand_size, 50 if game == "Hanabi-Full" else 20, 2
    old = np.repeat(then, Kn, axis=0)
    for i in range(m):
        n_h = int((then[i, 1] >> (15 + 3 * seat)) & 7)
        deck = np.ascontiguousarray(then[i, 10 + 3 * P:], dtype="<u4").view(np.uint8)
        size = int(then[i, 0] & 63)
        true = [(int(then[i, 10 + seat]) >> (5 * s)) & 31 for s in range(n_h)]
        pool = true + [int(c) for c in deck[D - size:D]]
        for k in range(Kn):
            mode = k % 4
            if mode == 0:
                hand = list(true)
            elif mode == 1:
                hand = [pool[j] for j in rng.permutation(len(pool))[:n_h]]
            elif mode == 2:
                hand = list(true)
                if n_h:
                    hand[int(rng.integers(n_h))] = pool[int(rng.integers(len(pool)))]
            else:
                hand = [int(x) for x in rng.integers(0, 32, H)]
            word = int(then[i, 10 + seat]) & ~0x1FFFFFF | 0x1FFFFFF
            for s, c in enumerate(hand):
                word = (word & ~(31 << (5 * s))) | (c << (5 * s))
            old[i * Kn + k, 10 + seat] = word
    ow = rng.integers(1, 1 << 32, m * Kn, dtype=np.uint64).astype(np.uint32)
    ow[rng.random(m * Kn) < 1 / 3] = 0
    return cfg, now, old, ow, slot, rev, drew


@pytest.mark.parametrize("game", ["Hanabi-Full", "Hanabi-Small"])
@pytest.mark.parametrize("m", [1, 3, 4, 5, 65])
def test_kernel_equals_the_restatement(game, m):
    """K in {1, 63, 64, 65, 130}, the observer's seat and the buffers' alignment alternating with K: real transitions (early,
    middle, late with an empty deck and short hands, finished), every output between sentinels, rows and weights compared with the
    restatement byte for byte; the same call split in two gives the same rows."""
    import torch

    import hanabi_hip
    from hanabi_hip import belief_carry, belief_carry_ref

    hcfg = hanabi_hip.make_config(game, 2, 0)
    rng = np.random.default_rng(m)
    for j, Kn in enumerate((1, 63, 64, 65, 130)):
        seat, shift = j % 2, (j // 2) % 2
        cfg, cur, old, ow, slot, rev, drew = _inputs(game, m, Kn, seat, rng)
        SW, n = cur.shape[1], m * Kn
        want_rows, want_w, info = belief_carry_ref(cfg, cur, old, ow, slot, rev, drew, seat, Kn, SEED, DRAW, first_row_id=1000, details=True)
        dev = {}
        for name, a in (("cur", cur), ("old", old)):   # the row inputs at the same (mis)alignment as the outputs
            buf, view = _guarded(a.size, shift)
            view.copy_(torch.from_numpy(a.view(np.int32).reshape(-1)))
            dev[name] = view.view(a.shape)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32) if a.dtype == np.uint32 else a.astype(np.int32)).cuda()
        ow_d, slot_d, rev_d, drew_d = t(ow), t(slot), t(rev), t(drew)
        rbuf, rview = _guarded(n * SW, shift)
        wbuf, wview = _guarded(n, shift)
        rows, w = belief_carry(hcfg, dev["cur"], dev["old"], ow_d, slot_d, rev_d, drew_d, seat, Kn, SEED, DRAW, first_row_id=1000,
                               out=(rview.view(n, SW), wview))
        torch.cuda.synchronize()
        assert _intact(rbuf, n * SW, shift) and _intact(wbuf, n, shift)
        assert np.array_equal(_u32(w), want_w), (game, m, Kn)
        assert np.array_equal(_u32(rows), want_rows), (game, m, Kn)
        if m >= 2:   # a split call: the row ids, not the call, key the draws
            h = m // 2
            for lo, hi in ((0, h), (h, m)):
                part = belief_carry(hcfg, dev["cur"][lo:hi].contiguous(), dev["old"][lo * Kn:hi * Kn].contiguous(), ow_d[lo * Kn:hi * Kn].contiguous(),
                                    slot_d[lo:hi].contiguous(), rev_d[lo:hi].contiguous(), drew_d[lo:hi].contiguous(), seat, Kn, SEED, DRAW,
                                    first_row_id=1000 + lo * Kn)
                assert np.array_equal(_u32(part[0]), want_rows[lo * Kn:hi * Kn]) and np.array_equal(_u32(part[1]), want_w[lo * Kn:hi * Kn])
        if m == 65 and Kn == 130:   # every branch of the rule in this one call
            dead = {d["dead"] for d in info}
            assert {0, 1, 2, 4} <= dead, dead
            root = lambda o: o // Kn
            live = [(o, d) for o, d in enumerate(info) if d["dead"] == 0]
            assert any(slot[root(o)] < 0 for o, d in live) and any(slot[root(o)] >= 0 for o, d in live)           # hints and card moves
            assert any(d["g"] > 1 for o, d in live) and any(drew[root(o)] < 0 for o, d in live)                     # g from the draw, and none
            assert any(d["ns"] == [] and slot[root(o)] >= 0 and cur[root(o), 0] & 63 == 0 for o, d in live)         # empty deck, short hand
            assert any(len(d["ns"]) == 1 and cur[root(o), 0] & 63 == 0 for o, d in live)                            # the deck's last card
            assert any(len(d["ns"]) == 1 for o, d in live)                                                          # a new slot
            assert any((cur[i, 0] >> 19) & 3 for i in range(m)) and (ow == 0).any()                                 # finished roots, dead inputs
            # the partner drew a card of the kind my new slot took: the k (k + 1) case
            hand_of = lambda o: [(int(want_rows[o, 10 + seat]) >> (5 * s)) & 31 for s in range(5)]
            assert any(len(d["ns"]) == 1 and d["g"] > 1 and hand_of(o)[len(d["kept"])] == drew[root(o)] for o, d in live)


def _piers():
    from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR

    return [RulebasedAgent(PR.piers_rules, seed=30), RulebasedAgent(PR.piers_rules, seed=31)]


def _ask(agent, env, seed, draw, out):
    agent.eval_moves(env, seed, draw, out)


@pytest.mark.parametrize("epsilon", [None, 0.1])
def test_tracked_step_equals_the_pipeline_by_hand(epsilon):
    import torch

    import hanabi_hip
    from hanabi_hip import (ConditionedDeterminizer, TrackedBelief, belief_carry, belief_select_soft, belief_splice, exact_table,
                            last_move_uid, soft_table)

    m, R, ov, seed, pseed = 48, 4, 3, 5, 7
    Kn = R * ov
    team = _piers()
    env = hanabi_hip.HanabiEnv("Hanabi-Full", 2, n_games=m, seed=3, auto_reset=False, packed=True)
    act = torch.zeros(m, dtype=torch.int32, device="cuda")
    tb = TrackedBelief("Hanabi-Full", 2, replicas=R, oversample=ov)
    draw, then = 1, None
    for turn in range(9):   # seat 0 observes on even turns: four tracked steps after the first
        seat = turn % 2
        rows = env.export_state().clone()
        if seat == 0:
            if then is None:
                got = tb.step(rows, None, None, rows, torch.zeros(m, dtype=torch.uint8, device="cuda"), team[1], 0, seed, draw, pseed,
                              draw - 1, env.first_game_id, epsilon=epsilon)
                assert bool(got.restarted.all()) and not bool(got.tracked.any()) and bool((got.fallback == 2).all())
            else:
                then_rows, then_moves, prev_rows = then
                valid = torch.ones(m, dtype=torch.uint8, device="cuda")
                valid[5] = 0   # one root without a usable previous turn: it starts over
                old_rows, old_w, have = tb.rows.clone(), tb.weights.clone(), tb.have.clone()
                got = tb.step(rows, then_rows, then_moves, prev_rows, valid, team[1], 0, seed, draw, pseed, draw - 1, env.first_game_id,
                              epsilon=epsilon)
                # ---- the same by hand ----
                cfg = tb.cfg
                live = ((rows[:, 0] >> 19) & 3) == 0
                usable = live & have & (valid != 0)
                slot, rev, drew = tb.observed(rows, then_rows, then_moves, prev_rows, 0)
                c_rows, c_w = belief_carry(cfg, rows, old_rows, torch.where(usable.repeat_interleave(Kn), old_w, 0), slot, rev, drew, 0, Kn,
                                           seed, draw)
                prev = torch.where(usable.view(m, 1), prev_rows, rows).contiguous()
                slabs = belief_splice(cfg, prev, c_rows, 0, Kn)
                scratch = hanabi_hip.HanabiEnv(config=cfg, n_games=m, device="cuda", packed=True)
                scratch.first_game_id = env.first_game_id
                hyp = torch.empty((1, Kn, m), dtype=torch.int32, device="cuda")
                nleg = torch.empty((1, Kn, m), dtype=torch.int32, device="cuda")
                for k in range(Kn):
                    scratch.import_state(slabs[k])
                    scratch.observe()
                    nleg[0, k] = scratch.legal.sum(1)
                    _ask(team[1], scratch, pseed, draw - 1, hyp[0, k])
                table = (exact_table(env.num_actions) if epsilon is None else soft_table(epsilon, env.num_actions)).cuda()
                actual = last_move_uid(cfg, rows).view(1, m)
                s_rows, s_w, n_surv, used, fb, ess = belief_select_soft(cfg, rows, c_rows, c_w, hyp, nleg, actual, usable.to(torch.uint8).view(1, m),
                                                                        table, Kn, seed, draw)
                tracked = usable & (s_w.view(m, Kn)[:, 0] != 0)
                restarted = live & ~tracked
                assert torch.equal(got.tracked, tracked) and torch.equal(got.restarted, restarted)
                assert bool(tracked.any()) and bool(restarted[5]) == bool(live[5])
                fresh = ConditionedDeterminizer("Hanabi-Full", 2).sample(rows, prev_rows, team[1], 0, Kn, 1, seed, draw, pseed, draw - 1,
                                                                         env.first_game_id, valid=valid, epsilon=epsilon)
                want_rows = torch.where(restarted.view(m, 1, 1), fresh.rows.view(m, Kn, -1), s_rows.view(m, Kn, -1))
                want_w = torch.where(restarted.view(m, 1), fresh.weights.view(m, Kn).int(), s_w.view(m, Kn))
                assert torch.equal(got.rows.view(m, Kn, -1), want_rows) and torch.equal(got.weights.view(m, Kn), want_w)
                assert torch.equal(got.carried_live, torch.where(tracked, (c_w.view(m, Kn) != 0).sum(1).int(), 0))
                assert torch.equal(got.n_surv[tracked], n_surv[0][tracked]) and torch.equal(got.ess[tracked], ess[tracked])
                assert bool((got.fallback[tracked] == 0).all()) and bool((got.depth_used[tracked] == 1).all())
                # a tracked root's particles all weigh 1, hold the kept cards of their ancestors, and, under the exact filter,
                # reproduce the partner's real move
                assert bool((got.weights.view(m, Kn)[tracked] == 1).all())
                if epsilon is None:
                    chosen = belief_splice(cfg, prev, got.rows, 0, Kn)
                    for k in range(Kn):
                        scratch.import_state(chosen[k])
                        _ask(team[1], scratch, pseed, draw - 1, hyp[0, k])
                    assert torch.equal(hyp[0][:, tracked], actual.expand(Kn, m)[:, tracked])
                assert got.rows is tb.rows and torch.equal(tb.have, live)
            _ask(team[0], env, pseed, draw, act)
            then = [rows, act.clone(), None]
        else:
            _ask(team[1], env, pseed, draw, act)
            if then is not None:
                then[2] = rows
        env.step(act)
        draw += 1


_GAMES = {}


def _games():
    """64 games of Hanabi-Full, [Piers, Piers], seat 0 searching: the default player, track=False, and track=True twice (the
    second a subclass that checks every call from the inside)."""
    if _GAMES:
        return _GAMES
    import torch

    import hanabi_hip
    from hanabi_hip import Evaluator, SearchPlayer, belief_splice, last_move_uid

    class Checked(SearchPlayer):
        """track=True, every call checked: the env's state is left as it was, and under the exact filter every live particle of a
        root whose belief was filtered reproduces the partner's real last move."""
        checked_particles = checked_calls = 0

        def _carry(self, env, rows, seed, draw, prev, valid, stack):
            got = super()._carry(env, rows, seed, draw, prev, valid, stack)
            m, Kn = rows.shape[0], got.n_particles
            filtered = got.tracked | (got.restarted & (got.fallback == 0))
            if bool(filtered.any()):
                slabs = belief_splice(env.cfg, torch.where(filtered.view(m, 1), prev, rows).contiguous(), got.rows, self.seat, Kn)
                if getattr(self, "_check_env", None) is None:
                    self._check_env = hanabi_hip.HanabiEnv(config=env.cfg, n_games=m, device=rows.device, packed=True)
                ce, out = self._check_env, torch.empty(m, dtype=torch.int32, device=rows.device)
                ce.first_game_id = env.first_game_id
                actual = last_move_uid(env.cfg, rows)
                for k in range(Kn):
                    ce.import_state(slabs[k])
                    self.blueprint[1 - self.seat].eval_moves(ce, int(seed), int(draw) - 1, out)
                    livek = filtered & (got.weights.view(m, Kn)[:, k] != 0)
                    assert torch.equal(out[livek], actual[livek])
                    self.checked_particles += int(livek.sum())
            return got

        def eval_moves(self, observations, seed, draw, actions_out, scratch=None):
            env = observations[0] if isinstance(observations, (tuple, list)) else observations
            before = env.export_state().clone()
            out = super().eval_moves(observations, seed, draw, actions_out, scratch=scratch)
            assert torch.equal(before, env.export_state())   # the session's env is left untouched
            self.checked_calls += 1
            return out

    team = _piers()
    ev = Evaluator("Hanabi-Full", 2, n_games=64, seed=7, record_actions=True)
    kw = dict(replicas=3, seed=2, z=1.0, condition=True, oversample=4, confirm_replicas=4)
    names = SearchPlayer.COUNTERS + ("rollouts", "dead_replicas", "replicas_drawn", "searches")
    for key, player in (("default", SearchPlayer(team, 0, **kw)), ("off", SearchPlayer(team, 0, track=False, **kw)),
                        ("on", SearchPlayer(team, 0, track=True, score_belief=True, **kw)), ("on2", Checked(team, 0, track=True, **kw))):
        res = ev.run([player, team[1]])
        _GAMES[key] = dict(player=player, scores=res.scores.clone(), actions=res.actions.clone(), lengths=res.lengths.clone(),
                           counters={k: int(getattr(player, k)) for k in names + SearchPlayer.TRACK_COUNTERS})
    return _GAMES


def test_search_player_without_tracking_is_the_old_player():
    """track=False is the default player move for move and counter for counter (tests/test_search_belief_gpu.py holds that player
    to the recording of tests/golden/search_belief_lastmove.json), and allocates nothing."""
    import torch

    g = _games()
    for k in ("scores", "actions", "lengths"):
        assert torch.equal(g["default"][k], g["off"][k]), k
    assert g["default"]["counters"] == g["off"]["counters"]
    off = g["off"]["player"]
    assert off._tracked is None and off._track_stats is None and off._belief_track is None and off._track_ess is None
    assert (off.tracked, off.restarts, off.carried_live) == (0, 0, 0) and "carried_ess" not in off.depth_stats()


def test_search_player_tracks_and_repeats_itself():
    import torch

    g = _games()
    for k in ("scores", "actions", "lengths"):
        assert torch.equal(g["on"][k], g["on2"][k]), k   # the same games twice
    assert g["on"]["counters"] == g["on2"]["counters"]
    c, on, on2 = g["on"]["counters"], g["on"]["player"], g["on2"]["player"]
    print(c, on.depth_stats(), float(g["on"]["scores"].float().mean()), float(g["off"]["scores"].float().mean()))
    K = on.replicas * on.oversample
    assert c["tracked"] > 0 and c["restarts"] >= 64   # every game starts over at least at its first move
    assert c["tracked"] + c["restarts"] == c["conditioned"] + c["unconditioned"] == c["moves"]
    assert c["unconditioned"] <= c["restarts"] and c["candidates"] == c["conditioned"] * K
    assert 0 < c["carried_live"] <= c["tracked"] * K and c["depth_used"] <= c["conditioned"]
    assert 1.0 <= on.depth_stats()["carried_ess"] <= K
    assert on2.checked_calls == on2.searches > 0 and on2.checked_particles > c["tracked"]
    st = on.belief_stats()
    t, r = st["tracked"], st["restarted"]
    assert t["roots"] == c["tracked"] and r["roots"] == c["restarts"] and t["cards"] + r["cards"] == st["cards"]
    assert (t["hit_rate"] * t["cards"] + r["hit_rate"] * r["cards"]) / st["cards"] == pytest.approx(st["hit_rate"], rel=1e-9)
    assert 0.0 < t["hit_rate"] <= 1.0 and 0.0 < t["joint_rate"] <= t["hit_rate"]
    on.reset_stats()
    assert (on.tracked, on.restarts, on.carried_live) == (0, 0, 0) and on.depth_stats()["carried_ess"] == 0.0
