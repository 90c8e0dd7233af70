"""What the search's beliefs give the cards a seat really holds (hb_belief_score, hanabi_hip.search.belief_score; DESIGN.md
sections 11f "Scoring a belief" and 11g) on one MI355X, and what scoring costs.

  beliefs  Evaluator(n_games=1024, seed=7) on Full, 2 players, [Piers, Piers], both seats SearchPlayer(threshold=inf,
           score_belief=True, replicas=32, oversample=8, seed=9): with that threshold no configuration ever leaves the blueprint,
           so all of them search the same roots of the same games and the comparison is paired (the script checks it: same
           scores, same roots, same cards, same prior figures). Configurations: the V0 belief; condition=True at depth 1, 2, 4;
           the same three with epsilon=0.1; track=True (the belief tracked across turns, hb_belief_carry) over depth 1 and 4 and
           over depth 1 with epsilon=0.1. Per configuration: hit rate, joint rate, cross-entropy, the card-counting prior's
           figures, by slot, and the conditioned / unconditioned split; with track=True also the tracked / restarted split, the
           restart share, the mean live particles after the carry and the mean effective sample size.
  track    the cost of one tracked turn (TrackedBelief.step: carry, splice, one partner pass over the 256 slabs, resampling)
           against one depth=4 turn (ConditionedDeterminizer.sample_history: 256 candidates, four partner passes, one filter) on
           the same 1 024 roots 24 moves into [Piers, Piers] games, event-timed over whole turns, rotating through enough
           particle sets to exceed the 256 MB Infinity Cache; and hb_belief_carry alone, call by call (one launch between two
           events: an upper bound).
  kernel   hb_belief_score alone, event-timed call by call at m=1024, R=32 and m=32768, R=1 (with and without the per-card tally):
           median of CALLS calls after a warm-up, once on one set of buffers (cache-resident) and once rotating through enough
           sets to exceed the 256 MB Infinity Cache. One launch between two events is mostly launch overhead: upper bounds.
  obl      one OffBeliefSession at 32 768 games, level 2, depth 2, oversample 4; score_belief toggled between the windows of the
           SAME session (windows of STEPS steps, alternated, the order of the two legs swapped from round to round, all REPS
           figures in the order they were taken), and the counters' rates.
  resources (--resources-only: this part alone, needs no GPU) the compiler's resource line of belief_score_kernel.

Writes one JSON file.
Usage: belief_score_probe.py [--out profiles/search/belief_score_probe.json] [--games 1024] [--parts beliefs,kernel,obl,track]
       [--resources-only]   (parts that are not run keep what the file holds)"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "hanabi-agents_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

CONFIGS = [("v0", {})] + [(f"depth{d}{'_eps0.1' if eps else ''}", dict(condition=True, depth=d, **({"epsilon": eps} if eps else {})))
                          for eps in (None, 0.1) for d in (1, 2, 4)]
CONFIGS += [("track_depth1", dict(condition=True, depth=1, track=True)), ("track_depth4", dict(condition=True, depth=4, track=True)),
            ("track_depth1_eps0.1", dict(condition=True, depth=1, track=True, epsilon=0.1))]
CALLS, WARM_CALLS = 40, 10
N, STEPS, REPS, WARM = 32768, 200, 3, 80
CACHE_BYTES = 256 << 20


def beliefs(games):
    import torch

    from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR
    from hanabi_hip import Evaluator, SearchPlayer, belief_stats_of

    piers = [RulebasedAgent(PR.piers_rules, seed=1), RulebasedAgent(PR.piers_rules, seed=2)]
    ev = Evaluator("Hanabi-Full", 2, n_games=games, seed=7)
    base = ev.run(piers)   # (builds the evaluator's env outside the timed runs; the blueprint's own score)
    rows = {}
    for label, kw in CONFIGS:
        players = [SearchPlayer(piers, s, replicas=32, threshold=float("inf"), seed=9, oversample=8, score_belief=True, **kw)
                   for s in range(2)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = ev.run(players)
        torch.cuda.synchronize()
        seconds = time.perf_counter() - t0
        tot = lambda k: sum(getattr(p, k) for p in players)
        st = belief_stats_of(players[0].belief_sums() + players[1].belief_sums(), split=bool(kw))
        rows[label] = dict(kw, mean=r.mean, moves=tot("moves"), deviations=tot("deviations"), conditioned=tot("conditioned"),
                           fallbacks=tot("fallbacks"), dead_replicas=tot("dead_replicas"), seconds=seconds, belief=st)
        if kw.get("track"):
            both = [p.belief_stats() for p in players]
            merge = lambda k, name, count: sum(b[k][name] * b[k][count] for b in both) / max(sum(b[k][count] for b in both), 1)
            ess = [p.depth_stats()["carried_ess"] for p in players]
            rows[label].update(
                tracked=tot("tracked"), restarts=tot("restarts"), restart_share=tot("restarts") / max(tot("moves"), 1),
                mean_carried_live=tot("carried_live") / max(tot("tracked"), 1), particles=32 * 8,
                carried_ess=sum(e * p.tracked for e, p in zip(ess, players)) / max(tot("tracked"), 1),
                split={k: dict(roots=sum(b[k]["roots"] for b in both), hit_rate=merge(k, "hit_rate", "cards"),
                               joint_rate=merge(k, "joint_rate", "roots"), cross_entropy=merge(k, "cross_entropy", "cards"))
                       for k in ("tracked", "restarted")})
        print(json.dumps({label: rows[label]}), flush=True)
        del players
        torch.cuda.empty_cache()
    first = rows["v0"]
    same = lambda a, b: abs(a - b) <= 1e-12 * max(abs(a), abs(b))   # (the same terms, summed in the same order)
    paired = all(r["mean"] == base.mean and r["deviations"] == 0 and r["moves"] == first["moves"] and
                 r["belief"]["cards"] == first["belief"]["cards"] and r["belief"]["roots"] == first["belief"]["roots"] and
                 same(r["belief"]["prior_rate"], first["belief"]["prior_rate"]) and
                 same(r["belief"]["prior_cross_entropy"], first["belief"]["prior_cross_entropy"]) for r in rows.values())
    if not paired:
        raise SystemExit("the configurations did not search the same roots: the comparison is not paired")
    return dict(setting=dict(game="Hanabi-Full", players=2, n_games=games, eval_seed=7, blueprint="[Piers, Piers]", search_seed=9,
                             threshold="inf", replicas=32, oversample=8, seats="both", blueprint_mean=base.mean),
                paired=paired, rows=rows)


def kernel():
    import torch

    import hanabi_hip
    from hanabi_hip import Determinizer, belief_score

    out = {}
    for m, R in ((1024, 32), (32768, 1)):
        env = hanabi_hip.HanabiEnv("Hanabi-Full", 2, n_games=m, seed=3, auto_reset=False, packed=True)
        for t in range(12):
            env.step(env.random_legal_actions(seed=4, draw=t))
        rows = env.export_state()
        SW = rows.shape[1]
        det, w = Determinizer(config=env.cfg).sample(rows, seat=-1, replicas=R, seed=9, draw=0, out=(
            torch.empty((m * R, SW), dtype=torch.int32, device="cuda"), torch.empty(m * R, dtype=torch.int32, device="cuda")))
        per_set = rows.numel() * 4 + det.numel() * 4 + w.numel() * 4
        n_sets = -(-CACHE_BYTES * 5 // 4 // per_set)
        sets = [(rows, det, w)] + [(rows.clone(), det.clone(), w.clone()) for _ in range(n_sets - 1)]
        for counts in (False, True):
            first = belief_score(env.cfg, rows, det, w, -1, R, counts=counts)
            bufs = (first.truth, first.hit, first.joint, first.wsum, first.n_live, first.prior) + ((first.counts,) if counts else ())
            leg = dict(m=m, replicas=R, counts=counts, calls=CALLS, input_bytes_per_call=per_set, sets_rotated=n_sets)
            for name, ring in (("cache_resident", sets[:1]), ("rotated", sets)):
                for k in range(WARM_CALLS):
                    belief_score(env.cfg, *ring[k % len(ring)], -1, R, counts=counts, out=bufs)
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(CALLS)]
                torch.cuda.synchronize()
                for k, (a, b) in enumerate(ev):
                    a.record()
                    belief_score(env.cfg, *ring[(WARM_CALLS + k) % len(ring)], -1, R, counts=counts, out=bufs)
                    b.record()
                torch.cuda.synchronize()
                us = sorted(a.elapsed_time(b) * 1000 for a, b in ev)
                leg[name + "_us_upper_bound"] = dict(median=round(statistics.median(us), 2), min=round(us[0], 2), max=round(us[-1], 2))
            out[f"m{m}_r{R}{'_counts' if counts else ''}"] = leg
            print(json.dumps(leg), flush=True)
        del sets, det, w, env
        torch.cuda.empty_cache()
    out["note"] = ("one launch between two events: launch overhead and the events' own resolution are in every figure, so these are "
                   "host-bound upper bounds on the kernel's time, not kernel times")
    return out


def track():
    import torch

    import hanabi_hip
    from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR
    from hanabi_hip import ConditionedDeterminizer, PartnerHistory, TrackedBelief, belief_carry, last_move_uid

    m, R, ov, depth, seed, pseed = 1024, 32, 8, 4, 9, 7
    Kn = R * ov
    piers = [RulebasedAgent(PR.piers_rules, seed=1), RulebasedAgent(PR.piers_rules, seed=2)]
    env = hanabi_hip.HanabiEnv("Hanabi-Full", 2, n_games=m, seed=3, auto_reset=False, packed=True)
    act = torch.zeros(m, dtype=torch.int32, device="cuda")
    tb = TrackedBelief("Hanabi-Full", 2, replicas=R, oversample=ov)
    hist = PartnerHistory(env.cfg, m, depth, "cuda", partner_seed=pseed, first_game_id=env.first_game_id)
    ones, then, last = torch.ones(m, dtype=torch.uint8, device="cuda"), None, None
    for turn in range(25):   # seat 0 observes on even turns; the last of them is the one timed
        rows, draw = env.export_state().clone(), turn + 1
        if turn % 2 == 0:
            if then is not None:
                hist.own_move(then[1])
                hist.push(then[2], last_move_uid(env.cfg, rows), draw - 1, ones, seat=0)
                last = dict(rows=rows, then_rows=then[0], then_moves=then[1], prev_rows=then[2], draw=draw,
                            old=(tb.rows.clone(), tb.weights.clone(), tb.have.clone()))
            tb.step(rows, *(then if then is not None else (None, None, rows)), None if then is not None else ones * 0, piers[1], 0, seed, draw,
                    pseed, draw - 1, env.first_game_id)
            piers[0].eval_moves(env, pseed, draw, act)
            then = [rows, act.clone(), None]
        else:
            piers[1].eval_moves(env, pseed, draw, act)
            then[2] = rows
        env.step(act)
    per_set = sum(t.numel() * t.element_size() for t in last["old"][:2])
    n_sets = -(-CACHE_BYTES * 5 // 4 // per_set)
    sets = [tuple(t.clone() for t in last["old"]) for _ in range(n_sets)]
    cdet = ConditionedDeterminizer(config=env.cfg)
    a = last

    def tracked_turn(k):
        tb.rows, tb.weights, tb.have = (t for t in sets[k % n_sets])   # (step swaps its buffers: the set comes back as scratch)
        tb._next = (torch.empty_like(tb.rows), torch.empty_like(tb.weights)) if k < 2 else tb._next
        return tb.step(a["rows"], a["then_rows"], a["then_moves"], a["prev_rows"], ones, piers[1], 0, seed, a["draw"], pseed, a["draw"] - 1,
                       env.first_game_id)

    def depth_turn(k):
        return cdet.sample_history(a["rows"], hist, piers[1], 0, R, ov, seed, a["draw"], pseed, env.first_game_id)

    out = dict(m=m, particles=Kn, depth=depth, turns_timed=10, particle_bytes_per_set=per_set, sets_rotated=n_sets)
    for name, fn in (("tracked_turn_ms", tracked_turn), ("depth4_turn_ms", depth_turn)):
        for k in range(2):
            got = fn(k)
        if name == "tracked_turn_ms":
            out.update(tracked_roots=int(got.tracked.sum()), restarted_roots=int(got.restarted.sum()),
                       mean_carried_live=float(got.carried_live.sum()) / max(int(got.tracked.sum()), 1))
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(10)]
        torch.cuda.synchronize()
        for k, (e0, e1) in enumerate(ev):
            sets[(k + 2) % n_sets] = tuple(t.clone() for t in last["old"]) if name == "tracked_turn_ms" else sets[(k + 2) % n_sets]
            e0.record()
            fn(k + 2)
            e1.record()
        torch.cuda.synchronize()
        ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
        out[name] = dict(median=round(statistics.median(ms), 3), min=round(ms[0], 3), max=round(ms[-1], 3))
    slot, rev, drew = tb.observed(a["rows"], a["then_rows"], a["then_moves"], a["prev_rows"], 0)
    sets = [tuple(t.clone() for t in last["old"]) for _ in range(n_sets)]
    bufs = (torch.empty_like(last["old"][0]), torch.empty_like(last["old"][1]))
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(CALLS)]
    for k in range(WARM_CALLS):
        belief_carry(env.cfg, a["rows"], sets[k % n_sets][0], sets[k % n_sets][1], slot, rev, drew, 0, Kn, seed, a["draw"], out=bufs)
    torch.cuda.synchronize()
    for k, (e0, e1) in enumerate(ev):
        e0.record()
        belief_carry(env.cfg, a["rows"], sets[k % n_sets][0], sets[k % n_sets][1], slot, rev, drew, 0, Kn, seed, a["draw"], out=bufs)
        e1.record()
    torch.cuda.synchronize()
    us = sorted(e0.elapsed_time(e1) * 1000 for e0, e1 in ev)
    out["carry_kernel_us_upper_bound"] = dict(median=round(statistics.median(us), 2), min=round(us[0], 2), max=round(us[-1], 2),
                                              rows_per_call=m * Kn)
    out["note"] = ("whole turns between two events (dozens of launches each; the restart decision's one synchronisation is inside the "
                   "tracked turn); the single-kernel figure is one launch between two events: a host-bound upper bound")
    print(json.dumps(out), flush=True)
    return out


def obl():
    import torch

    import hanabi_hip
    from hanabi_agents.rlax_dqn import ActionSpec, DQNAgent, ObservationSpec, RlaxRainbowParams
    from hanabi_hip import OffBeliefSession
    from hanabi_hip.obl import frozen_copy

    env = hanabi_hip.HanabiEnv("Hanabi-Full", 2, n_games=N, seed=1, packed=True)
    agents = [DQNAgent(ObservationSpec((env.n, env.obs_len)), ActionSpec(env.num_actions),
                       RlaxRainbowParams(seed=s, train_batch_size=256, experience_buffer_size=1 << 19, layers=[512], mask_terminal=True,
                                         compute_dtype="bfloat16", packed_obs=True), device="cuda") for s in (1, 2)]
    sess = OffBeliefSession(env, agents, belief_policy=[frozen_copy(x) for x in agents], depth=2, oversample=4, score_belief=True)

    def window(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            sess.step()
        sess.flush()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1000 / steps

    window(WARM)
    sess.score_belief = False   # both paths warm
    window(20)
    ms, order = {"off": [], "on": []}, []
    for rep in range(REPS):
        for leg in (("off", "on"), ("on", "off"))[rep % 2]:
            sess.score_belief = leg == "on"
            ms[leg].append(round(window(STEPS), 4))
            order.append(leg)
    c = {k: getattr(sess, k) for k in OffBeliefSession.BELIEF_COUNTERS}
    out = dict(games=N, level=2, depth=2, oversample=4, steps_per_window=STEPS, windows_per_leg=REPS, window_order=order, ms_per_step_runs=ms,
               ms_per_step_best={k: min(v) for k, v in ms.items()}, window_spread_ms={k: round(max(v) - min(v), 4) for k, v in ms.items()},
               counters=c, hit_rate=c["belief_hit_sum"] / max(c["belief_cards"], 1), prior_rate=c["belief_prior_sum"] / max(c["belief_cards"], 1),
               joint_rate=c["belief_joint_sum"] / max(c["belief_roots"], 1),
               conditioned_share=sess.conditioned_rows / max(sess.conditioned_rows + sess.fallback_rows + sess.unconditioned_rows, 1),
               note="an untrained agent and its frozen copy: the rates say what the counters read, not what a trained level-2 belief gives")
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search", "belief_score_probe.json"))
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--parts", default="beliefs,kernel,obl")
    ap.add_argument("--resources-only", action="store_true")
    args = ap.parse_args()
    out = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            out = json.load(f)

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)

    if args.resources_only:
        from obl_probe import kernel_resources

        out["resources"] = kernel_resources("belief.hip", only="belief_score")
        out["resources"].update(kernel_resources("belief.hip", only="belief_carry"))
        print(json.dumps(out["resources"]), flush=True)
        return save()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("belief_score_probe.py measures on the GPU: none found")
    out["device"] = torch.cuda.get_device_name(0)
    for part in args.parts.split(","):
        out[part] = {"beliefs": lambda: beliefs(args.games), "kernel": kernel, "obl": obl, "track": track}[part]()
        save()


if __name__ == "__main__":
    main()
