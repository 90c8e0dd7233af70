"""Cost and effect of depth-limited rollouts (RolloutSearch(horizon=H), DESIGN.md section 11f, "Depth-limited rollouts") on one MI355X.

(a) time: RolloutSearch.run for H in {1, 2, 4, 8, 16, None} on section 11f's setting (Full, 2 players, 1 024 roots ten turns of
    [Piers, Piers] in, 32 replicas, two untrained bf16 DQN agents), the horizons alternating inside every round so that all of them
    see the same machine; horizon=None is the unchanged full search.
(b) value shift: mean and RMS of value_H - value_full over the legal (root, action) pairs, on the same replicas (same seed and
    draw: the first H turns of every rollout are the same games), for the untrained agents (timing only: their q means nothing)
    and for agents trained briefly by scripts/train_small.py (run here, on Hanabi-Full).
(c) score: Evaluator(n_games=1024, seed=7) for the trained blueprint, SearchPlayer(horizon=H) in seat 0 and SearchPlayer() in seat 0.

Usage: search_horizon_probe.py [--out profiles/search/horizon_probe.json] [--train-steps 6000] [--rounds 7] [--score-horizons 2,8]"""
import argparse
import json
import os
import runpy
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "hanabi-agents_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import hanabi_hip  # noqa: E402
from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR  # noqa: E402
from hanabi_hip import Evaluator, RolloutSearch, SearchPlayer  # noqa: E402

HORIZONS = (1, 2, 4, 8, 16, None)


def dqn(env_like, seed):
    from hanabi_agents.rlax_dqn import ActionSpec, DQNAgent, ObservationSpec, RlaxRainbowParams

    params = RlaxRainbowParams(train_batch_size=128, experience_buffer_size=8192, compute_dtype="bfloat16", packed_obs=True,
                               layers=[512], seed=seed)
    return DQNAgent(ObservationSpec((1, env_like.obs_len)), ActionSpec(env_like.num_actions), params, device="cuda")


def time_horizons(rows, legal, team, R, rounds, window_s=0.3):
    """Per horizon: milliseconds per RolloutSearch.run, best and median over `rounds` windows; each window repeats the call until
    `window_s` seconds have passed (at least twice) and ends in a device synchronise. Every round visits every horizon."""
    searches = {H: RolloutSearch("Hanabi-Full", 2, replicas=R, seed=1, horizon=H) for H in HORIZONS}
    info = {}
    for H, rs in searches.items():   # warm-up: every shape, every path
        res = rs.run(rows, legal, team, draw=1)
        info[H] = dict(rollouts=res.rollouts, turns=res.turns, leaves=res.leaves)
    torch.cuda.synchronize()
    ms = {H: [] for H in HORIZONS}
    for _ in range(rounds):
        for H, rs in searches.items():
            calls, t0 = 0, time.perf_counter()
            while calls < 2 or time.perf_counter() - t0 < window_s:
                rs.run(rows, legal, team, draw=1)
                calls += 1
            torch.cuda.synchronize()
            ms[H].append((time.perf_counter() - t0) * 1e3 / calls)
    out = {}
    for H in HORIZONS:
        ts = sorted(ms[H])
        out["full" if H is None else f"H{H}"] = dict(best_ms=ts[0], median_ms=ts[len(ts) // 2], worst_ms=ts[-1], windows=rounds, **info[H])
    return out


def value_shift(rows, legal, team, R):
    """value_H - value_full over the legal (root, action) pairs with a value in both, on the same replicas."""
    full = RolloutSearch("Hanabi-Full", 2, replicas=R, seed=1).run(rows, legal, team, draw=1)
    out = {}
    for H in HORIZONS[:-1]:
        res = RolloutSearch("Hanabi-Full", 2, replicas=R, seed=1, horizon=H).run(rows, legal, team, draw=1)
        ok = ~torch.isnan(full.value) & ~torch.isnan(res.value)
        d = (res.value.double() - full.value.double())[ok]
        out[f"H{H}"] = dict(mean=float(d.mean()), rms=float(d.pow(2).mean().sqrt()), pairs=int(ok.sum()), leaves=res.leaves,
                            rollouts=res.rollouts, mean_value_H=float(res.value[ok].double().mean()),
                            mean_value_full=float(full.value[ok].double().mean()),
                            best_agrees=float((res.best == full.best).double().mean()))
        del res
        torch.cuda.empty_cache()
    return out


def train(steps):
    """scripts/train_small.py itself, on Hanabi-Full (2 048 games, 4 updates per step) -> (its two agents, seconds, its last lines)."""
    argv, sys.argv = sys.argv, [os.path.join(ROOT, "scripts", "train_small.py"), "Hanabi-Full", str(steps), "2048", "4"]
    t0 = time.perf_counter()
    try:
        g = runpy.run_path(sys.argv[0], run_name="train_small")
    finally:
        sys.argv = argv
    g["sess"].flush()
    torch.cuda.synchronize()
    return g["agents"], time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search", "horizon_probe.json"))
    ap.add_argument("--train-steps", type=int, default=6000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--score-horizons", default="2,8")
    args = ap.parse_args()
    out = dict(device=torch.cuda.get_device_name(0), setting="Hanabi-Full, 2 players, 1024 roots ten turns of [Piers, Piers] in, 32 replicas, "
               "two bf16 DQN agents (hidden 512, packed observations)")
    m, R = 1024, 32
    src = hanabi_hip.HanabiEnv("Hanabi-Full", 2, n_games=m, seed=3, auto_reset=False, packed=True)
    piers = [RulebasedAgent(PR.piers_rules, seed=1), RulebasedAgent(PR.piers_rules, seed=2)]
    for t in range(10):
        act = torch.empty(m, dtype=torch.int32, device="cuda")
        piers[t % 2].eval_moves(src, 5, t + 1, act)
        src.step(act)
    rows, legal = src.export_state(), src.legal.clone()
    untrained = [dqn(src, 1), dqn(src, 2)]
    out["time_untrained"] = time_horizons(rows, legal, untrained, R, args.rounds)
    print(json.dumps(dict(time_untrained=out["time_untrained"])), flush=True)
    torch.cuda.empty_cache()
    out["shift_untrained"] = dict(note="timing only: an untrained network's q means nothing", **value_shift(rows, legal, untrained, R))
    print(json.dumps(dict(shift_untrained=out["shift_untrained"])), flush=True)
    del untrained
    torch.cuda.empty_cache()
    if args.train_steps > 0:
        trained, seconds = train(args.train_steps)
        out["training"] = dict(script="scripts/train_small.py Hanabi-Full", steps=args.train_steps, games=2048, updates_per_step=4,
                               seconds=seconds)
        out["shift_trained"] = value_shift(rows, legal, trained, R)
        print(json.dumps(dict(shift_trained=out["shift_trained"])), flush=True)
        torch.cuda.empty_cache()
        ev = Evaluator("Hanabi-Full", 2, n_games=1024, seed=7)
        score = out["score_trained"] = {}
        horizons = [int(x) for x in args.score_horizons.split(",") if x] + [None]
        for label, H in [("blueprint", "none")] + [("search_full" if H is None else f"search_H{H}", H) for H in horizons]:
            sp = None if H == "none" else SearchPlayer(trained, 0, replicas=R, threshold=0.0, seed=9, horizon=H)
            t0 = time.perf_counter()
            r = ev.run(trained if sp is None else [sp, trained[1]])
            score[label] = dict(mean=r.mean, stderr=r.stderr, bombout_rate=r.bombout_rate, seconds=time.perf_counter() - t0)
            if sp is not None:
                score[label].update(moves=sp.moves, deviations=sp.deviations, rollouts=sp.rollouts, leaf_games=sp.leaf_games)
            print(json.dumps({label: score[label]}), flush=True)
            del sp
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
