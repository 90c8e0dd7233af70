"""What conditioning the search belief on the partner's last move is worth (hanabi_hip.search) on one
MI355X: the evaluator, blueprint, seed and thresholds of scripts/search_confirm_probe.py — Evaluator(n_games=1024, seed=7),
[Piers, Piers], search seed 9, threshold 0 — at 32 replicas, for the threshold alone and for z = 2, one seat searching and both,
with `condition` off and on (oversample 8; z = 2 with both seats also at oversample 2 and 4). The condition=False rows are the
same seeds as confirm_probe.json's and must reproduce its scores exactly: the script checks that against the file when it is
there. Then the cost of ConditionedDeterminizer.sample alone on 1 024 roots ten turns into play, by oversample: the slope is the
price of one slab pass (import the m spliced rows, the partner's eval_moves).
Writes one JSON file.
Usage: search_belief_probe.py [--out profiles/search/belief_probe.json] [--games 1024]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "hanabi-agents_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR  # noqa: E402
from hanabi_hip import ConditionedDeterminizer, Determinizer, Evaluator, HanabiEnv, SearchPlayer  # noqa: E402

SETTINGS = [   # (label, z, seats, condition, oversample)
    ("plain_r32_seat0", None, (0,), False, 8), ("plain_r32_seat0_cond", None, (0,), True, 8),
    ("plain_r32_both", None, (0, 1), False, 8), ("plain_r32_both_cond", None, (0, 1), True, 8),
    ("z2_r32_seat0", 2.0, (0,), False, 8), ("z2_r32_seat0_cond", 2.0, (0,), True, 8),
    ("z2_r32_both", 2.0, (0, 1), False, 8), ("z2_r32_both_cond", 2.0, (0, 1), True, 8),
    ("z2_r32_both_cond_ov2", 2.0, (0, 1), True, 2), ("z2_r32_both_cond_ov4", 2.0, (0, 1), True, 4),
]


def timed(fn, repeat=3):
    best = None
    for _ in range(repeat + 1):   # (the first call builds envs and buffers)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search", "belief_probe.json"))
    ap.add_argument("--games", type=int, default=1024)
    args = ap.parse_args()
    out = dict(device=torch.cuda.get_device_name(0), setting=dict(game="Hanabi-Full", players=2, n_games=args.games, eval_seed=7,
                                                                 blueprint="[Piers, Piers]", search_seed=9, threshold=0.0, replicas=32),
               rows={}, cost={})
    piers = [RulebasedAgent(PR.piers_rules, seed=1), RulebasedAgent(PR.piers_rules, seed=2)]
    ev = Evaluator("Hanabi-Full", 2, n_games=args.games, seed=7)
    base = ev.run(piers)
    out["rows"]["blueprint"] = dict(mean=base.mean, stderr=base.stderr)
    print(json.dumps({"blueprint": out["rows"]["blueprint"]}), flush=True)
    for label, z, seats, cond, ov in SETTINGS:
        players = [SearchPlayer(piers, s, replicas=32, threshold=0.0, seed=9, z=z, condition=cond, oversample=ov) if s in seats
                   else piers[s] for s in range(2)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = ev.run(players)
        torch.cuda.synchronize()
        seconds = time.perf_counter() - t0
        sps = [p for p in players if isinstance(p, SearchPlayer)]
        mv, dv = sum(p.moves for p in sps), sum(p.deviations for p in sps)
        cn, sv, cd, fb = (sum(getattr(p, k) for p in sps) for k in ("conditioned", "survivors", "candidates", "fallbacks"))
        row = dict(z=z, seats=list(seats), condition=cond, oversample=ov if cond else None, mean=r.mean, stderr=r.stderr, moves=mv,
                   deviations=dv, deviation_rate=dv / max(mv, 1), conditioned=cn, survivor_share=(sv / cd if cd else None),
                   fallback_share=(fb / cn if cn else None), rollouts=sum(p.rollouts for p in sps),
                   dead_replicas=sum(p.dead_replicas for p in sps), seconds=seconds)
        out["rows"][label] = row
        print(json.dumps({label: row}), flush=True)
        del players, sps
        torch.cuda.empty_cache()
    for label, row in out["rows"].items():   # the filter's cost: conditioned over unconditioned seconds at equal replicas
        if label.endswith("_cond") or "_cond_ov" in label:
            row["seconds_over_unconditioned"] = row["seconds"] / out["rows"][label.split("_cond")[0]]["seconds"]
    ref_path = os.path.join(ROOT, "profiles", "search", "confirm_probe.json")
    if os.path.exists(ref_path) and args.games == 1024:
        ref = json.load(open(ref_path))["rows"]
        same = {k: out["rows"][k]["mean"] == ref[k]["mean"] for k in ("plain_r32_seat0", "plain_r32_both", "z2_r32_seat0", "z2_r32_both")}
        out["condition_off_reproduces_confirm_probe"] = same
        print(json.dumps({"condition_off_reproduces_confirm_probe": same}), flush=True)

    # ---- ConditionedDeterminizer.sample alone: 1 024 roots ten turns into [Piers, Piers] play, 32 replicas
    m, turns = 1024, 10
    env = HanabiEnv("Hanabi-Full", 2, n_games=m, seed=7, auto_reset=False, packed=True)
    act = torch.empty(m, dtype=torch.int32, device="cuda")
    prev = None
    for t in range(turns):
        piers[t % 2].eval_moves(env, 7, t + 1, act)
        prev = env.export_state()
        env.step(act)
    rows = env.export_state()
    det, cd = Determinizer("Hanabi-Full", 2), ConditionedDeterminizer("Hanabi-Full", 2)
    out["cost"]["determinize_r32_ms"] = 1e3 * timed(lambda: det.sample(rows, seat=0, replicas=32, seed=9, draw=11))
    for ov in (1, 2, 4, 8):
        res = []
        ms = 1e3 * timed(lambda: res.append(cd.sample(rows, prev, piers[1], 0, 32, ov, seed=9, draw=11, partner_seed=7, partner_draw=10,
                                                      first_game_id=0)))
        n_surv, fallback = res[-1].n_surv[0], res[-1].fallback
        out["cost"][f"conditioned_sample_ov{ov}"] = dict(ms=ms, slabs=32 * ov, survivor_share=float(n_surv.double().mean()) / (32 * ov),
                                                         roots_short_of_32=float((n_surv < 32).double().mean()),
                                                         fallback_share=float((fallback == 1).double().mean()))
    print(json.dumps({"cost": out["cost"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
