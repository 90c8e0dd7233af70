"""What conditioning the search belief on the partner's last L moves is worth and costs (hanabi_hip.search, DESIGN.md section
11f) on one MI355X: the evaluator, blueprint, seeds and settings of scripts/search_belief_probe.py — Evaluator(n_games=1024,
seed=7), [Piers, Piers], search seed 9, threshold 0, 32 replicas, z = 2 — with one seat searching and both, condition on, at
depth 1, 2 and 4 and oversample 4 and 8. The depth-1 rows are the same seeds as belief_probe.json's and must reproduce its scores
exactly: the script checks that against the file when it is there. Per row: the score, the share of the candidates that
reproduce the last D moves (over the roots that have D usable ones), the share of the conditioned roots that use fewer moves
than they have, fallbacks, rollouts and seconds.
Writes one JSON file.
Usage: search_depth_probe.py [--out profiles/search/depth_probe.json] [--games 1024]"""
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
from hanabi_hip import Evaluator, SearchPlayer  # noqa: E402

SETTINGS = [(f"z2_r32_{name}_ov{ov}_d{depth}", seats, ov, depth)
            for name, seats in (("seat0", (0,)), ("both", (0, 1))) for ov in (4, 8) for depth in (1, 2, 4)]
SAME_AS = {"z2_r32_seat0_ov8_d1": "z2_r32_seat0_cond", "z2_r32_both_ov8_d1": "z2_r32_both_cond", "z2_r32_both_ov4_d1": "z2_r32_both_cond_ov4"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search", "depth_probe.json"))
    ap.add_argument("--games", type=int, default=1024)
    args = ap.parse_args()
    out = dict(device=torch.cuda.get_device_name(0), setting=dict(game="Hanabi-Full", players=2, n_games=args.games, eval_seed=7,
                                                                 blueprint="[Piers, Piers]", search_seed=9, threshold=0.0, replicas=32,
                                                                 z=2.0),
               rows={})
    piers = [RulebasedAgent(PR.piers_rules, seed=1), RulebasedAgent(PR.piers_rules, seed=2)]
    ev = Evaluator("Hanabi-Full", 2, n_games=args.games, seed=7)
    ev.run(piers)   # (builds the evaluator's env outside the timed runs)
    for label, seats, ov, depth in SETTINGS:
        players = [SearchPlayer(piers, s, replicas=32, threshold=0.0, seed=9, z=2.0, condition=True, oversample=ov, depth=depth)
                   if s in seats else piers[s] for s in range(2)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = ev.run(players)
        torch.cuda.synchronize()
        seconds = time.perf_counter() - t0
        sps = [p for p in players if isinstance(p, SearchPlayer)]
        tot = lambda k: sum(getattr(p, k) for p in sps)
        mv, cn, K = tot("moves"), tot("conditioned"), 32 * ov
        row = dict(seats=list(seats), oversample=ov, depth=depth, mean=r.mean, stderr=r.stderr, moves=mv, deviations=tot("deviations"),
                   deviation_rate=tot("deviations") / max(mv, 1), conditioned=cn, fallback_share=tot("fallbacks") / max(cn, 1),
                   mean_depth_used=tot("depth_used") / max(cn, 1), rollouts=tot("rollouts"), dead_replicas=tot("dead_replicas"),
                   seconds=seconds)
        if depth == 1:
            row["survivor_share"] = [tot("survivors") / max(tot("candidates"), 1)]
            row["shallow_share"] = row["fallback_share"]
        else:
            st = [p.depth_stats() for p in sps]
            reached = [sum(s["reached"][d] for s in st) for d in range(depth)]
            row["reached"] = reached
            row["used"] = [sum(s["used"][d] for s in st) for d in range(depth)]
            row["survivor_share"] = [sum(s["survivors"][d] for s in st) / max(reached[d] * K, 1) for d in range(depth)]
            row["shallow_share"] = sum(sum(s["shallow"]) for s in st) / max(cn, 1)
        out["rows"][label] = row
        print(json.dumps({label: row}), flush=True)
        del players, sps
        torch.cuda.empty_cache()
    ref_path = os.path.join(ROOT, "profiles", "search", "belief_probe.json")
    if os.path.exists(ref_path) and args.games == 1024:
        ref = json.load(open(ref_path))["rows"]
        same = {k: out["rows"][k]["mean"] == ref[v]["mean"] for k, v in SAME_AS.items() if v in ref}
        out["depth_1_reproduces_belief_probe"] = same
        print(json.dumps({"depth_1_reproduces_belief_probe": same}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
