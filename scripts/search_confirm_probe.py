"""Effect of a standard-error test and of a confirming second stage on belief-sampled rollout search (hanabi_hip.search,
DESIGN.md section 11f) on one MI355X: Evaluator(n_games=1024, seed=7), blueprint [Piers, Piers], search seed 9, threshold 0 — the
setting of scripts/search_probe.py's effect table, whose rows (blueprint; plain search at 32 and 128 replicas) are re-measured
in the same run. Added: z in {1, 2, 3} on the search's own 32 replicas; 32 replicas screening + 256 fresh replicas confirming
{blueprint move, challenger} with z in {0, 2}; 128 replicas with z = 2. Each for one seat searching and for both.
Writes one JSON file.
Usage: search_confirm_probe.py [--out profiles/search/confirm_probe.json] [--games 1024]"""
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

SETTINGS = [   # (label, replicas, z, confirm_replicas)
    ("plain_r32", 32, None, 0),
    ("z1_r32", 32, 1.0, 0),
    ("z2_r32", 32, 2.0, 0),
    ("z3_r32", 32, 3.0, 0),
    ("confirm256_z0_r32", 32, 0.0, 256),
    ("confirm256_z2_r32", 32, 2.0, 256),
    ("plain_r128", 128, None, 0),
    ("z2_r128", 128, 2.0, 0),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search", "confirm_probe.json"))
    ap.add_argument("--games", type=int, default=1024)
    args = ap.parse_args()
    out = dict(device=torch.cuda.get_device_name(0), setting=dict(game="Hanabi-Full", players=2, n_games=args.games, eval_seed=7,
                                                                 blueprint="[Piers, Piers]", search_seed=9, threshold=0.0), rows={})
    piers = [RulebasedAgent(PR.piers_rules, seed=1), RulebasedAgent(PR.piers_rules, seed=2)]
    ev = Evaluator("Hanabi-Full", 2, n_games=args.games, seed=7)
    base = ev.run(piers)
    out["rows"]["blueprint"] = dict(mean=base.mean, stderr=base.stderr, perfect_rate=base.perfect_rate, bombout_rate=base.bombout_rate)
    print(json.dumps({"blueprint": out["rows"]["blueprint"]}), flush=True)
    for label, reps, z, confirm in SETTINGS:
        for who, seats in (("seat0", (0,)), ("both", (0, 1))):
            players = [SearchPlayer(piers, s, replicas=reps, threshold=0.0, seed=9, z=z, confirm_replicas=confirm) if s in seats else piers[s]
                       for s in range(2)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = ev.run(players)
            torch.cuda.synchronize()
            seconds = time.perf_counter() - t0
            sps = [p for p in players if isinstance(p, SearchPlayer)]
            mv, dv = sum(p.moves for p in sps), sum(p.deviations for p in sps)
            cf, rj = sum(p.confirmed for p in sps), sum(p.rejected for p in sps)
            row = dict(replicas=reps, z=z, confirm_replicas=confirm, seats=list(seats), mean=r.mean, stderr=r.stderr,
                       perfect_rate=r.perfect_rate, bombout_rate=r.bombout_rate, moves=mv, deviations=dv, deviation_rate=dv / max(mv, 1),
                       confirmed=cf, rejected=rj, rejected_share=(rj / cf if cf else None), rollouts=sum(p.rollouts for p in sps),
                       dead_replicas=sum(p.dead_replicas for p in sps), seconds=seconds)
            out["rows"][f"{label}_{who}"] = row
            print(json.dumps({f"{label}_{who}": row}), flush=True)
            del players, sps
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
