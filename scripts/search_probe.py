"""Cost and effect of belief-sampled rollout search (hanabi_hip.search) on one MI355X.

Cost: hb_belief_determinize alone for 1 024 roots x 32 replicas (Full, 2 players); a whole RolloutSearch.run for the same roots x
20 actions (655 360 rollout games) with [Piers, Piers] and with a bf16 DQN blueprint, next to Evaluator.run on the same number
of games with the same team. Effect: Evaluator(n_games=1024, seed=7) for [Piers, Piers], search on seat 0, and search on both
seats, with 32 and 128 replicas. Writes one JSON file.
Usage: search_probe.py [--out profiles/search/search_probe.json] [--skip-effect] [--replicas 32,128]"""
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

import hanabi_hip  # noqa: E402
from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR  # noqa: E402
from hanabi_hip import Determinizer, Evaluator, RolloutSearch, SearchPlayer  # noqa: E402


def timed(fn, reps=3):
    """Wall-clock milliseconds of fn() (synchronised), best and median of `reps` after one warm-up call."""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return dict(best_ms=ts[0], median_ms=ts[len(ts) // 2], reps=reps)


def dqn(env_like, seed):
    from hanabi_agents.rlax_dqn import ActionSpec, DQNAgent, ObservationSpec, RlaxRainbowParams

    params = RlaxRainbowParams(train_batch_size=128, experience_buffer_size=8192, compute_dtype="bfloat16", packed_obs=True,
                               layers=[512], seed=seed)
    return DQNAgent(ObservationSpec((1, env_like.obs_len)), ActionSpec(env_like.num_actions), params, device="cuda")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search", "search_probe.json"))
    ap.add_argument("--skip-effect", action="store_true")
    ap.add_argument("--replicas", default="32,128")
    args = ap.parse_args()
    out = dict(device=torch.cuda.get_device_name(0), cost={}, effect={})
    m, R, A = 1024, 32, 20
    src = hanabi_hip.HanabiEnv("Hanabi-Full", 2, n_games=m, seed=3, auto_reset=False, packed=True)
    piers = [RulebasedAgent(PR.piers_rules, seed=1), RulebasedAgent(PR.piers_rules, seed=2)]
    for t in range(10):   # ten turns of Piers: hints given, every game still running or nearly so
        act = torch.empty(m, dtype=torch.int32, device="cuda")
        piers[t % 2].eval_moves(src, 5, t + 1, act)
        src.step(act)
    rows, legal = src.export_state(), src.legal.clone()
    det = Determinizer("Hanabi-Full", 2)
    bufs = (torch.empty((m * R, det.state_words), dtype=torch.int32, device="cuda"), torch.empty(m * R, dtype=torch.int32, device="cuda"))

    def det_many():
        for _ in range(100):
            det.sample(rows, replicas=R, seed=1, draw=1, out=bufs)

    c = timed(det_many)
    out["cost"]["determinize_1024x32_us"] = dict(best=c["best_ms"] * 10, median=c["median_ms"] * 10, note="100 back-to-back launches / 100")
    teams = dict(piers_piers=piers, dqn_dqn=[dqn(src, 1), dqn(src, 2)])
    for name, team in teams.items():
        rs = RolloutSearch("Hanabi-Full", 2, replicas=R, seed=1)
        res = rs.run(rows, legal, team, draw=1)
        c = timed(lambda: rs.run(rows, legal, team, draw=1))
        c.update(rollouts=res.rollouts, turns=res.turns, games_in_env=m * A * R, dead=res.dead)
        out["cost"][f"rollout_search_{name}"] = c
        del rs
        torch.cuda.empty_cache()
        ev = Evaluator("Hanabi-Full", 2, n_games=m * A * R, seed=1)
        r = ev.run(team)
        c = timed(lambda: ev.run(team))
        c.update(turns=r.turns, mean=r.mean)
        out["cost"][f"evaluator_same_games_{name}"] = c
        del ev
        torch.cuda.empty_cache()
    if not args.skip_effect:
        ev = Evaluator("Hanabi-Full", 2, n_games=1024, seed=7)
        base = ev.run(piers)
        out["effect"]["piers_piers"] = dict(mean=base.mean, stderr=base.stderr, perfect_rate=base.perfect_rate, bombout_rate=base.bombout_rate)
        for reps in [int(x) for x in args.replicas.split(",")]:
            for label, seats in (("seat0", (0,)), ("both", (0, 1))):
                players = [SearchPlayer(piers, s, replicas=reps, threshold=0.0, seed=9) if s in seats else piers[s] for s in range(2)]
                t0 = time.perf_counter()
                r = ev.run(players)
                sps = [p for p in players if isinstance(p, SearchPlayer)]
                mv, dv = sum(p.moves for p in sps), sum(p.deviations for p in sps)
                out["effect"][f"search_{label}_replicas{reps}"] = dict(
                    mean=r.mean, stderr=r.stderr, perfect_rate=r.perfect_rate, bombout_rate=r.bombout_rate, moves=mv, deviations=dv,
                    deviation_rate=dv / max(mv, 1), dead_replica_share=sum(p.dead_replicas for p in sps) / max(sum(p.replicas_drawn for p in sps), 1),
                    seconds=time.perf_counter() - t0)
                print(json.dumps({f"search_{label}_replicas{reps}": out["effect"][f"search_{label}_replicas{reps}"]}), flush=True)
                del players, sps
                torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
