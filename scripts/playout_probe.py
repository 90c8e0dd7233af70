"""What playout=True (rule-list teams played to the end by one hb_rule_playout launch instead of the per-turn loop) is worth on
one MI355X. Four workloads, each with the switch off (the loop) and on in the same process: a warm-up run of both, then the two
alternated, best of 3 each (host clock around a run that ends in a device synchronise); every run is printed.
  * Evaluator(n_games=32768).run([Piers, Piers]), and the same at 655 360 games;
  * RolloutSearch over 1 024 roots x 20 actions x 32 replicas, [Piers, Piers], roots ten turns into a game;
  * one SearchPlayer([Piers, Piers], replicas=32) evaluation of 1 024 games.
Also event-times the kernel alone at both evaluator sizes, on the deals as they are and on waves whose 64 lanes hold copies of one
deal (lanes that take the same branches: what the divergence between a wave's games costs), and checks that the switch changes
no score.
Usage: playout_probe.py [out.json]   (default profiles/playout/playout_probe.json)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hanabi-agents_amd")]

import torch  # noqa: E402

import hanabi_hip  # noqa: E402
from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR  # noqa: E402
from hanabi_hip import Evaluator, RolloutSearch, SearchPlayer  # noqa: E402

REPS = 3


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1000, out


def pair(off, on):
    """Warm both, then alternate them: best-of-REPS ms of each, every run, and the last results."""
    off(), on()
    ms = dict(off=[], on=[])
    res = {}
    for _ in range(REPS):
        for name, fn in (("off", off), ("on", on)):
            t, res[name] = timed(fn)
            ms[name].append(t)
    best = {k: round(min(v), 3) for k, v in ms.items()}
    best["ratio"] = round(best["off"] / best["on"], 2)
    best["spread_on_pct"] = round(100 * (max(ms["on"]) / min(ms["on"]) - 1), 1)
    return best, {k: [round(x, 3) for x in v] for k, v in ms.items()}, res


def kernel_ms(ev, rows0, team, seed, iters=5):
    """Event-timed ms of hb_rule_playout alone (its buffers prepared outside the timed span), best of `iters`."""
    cfg, n = ev.cfg, rows0.shape[0]
    rows = torch.empty_like(rows0)
    out = (torch.empty(n, dtype=torch.int8, device="cuda"), torch.empty(n, dtype=torch.int16, device="cuda"),
           torch.empty(ev.n_counters, dtype=torch.int64, device="cuda"))
    done = torch.empty(n, dtype=torch.uint8, device="cuda")
    best = float("inf")
    for _ in range(iters + 1):
        rows.copy_(rows0)
        done.zero_()
        for t in out:
            t.zero_()
        out[2][0] = n
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = hanabi_hip.playout._launch(cfg, rows, team, seed, 0, None, ev.max_turns, 0, done, *out, None)
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1))
    return round(best, 3), int(res.max_len), int(res.counters[0])


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "playout", "playout_probe.json")
    out = {}
    team = [RulebasedAgent(PR.piers_rules, seed=1), RulebasedAgent(PR.piers_rules, seed=2)]
    for n in (32768, 655360):
        ev = {k: Evaluator("Hanabi-Full", 2, n_games=n, seed=7, playout=k == "on") for k in ("off", "on")}
        best, runs, res = pair(lambda: ev["off"].run(team), lambda: ev["on"].run(team))
        rows0 = ev["on"].rows0
        uniform = rows0[::64].repeat_interleave(64, 0)[:n].contiguous()
        k_ms, k_len, k_live = kernel_ms(ev["on"], rows0, team, 7)
        u_ms, u_len, _ = kernel_ms(ev["on"], uniform, team, 7)
        out[f"evaluator_{n}"] = dict(n_games=n, team="Piers/Piers", paths=[ev["off"].last_path, ev["on"].last_path],
                                     turns=[res["off"].turns, res["on"].turns], ms_best=best, ms_runs=runs,
                                     scores_equal=bool(torch.equal(res["on"].scores, res["off"].scores)),
                                     histogram_equal=bool(torch.equal(res["on"].histogram, res["off"].histogram)),
                                     kernel_ms=k_ms, kernel_longest_game=k_len, kernel_live_after=k_live,
                                     kernel_ms_waves_of_one_deal=u_ms, longest_game_waves_of_one_deal=u_len)
        print(json.dumps(out[f"evaluator_{n}"]), flush=True)
        del ev
        torch.cuda.empty_cache()
    # RolloutSearch: 1 024 roots ten turns into [Piers, Piers] play, every legal action, 32 replicas
    m = 1024
    env = hanabi_hip.HanabiEnv("Hanabi-Full", 2, n_games=m, seed=7, auto_reset=False, packed=True)
    act = torch.zeros(m, dtype=torch.int32, device="cuda")
    for t in range(10):
        team[t % 2].eval_moves(env, 7, t + 1, act)
        env.step(act)
    rows, legal = env.export_state(), env.legal.clone()
    rs = {k: RolloutSearch("Hanabi-Full", 2, replicas=32, seed=3, playout=k == "on") for k in ("off", "on")}
    best, runs, res = pair(lambda: rs["off"].run(rows, legal, team, draw=10), lambda: rs["on"].run(rows, legal, team, draw=10))
    same = torch.equal(torch.nan_to_num(res["on"].value, nan=-1.0), torch.nan_to_num(res["off"].value, nan=-1.0))
    out["rollout_search"] = dict(roots=m, replicas=32, rollouts=res["on"].rollouts, paths=[rs["off"].last_path, rs["on"].last_path],
                                 turns=[res["off"].turns, res["on"].turns], ms_best=best, ms_runs=runs, values_equal=bool(same),
                                 best_equal=bool(torch.equal(res["on"].best, res["off"].best)))
    print(json.dumps(out["rollout_search"]), flush=True)
    del rs
    torch.cuda.empty_cache()
    # SearchPlayer in seat 0 of an evaluation of 1 024 games
    ev = Evaluator("Hanabi-Full", 2, n_games=m, seed=7)
    sp = {k: SearchPlayer(team, 0, replicas=32, playout=k == "on") for k in ("off", "on")}
    best, runs, res = pair(lambda: ev.run([sp["off"], team[1]]), lambda: ev.run([sp["on"], team[1]]))
    out["search_player"] = dict(n_games=m, replicas=32, ms_best=best, ms_runs=runs, mean=[res["off"].mean, res["on"].mean],
                                scores_equal=bool(torch.equal(res["on"].scores, res["off"].scores)))
    print(json.dumps(out["search_player"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
