"""Cost of the partner-response counts (responses=True: one hb_eval_response_tally per turn) on one MI355X.
Evaluator(n_games=32768).run([Piers, Piers]) and the 8-agent CrossPlay(n_games=4096) of the README (4 untrained bf16 DQN agents
+ Flawed / IGGI / Outer / Piers, 64 teams), each with the switch off and on in the same process: a warm-up run of both, then
the two alternated, best of 3 each (host clock around a run that ends in a device synchronise). Also event-times the new launch
alone at both shapes, and checks that the switch changes no score.
Usage: response_probe.py [out.json]   (default profiles/eval/response_probe.json)"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hanabi-agents_amd")]

import torch  # noqa: E402

import hanabi_hip  # noqa: E402
from hanabi_agents.rlax_dqn import ActionSpec, DQNAgent, ObservationSpec, RlaxRainbowParams  # noqa: E402
from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR  # noqa: E402
from hanabi_hip import CrossPlay, Evaluator, _capi as K  # noqa: E402

REPS = 3


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1000, out


def pair(off, on):
    """Warm both, then alternate them: best-of-REPS ms of each, and the last results."""
    off(), on()
    ms = dict(off=[], on=[])
    res = {}
    for _ in range(REPS):
        for name, fn in (("off", off), ("on", on)):
            t, res[name] = timed(fn)
            ms[name].append(t)
    return {k: round(min(v), 3) for k, v in ms.items()}, {k: [round(x, 3) for x in v] for k, v in ms.items()}, res


def launch_us(cfg, nb, bg, live_fraction=0.5, iters=200):
    """Event-timed us per hb_eval_response_tally(_grouped) launch, back to back, on random moves with `live_fraction` of the
    games live (a floor: the launches of a run sit between other kernels)."""
    L = K.lib()
    A = L.hb_num_actions(C.byref(cfg))
    n = nb * bg
    g = torch.Generator(device="cuda").manual_seed(1)
    act = torch.randint(0, A, (n,), dtype=torch.int32, device="cuda", generator=g)
    done = (torch.rand(n, device="cuda", generator=g) >= live_fraction).to(torch.uint8) * 0x80
    prev = torch.randint(-1, A, (n,), dtype=torch.int32, device="cuda", generator=g)
    resp = torch.zeros(nb, cfg.players, A + 1, A, dtype=torch.int64, device="cuda")

    def call():
        K.check(L.hb_eval_response_tally_grouped(C.byref(cfg), nb, bg, 0, K.dptr(act), K.dptr(done), K.dptr(prev), K.dptr(resp),
                                                 K.current_stream()))
    for _ in range(10):
        call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        call()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) * 1000 / iters, 2)


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "eval", "response_probe.json")
    out = {}
    # Evaluator, 32 768 two-player games, Piers / Piers
    team = [RulebasedAgent(PR.piers_rules, seed=1), RulebasedAgent(PR.piers_rules, seed=2)]
    ev = {k: Evaluator("Hanabi-Full", 2, n_games=32768, seed=7, responses=k == "on") for k in ("off", "on")}
    best, runs, res = pair(lambda: ev["off"].run(team), lambda: ev["on"].run(team))
    out["evaluator"] = dict(n_games=32768, team="Piers/Piers", turns=res["on"].turns, ms_best=best, ms_runs=runs,
                            overhead_pct=round(100 * (best["on"] / best["off"] - 1), 2),
                            scores_equal=bool(torch.equal(res["on"].scores, res["off"].scores)),
                            counted=int(res["on"].responses.sum()), moves=int(res["on"].moves.sum()),
                            launch_us=launch_us(ev["on"].cfg, 1, 32768))
    print(json.dumps(out["evaluator"]), flush=True)
    # CrossPlay, the README's pool: 64 teams of 4 096 games
    probe = hanabi_hip.HanabiEnv("Hanabi-Full", 2, n_games=1, auto_reset=False, packed=True)
    pool = []
    for s in range(1, 5):
        params = RlaxRainbowParams(compute_dtype="bfloat16", packed_obs=True, layers=[512], experience_buffer_size=1024, seed=s)
        pool.append(DQNAgent(ObservationSpec((1, probe.obs_len)), ActionSpec(probe.num_actions), params, device="cuda"))
    pool += [RulebasedAgent(r) for r in (PR.flawed_rules, PR.iggi_rules, PR.outer_rules, PR.piers_rules)]
    cp = {k: CrossPlay("Hanabi-Full", 2, n_games=4096, seed=7, responses=k == "on") for k in ("off", "on")}
    best, runs, res = pair(lambda: cp["off"].run(pool), lambda: cp["on"].run(pool))
    d = res["on"].convention_distance()
    out["crossplay"] = dict(n_games=4096, pool=len(pool), teams=len(res["on"].teams), turns=cp["on"].last_turns, ms_best=best,
                            ms_runs=runs, overhead_pct=round(100 * (best["on"] / best["off"] - 1), 2),
                            means_equal=bool(torch.equal(res["on"].mean_matrix(), res["off"].mean_matrix())),
                            launch_us=launch_us(cp["on"].cfg, 64, 4096),
                            distance_self_teams=[[round(float(d[9 * i, 9 * j]), 4) for j in range(8)] for i in range(8)])
    print(json.dumps({k: v for k, v in out["crossplay"].items() if k != "distance_self_teams"}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
