"""Evaluator.run (hanabi_hip.evaluate) on one MI355X: ms per evaluation, turns played, the per-turn split between the agents'
moves, the env step and the tally kernel, and the fraction of games still live per turn (for a later decision on compacting
finished games out of the forward pass). Untrained agents (the speed does not depend on the weights; the game lengths do).
Every configuration runs in a child process of its own under `timeout` (120 s); the probe stops at the first failing one.
Usage: eval_probe.py [out.json]"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hanabi-agents_amd")]

import torch  # noqa: E402

import hanabi_hip  # noqa: E402
from hanabi_agents.rlax_dqn import ActionSpec, DQNAgent, ObservationSpec, RlaxRainbowParams  # noqa: E402
from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR  # noqa: E402
from hanabi_hip import Evaluator, _capi as K  # noqa: E402


def team(kind, players, env):
    params = RlaxRainbowParams(compute_dtype="bfloat16", packed_obs=True, layers=[512], experience_buffer_size=1024)
    dqn = DQNAgent(ObservationSpec((1, env.obs_len)), ActionSpec(env.num_actions), params, device="cuda")
    piers = RulebasedAgent(PR.piers_rules)
    return [dqn if (kind == "dqn_dqn" or s % 2 == 0) else piers for s in range(players)]


def split(ev, agents):
    """One instrumented run: events around each turn's three phases, the live count read every turn."""
    env, L = ev.env, K.lib()
    env.import_state(ev.rows0)
    env.observe()
    ev.done.zero_(); ev.final_score.zero_(); ev.length.zero_(); ev.counters.zero_(); ev.counters[0] = ev.n
    bufs = tuple(K.dptr(t) for t in (env.reward, env.terminal, env.score, ev.done, ev.final_score, ev.length, ev.counters))
    ms = dict(moves=0.0, env=0.0, tally=0.0)
    live = []
    act = ev.actions[0]
    scratch = {}
    import ctypes as C
    for t in range(ev.max_turns):
        a = agents[t % ev.players]
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record()
        if a.requires_vectorized_observation():
            a.eval_moves((env, (env.net_obs, env.legal)), ev.seed, t + 1, act, scratch=scratch.setdefault(a, {}))
        else:
            a.eval_moves(env, ev.seed, t + 1, act)
        e[1].record()
        env.step(act)
        e[2].record()
        K.check(L.hb_eval_tally(C.byref(ev.cfg), ev.n, t % ev.players, t, K.dptr(act), *bufs, K.current_stream()))
        e[3].record()
        torch.cuda.synchronize()
        ms["moves"] += e[0].elapsed_time(e[1]); ms["env"] += e[1].elapsed_time(e[2]); ms["tally"] += e[2].elapsed_time(e[3])
        live.append(int(ev.counters[0].item()) / ev.n)
        if live[-1] == 0:
            break
    turns = len(live)
    return {k: v * 1000 / turns for k, v in ms.items()}, live


def one(players, n, kind):
    ev = Evaluator("Hanabi-Full", players, n_games=n, seed=1)
    ev._setup()
    agents = team(kind, players, ev.env)
    ev.run(agents)   # warm-up (packs, allocations)
    torch.cuda.synchronize()
    reps = 5
    t0 = time.perf_counter()
    for _ in range(reps):
        r = ev.run(agents)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1000 / reps
    us, live = split(ev, agents)
    return dict(players=players, n_games=n, team=kind, ms_per_eval=round(ms, 3), turns=r.turns, longest_game=int(r.lengths.max()),
                mean_score=r.mean, us_per_turn={k: round(v, 2) for k, v in us.items()}, live_fraction=[round(x, 4) for x in live])


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        print(json.dumps(one(int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])))
        return
    out = []
    for players in (2, 5):
        for n in (4096, 32768):
            for kind in ("dqn_dqn", "dqn_piers"):
                p = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__), "--one", str(players), str(n),
                                    kind], capture_output=True, text=True)
                if p.returncode != 0:
                    sys.stderr.write(p.stderr[-4000:])
                    sys.exit(f"eval_probe: {players}p {n} {kind} failed with exit status {p.returncode}")
                row = json.loads(p.stdout.strip().splitlines()[-1])
                out.append(row)
                print(json.dumps({k: v for k, v in row.items() if k != "live_fraction"}), flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
