"""CrossPlay.run (hanabi_hip.crossplay) against the Evaluator loop it replaces, on one MI355X. Pool: 4 untrained bf16 DQN agents
(seeds 1-4) + Flawed / IGGI / Outer / Piers, every default team (64); 2 players at 4 096 games per team and 5 players at 1 024.
Reports ms per grouped run, ms per loop of Evaluator.run over the same teams (one Evaluator, as a user would write it), the
speed-up, turns, and the grouped run's per-turn split (actor / rule / env / tally, from events around each phase of every turn).
Untrained agents: the speed does not depend on the weights; the game lengths do. Every configuration runs in a child process of
its own under `timeout -k 10 300`; the probe stops at the first failing one.
Usage: crossplay_probe.py [out.json]   (default profiles/crossplay/crossplay_probe.json)"""
import ctypes as C
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
from hanabi_hip import CrossPlay, Evaluator, _capi as K  # noqa: E402


def make_pool(players):
    probe = hanabi_hip.HanabiEnv("Hanabi-Full", players, n_games=1, auto_reset=False, packed=True)
    pool = []
    for s in range(1, 5):
        params = RlaxRainbowParams(compute_dtype="bfloat16", packed_obs=True, layers=[512], experience_buffer_size=1024, seed=s)
        pool.append(DQNAgent(ObservationSpec((1, probe.obs_len)), ActionSpec(probe.num_actions), params, device="cuda"))
    return pool + [RulebasedAgent(r) for r in (PR.flawed_rules, PR.iggi_rules, PR.outer_rules, PR.piers_rules)]


def split(cp, pool):
    """One instrumented grouped run (one chunk): events around each turn's phases, summed over the turns; us per turn."""
    teams = hanabi_hip.crossplay.default_teams(len(pool), cp.players)
    (first, nb), = cp.chunks(len(teams))
    ch = cp._chunk(nb)
    env, L = ch.env, K.lib()
    kinds, rule_sets = cp.classify_pool(pool)
    rule_sets.upload(env.device)
    tables = [cp.seat_table(ch, [pool[t[s]] for t in teams], kinds, rule_sets) for s in range(cp.players)]
    env.import_state(ch.rows0)
    env.observe()
    ch.done.copy_(ch.done0); ch.final_score.zero_(); ch.length.zero_(); ch.counters.copy_(ch.counters0)
    bufs = tuple(K.dptr(x) for x in (env.reward, env.terminal, env.score, ch.done, ch.final_score, ch.length, ch.counters))
    ms = dict(actor=0.0, rule=0.0, env=0.0, tally=0.0)
    live = []
    act = ch.actions[0]
    for t in range(cp.max_turns):
        tab = tables[t % cp.players]
        e = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        st = K.current_stream()
        e[0].record()
        tab.launch_tiles(env, cp.seed, t + 1, act, ch.q)
        e[1].record()
        tab.launch_rules(env, cp.seed, t + 1, cp.first_game_id, act)
        e[2].record()
        env.step(act)
        e[3].record()
        K.check(L.hb_eval_tally_grouped(C.byref(cp.cfg), nb, cp.n_pad, t % cp.players, t, K.dptr(act), *bufs, st))
        e[4].record()
        torch.cuda.synchronize()
        for k, (i, j) in zip(ms, ((0, 1), (1, 2), (2, 3), (3, 4))):
            ms[k] += e[i].elapsed_time(e[j])
        live.append(int(ch.counters[:, 0].sum().item()))
        if live[-1] == 0:
            break
    turns = len(live)
    return {k: round(v * 1000 / turns, 2) for k, v in ms.items()}, turns


def one(players, n):
    pool = make_pool(players)
    teams = hanabi_hip.crossplay.default_teams(len(pool), players)
    cp = CrossPlay("Hanabi-Full", players, n_games=n, seed=1)
    res = cp.run(pool)   # warm-up (learners, packs, the chunk's env and buffers)
    torch.cuda.synchronize()
    reps = 3
    t0 = time.perf_counter()
    for _ in range(reps):
        res = cp.run(pool)
    torch.cuda.synchronize()
    grouped_ms = (time.perf_counter() - t0) * 1000 / reps
    ev = Evaluator("Hanabi-Full", players, n_games=n, seed=1)
    loop = lambda: [ev.run([pool[i] for i in t]) for t in teams]
    want = loop()        # warm-up, and the reference results
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        loop()
    torch.cuda.synchronize()
    loop_ms = (time.perf_counter() - t0) * 1000 / reps
    same = all(torch.equal(a.scores, b.scores) and torch.equal(a.lengths, b.lengths) and torch.equal(a.moves, b.moves)
               for a, b in zip(res.results, want))
    us, turns = split(cp, pool)
    return dict(players=players, n_games=n, n_pad=cp.n_pad, pool=len(pool), teams=len(teams), rows=len(teams) * cp.n_pad,
                grouped_ms=round(grouped_ms, 3), evaluator_loop_ms=round(loop_ms, 3), speedup=round(loop_ms / grouped_ms, 2),
                grouped_turns=cp.last_turns, split_turns=turns, us_per_turn=us, results_equal=same,
                mean_matrix=[[round(x, 4) for x in row] for row in res.mean_matrix().tolist()])


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        print(json.dumps(one(int(sys.argv[2]), int(sys.argv[3]))))
        return
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "crossplay", "crossplay_probe.json")
    out = []
    for players, n in ((2, 4096), (5, 1024)):
        p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--one", str(players), str(n)],
                           capture_output=True, text=True)
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-4000:])
            sys.exit(f"crossplay_probe: {players}p {n} failed with exit status {p.returncode}")
        row = json.loads(p.stdout.strip().splitlines()[-1])
        out.append(row)
        print(json.dumps({k: v for k, v in row.items() if k != "mean_matrix"}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
