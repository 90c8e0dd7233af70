"""Cost of colour-permuted frames on one MI355X.
  env:     the env kernel alone (hb_env_step_packed, dispatch timestamps via hb_env_set_profile_events), plain against shuffled,
           32 768 games of Hanabi-Full with 2 and 5 players, packed rows, random legal moves; median us per launch.
  session: SelfPlaySession step time (2-player Hanabi-Full, 32 768 games, two bf16 DQN agents), default env against an env with
           every seat shuffled (which takes the policy launch + selection-fused env step instead of the one-launch actor),
           three alternating runs each; ms per step.
Every measurement runs in a child process of its own under `timeout -k 10 600`; the probe stops at the first failing one.
Usage: color_shuffle_probe.py [out.json]   (default profiles/color_shuffle/probe.json)"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hanabi-agents_amd")]


def env_kernel(players, shuffled, steps=300, warm=50):
    import torch

    import hanabi_hip

    flags = hanabi_hip.FLAG_AUTO_RESET | hanabi_hip.FLAG_RESET_START_NEXT
    env = hanabi_hip.HanabiEnv(config=hanabi_hip.make_config("Hanabi-Full", players, flags), n_games=32768, seed=1, packed=True,
                               color_shuffle=shuffled)
    acts = [env.random_legal_actions(seed=2, draw=t) for t in range(1)]
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record(); e.record()
    env.set_profile_events(s, e)
    us = []
    for t in range(steps + warm):
        a = env.random_legal_actions(seed=2, draw=t, out=acts[0])
        env.step(a)
        e.synchronize()
        if t >= warm:
            us.append(s.elapsed_time(e) * 1e3)
    env.set_profile_events()
    assert env.illegal_count() == 0
    us.sort()
    return dict(median_us=us[len(us) // 2], p10_us=us[len(us) // 10], p90_us=us[9 * len(us) // 10])


def session(shuffled, steps=300, warm=100):
    import torch

    import hanabi_hip
    from hanabi_agents.rlax_dqn import ActionSpec, DQNAgent, ObservationSpec, RlaxRainbowParams
    from hanabi_hip.selfplay import SelfPlaySession

    n = 32768
    flags = hanabi_hip.FLAG_AUTO_RESET | hanabi_hip.FLAG_RESET_START_NEXT
    env = hanabi_hip.HanabiEnv(config=hanabi_hip.make_config("Hanabi-Full", 2, flags), n_games=n, seed=1, packed=True,
                               color_shuffle=shuffled)
    params = RlaxRainbowParams(compute_dtype="bfloat16", packed_obs=True, experience_buffer_size=2 ** 20)
    agents = [DQNAgent(ObservationSpec((n, env.obs_len)), ActionSpec(env.num_actions), params._replace(seed=s), device="cuda")
              for s in (1, 2)]
    sess = SelfPlaySession(env, agents)
    sess.run(warm)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sess.run(steps)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    assert env.illegal_count() == 0
    return dict(ms_per_step=ms, fused_env_step=bool(sess.fuse_env_step), native_steps=sess.native_steps)


def child(spec):
    out = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.abspath(__file__), "--child", json.dumps(spec)],
                         capture_output=True, text=True)
    if out.returncode != 0:
        sys.stderr.write(out.stdout + out.stderr)
        raise SystemExit(f"child {spec} failed with exit status {out.returncode}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        spec = json.loads(sys.argv[2])
        fn = env_kernel if spec.pop("what") == "env" else session
        print(json.dumps(fn(**spec)))
        return
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "color_shuffle", "probe.json")
    res = dict(env_kernel={}, session=dict(default=[], shuffled=[]))
    for players in (2, 5):
        for shuffled in (False, True):
            r = child(dict(what="env", players=players, shuffled=shuffled))
            res["env_kernel"][f"{players}p_{'shuffled' if shuffled else 'plain'}"] = r
            print(players, shuffled, r, flush=True)
    for _ in range(3):
        for shuffled in (False, True):
            r = child(dict(what="session", shuffled=shuffled))
            res["session"]["shuffled" if shuffled else "default"].append(r)
            print("session", shuffled, r, flush=True)
    med = lambda v: sorted(x["ms_per_step"] for x in v)[len(v) // 2]
    res["session"]["median_ms"] = dict(default=med(res["session"]["default"]), shuffled=med(res["session"]["shuffled"]))
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["session"]["median_ms"]))


if __name__ == "__main__":
    main()
