"""Training against a partner pool (hanabi_hip.partner_pool) on one MI355X: 2-player Hanabi-Full, 32 768 games, bf16, packed, one
update per step. Reports the step time (ms per env step, every seat's step counted) of self-play [dqn, dqn], of [dqn, Piers] and
of [dqn, pool(Flawed, IGGI, Outer, Piers, 2 frozen bf16 DQN)], then the per-launch split of one pool turn (the grouped actor, the
rule launch) and the training tally alone, from events around each launch (us per launch, mean over repeats).
Usage: pool_probe.py [steps] [out.json]   (default 600 steps, profiles/partner_pool/pool_probe.json)"""
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
from hanabi_hip import PartnerPool, _capi as K  # noqa: E402
from hanabi_hip.selfplay import SelfPlaySession  # noqa: E402

N = 32768


def env_():
    flags = hanabi_hip.FLAG_AUTO_RESET | hanabi_hip.FLAG_RESET_START_NEXT
    return hanabi_hip.HanabiEnv(config=hanabi_hip.make_config("Hanabi-Full", 2, flags), n_games=N, seed=5, packed=True)


def dqn(env, seed, rows=N):
    params = RlaxRainbowParams(train_batch_size=256, experience_buffer_size=N * 8, mask_terminal=True, compute_dtype="bfloat16",
                               packed_obs=True, layers=[512], seed=seed)
    return DQNAgent(ObservationSpec((rows, env.obs_len)), ActionSpec(env.num_actions), params, device="cuda")


def timed(sess, steps):
    sess.run(200)   # warm-up: replay past min_replay, graphs captured, command arrays built
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sess.run(steps)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def launch_split(sess, pool, reps=200):
    """us per launch of the pool turn's parts and of the tally, on the session's env as it stands."""
    env, L = sess.env, K.lib()
    tab = pool.move_table(env)
    act = torch.zeros(env.n, dtype=torch.int32, device="cuda")
    q = torch.empty(env.n, env.num_actions, dtype=torch.float32, device="cuda")
    st = K.current_stream()
    parts = {
        "grouped_actor": lambda: tab.launch_tiles(env, 1, 9, act, q),
        "rule_blocks": lambda: tab.launch_rules(env, 1, 9, env.first_game_id, act),
    }
    out = {}
    for name, fn in parts.items():
        fn()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(reps):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        out[name] = ev[0].elapsed_time(ev[1]) * 1e3 / reps
    # the tally alone, on the last step's outputs, into scratch counters (the pool's own are left as they are)
    cnt = torch.zeros_like(pool.counters)
    lost, length = pool._lost.clone(), pool._length.clone()
    fn = lambda: K.check(L.hb_train_tally(C.byref(env.cfg), env.n, 0, K.dptr(act), K.dptr(env.reward), K.dptr(env.terminal),
                                          K.dptr(env.score), K.dptr(pool._tile_member), len(pool.members), K.dptr(lost),
                                          K.dptr(length), K.dptr(cnt), st))
    fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    out["train_tally"] = ev[0].elapsed_time(ev[1]) * 1e3 / reps
    return out


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 600
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "partner_pool", "pool_probe.json")
    res = dict(game="Hanabi-Full", players=2, games=N, dtype="bfloat16", packed=True, steps=steps)
    torch.manual_seed(0)
    env = env_()
    s = SelfPlaySession(env, [dqn(env, 1), dqn(env, 2)])
    res["selfplay_ms_per_step"] = timed(s, steps)
    del s, env
    env = env_()
    s = SelfPlaySession(env, [dqn(env, 1), RulebasedAgent(PR.piers_rules)], train_seats=[0])
    res["vs_piers_ms_per_step"] = timed(s, steps)
    res["vs_piers_native_steps"] = s.native_steps
    del s, env
    env = env_()
    frozen = [dqn(env, 7, rows=1), dqn(env, 8, rows=1)]
    pool = PartnerPool([RulebasedAgent(r) for r in (PR.flawed_rules, PR.iggi_rules, PR.outer_rules, PR.piers_rules)] + frozen)
    s = SelfPlaySession(env, [dqn(env, 1), pool], train_seats=[0])
    res["vs_pool_ms_per_step"] = timed(s, steps)
    res["vs_pool_native_steps"] = s.native_steps
    res["pool_turn_us"] = launch_split(s, pool)
    res["pool_stats"] = [x.as_dict() for x in pool.stats()]
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "pool_stats"}))


if __name__ == "__main__":
    main()
