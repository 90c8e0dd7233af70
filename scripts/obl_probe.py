"""Off-belief learning (hanabi_hip.obl) on one MI355X: what the fictitious branch costs and what a short
run learns.

  step      ms per step of OffBeliefSession against SelfPlaySession (its one-call step, and its ordinary path, which is the one
            OffBeliefSession extends), 32 768 games of 2-player Hanabi-Full, bf16: each session warmed, then windows of STEPS
            steps alternated, best of REPS (host clock around a window that ends in a device synchronise);
  split     event-timed us per launch of the branch's parts at that size, back to back (a floor: in a step they sit between
            other kernels): state export, determinize, import, scratch env step, the partner's greedy forward, hb_obl_insert, and
            hb_replay_insert on the same rows for comparison;
  kernel    registers / spills / LDS of obl_insert_kernel from the compiler's resource remarks (needs hipcc, no GPU);
  learn     Hanabi-Small, 2 players: two runs (one agent per seat) each of off-belief and plain self-play for the same number of env steps,
            then greedy self-play score, cross-play between the runs (seats swapped) and convention distance (CrossPlay(responses=True)).

  level2    (--level2: this part alone, to profiles/obl/obl_level2_probe.json) off-belief learning level 2 (belief_policy =
            frozen copies of the session's own starting agents): ms per step at depth 1 and 2 with oversample 4 against the
            level-1 session and plain self-play, same size and windows as `step`; hb_belief_history_step event-timed alone
            against the torch path it replaces (own_move + push + the validity rule + last_move_uid) at 32 768 games, depth 4;
            the counters' rates; registers of the history kernel; and a short ladder on Hanabi-Small: level 1, a frozen_copy,
            level 2 from fresh agents on that copy's belief, two runs, then self-play, cross-play between the runs and
            convention distance for both levels.

  encode    (--encode-rows: this part alone, to profiles/obl/encode_rows_probe.json) the stateless encoder hb_encode_rows
            (csrc/encode_rows.hip): event-timed us per call on 4 x 32 768 rows of 2-player Hanabi-Full in ONE call against the
            loop of 4 x (import_state + observe) on a 32 768-game scratch env that it replaces, with bytes per second from the
            shapes (128 B row + 84 B packed observation + 20 B legal mask); the level-2 step (`level2`'s protocol: 32 768 games,
            oversample 4, depth 1 and 2, alternated windows, best of REPS) with ConditionedDeterminizer.stateless on and off; and
            (--sessions-in-a-row: in a fresh process, merged into the same file) four level-2 sessions built in a row on either
            path: a session's place in its process can move its step time by a factor of three, on the scratch-env path as well,
            which is why the step is timed on ONE session with the switch toggled; and
            the kernel's registers / LDS per configuration from the compiler's remarks (--resources-only: that part alone, no GPU;
            --skip-resources: everything else). Parts already in the output file are kept.

  soft      (--level2 --soft: this part alone, to profiles/obl/obl_soft_probe.json) the epsilon-aware soft likelihood filter
            (OffBeliefSession(belief_epsilon=...), hb_belief_select_soft) against the exact-match filter: `level2`'s sessions at
            depth 1 and 2 (32 768 games, oversample 4), ONE session per depth with `belief_epsilon` toggled between None and the
            training epsilon (0.1) from window to window, alternated windows, all REPS figures and their spread; the counters'
            rates and the mean effective sample size per leg (differences of the session's counters around each window);
            registers of the kernel (--resources-only: that part alone, no GPU; --skip-resources: everything else); the ladder's
            level-2 session (Hanabi-Small, 4 096 games) timed with the same toggle; and `level2`'s short ladder on Hanabi-Small
            with belief_epsilon = the training epsilon at level 2 (--skip-learn: not).
            It is a different estimator, not a speed-up: no time is gated. Parts already in the output file are kept.

Usage: obl_probe.py [out.json] [--skip-learn] [--learn-steps N] [--level2 [--soft]] [--level2-steps N]
                    [--encode-rows [--resources-only | --skip-resources]] [--sessions-in-a-row]
       (default profiles/obl/obl_probe.json; with --level2 profiles/obl/obl_level2_probe.json; with --level2 --soft
       profiles/obl/obl_soft_probe.json; with --encode-rows profiles/obl/encode_rows_probe.json)"""
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hanabi-agents_amd")]

N, STEPS, REPS, WARM = 32768, 200, 3, 80


def kernel_resources(name="obl.hip", only=None):
    """{kernel: {sgprs, vgprs, spill, scratch, lds, occupancy}} of csrc/<name> for gfx950, from -Rpass-analysis (`only`: the
    kernels whose mangled name contains it)."""
    src = os.path.join(ROOT, "hanabi-agents_amd", "csrc", name)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    try:
        p = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-c", src, "-o", os.devnull,
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=300)
    except (OSError, subprocess.TimeoutExpired) as e:
        return {"error": str(e)}
    out, cur = {}, None
    keys = {"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch", "SGPRs Spill": "sgpr_spill",
            "VGPRs Spill": "vgpr_spill", "LDS Size [bytes/block]": "lds", "Occupancy [waves/SIMD]": "occupancy"}
    for line in p.stderr.splitlines():
        m = re.search(r"remark: .*?Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark: .*?\s{2,}([A-Za-z \[\]/]+): (\d+)", line)
        if m and cur is not None and m.group(1).strip() in keys:
            cur[keys[m.group(1).strip()]] = int(m.group(2))
    if only is not None:
        out = {k: v for k, v in out.items() if only in k}
    return out or {"error": p.stderr[-400:]}


def encode_rows_probe(path, resources, measure):
    """The `encode` part; see the module docstring."""
    out = {}
    if os.path.exists(path):
        with open(path) as f:
            out = json.load(f)

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)

    if resources:
        table = {}
        for src in ("env_full.hip", "env_small.hip", "env_vsmall.hip"):
            res = kernel_resources(src)
            for name, r in res.items():
                m = re.search(r"(encode_rows_kernel|env_kernel)INS_3CfgILi(\d)ELi(\d)ELi(\d)ELi(\d)ELi(\d+)ELi(\d)EEELi(\d+)E", name)
                if not m or not isinstance(r, dict):
                    continue
                key = "players=%s colors=%s ranks=%s hand=%s G=%s" % (m.group(2), m.group(3), m.group(4), m.group(5), m.group(8))
                table.setdefault(key, {})[m.group(1)] = r
        # the encoder does a subset of the env step's work: its scratch must not exceed the env kernel's for the same configuration
        out["kernel"] = {k: dict(v["encode_rows_kernel"], env_kernel_scratch=v["env_kernel"]["scratch"])
                         for k, v in sorted(table.items()) if "encode_rows_kernel" in v and "env_kernel" in v}
        out["kernel_scratch_within_env_kernel"] = all(v["scratch"] <= v["env_kernel_scratch"] for v in out["kernel"].values())
        print(json.dumps(out["kernel"]), flush=True)
        save()
    if not measure:
        return

    import torch

    import hanabi_hip
    from hanabi_agents.rlax_dqn import ActionSpec, DQNAgent, ObservationSpec, RlaxRainbowParams
    from hanabi_hip import OffBeliefSession, encode_rows
    from hanabi_hip.obl import frozen_copy

    if not torch.cuda.is_available():
        raise SystemExit("obl_probe.py measures on the GPU: none found")

    # ---- the kernel alone against the loop it replaces ---------------------------------------------------------------------------
    slabs = 4
    env = hanabi_hip.HanabiEnv("Hanabi-Full", 2, n_games=N, seed=2, packed=True)
    for t in range(9):
        env.step(env.random_legal_actions(seed=3, draw=t))
    cfg, SW = env.cfg, env.state_words
    rows = env.export_state().repeat(slabs, 1).view(slabs, N, SW).contiguous()
    scratch = hanabi_hip.HanabiEnv(config=cfg, n_games=N, packed=True)
    obs = torch.empty((slabs * N, env.obs_words), dtype=torch.int32, device="cuda")
    legal = torch.empty((slabs * N, env.num_actions), dtype=torch.int8, device="cuda")
    flat = rows.view(slabs * N, SW)

    def loop():
        for k in range(slabs):
            scratch.import_state(rows[k])
            scratch.observe()

    # the same call over SETS distinct sets of rows and outputs in turn (SETS x 30.4 MB, more than the 256 MiB last-level cache),
    # the rows of every set from another depth of the game: nothing a call touches is left in cache from the call before
    SETS = 10
    cold = []
    for k in range(SETS):
        for t in range(3):
            env.step(env.random_legal_actions(seed=3, draw=100 + 3 * k + t))
        cold.append((env.export_state().repeat(slabs, 1).contiguous(), torch.empty_like(obs), torch.empty_like(legal)))
    turn = [0]

    def encode_cold():
        r, o, l = cold[turn[0] % SETS]
        turn[0] += 1
        encode_rows(cfg, r, out=(o, l))

    parts = dict(encode_rows=lambda: encode_rows(cfg, flat, out=(obs, legal)), import_observe_loop=loop,
                 encode_rows_one_slab=lambda: encode_rows(cfg, rows[0], out=(obs[:N], legal[:N])), encode_rows_cold=encode_cold)
    kern = {}
    for name, fn in parts.items():
        for _ in range(10):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(100):
            fn()
        e1.record()
        torch.cuda.synchronize()
        kern[name] = round(e0.elapsed_time(e1) * 10, 2)
    # the same bits, while both are here
    loop()
    same = bool(torch.equal(obs[(slabs - 1) * N:], scratch.obs_bits)) and bool(torch.equal(legal[(slabs - 1) * N:], scratch.legal))
    row_bytes = SW * 4 + env.obs_words * 4 + env.num_actions
    kern.update(rows=slabs * N, bytes_per_row=row_bytes, bytes=slabs * N * row_bytes, equal_outputs=same)
    kern["encode_rows_TBps"] = round(kern["bytes"] / kern["encode_rows"] / 1e6, 3)
    kern["encode_rows_cold_TBps"] = round(kern["bytes"] / kern["encode_rows_cold"] / 1e6, 3)
    kern["cold_sets"], kern["cold_bytes"] = SETS, SETS * kern["bytes"]
    kern["note"] = ("event time over 100 calls from Python: host-bound (one slab takes no less than four), so an upper bound on the kernel's "
                    "time; `encode_rows` re-reads and re-writes the same 30 MB, which stay in the 256 MiB last-level cache, `encode_rows_cold` "
                    "cycles over distinct buffers larger than that cache")
    kern["import_observe_loop_TBps"] = round(kern["bytes"] / kern["import_observe_loop"] / 1e6, 3)
    kern["loop_over_kernel"] = round(kern["import_observe_loop"] / kern["encode_rows"], 2)
    kern["not_slower_than_the_loop"] = kern["encode_rows"] <= kern["import_observe_loop"]
    kern["history_step_TBps"] = 3.45     # hb_belief_history_step, profiles/obl/obl_level2_probe.json (host-bound: a floor)
    kern["fraction_of_history_step_rate"] = round(kern["encode_rows_TBps"] / 3.45, 3)
    out["kernel_us"] = kern
    print(json.dumps(kern), flush=True)
    save()
    del env, scratch, rows, obs, legal, flat, cold
    torch.cuda.empty_cache()

    # ---- the level-2 step --------------------------------------------------------------------------------------------------------
    def agents_for(env, seeds):
        base = dict(train_batch_size=256, experience_buffer_size=1 << 19, layers=[512], mask_terminal=True, compute_dtype="bfloat16",
                    packed_obs=True)
        return [DQNAgent(ObservationSpec((env.n, env.obs_len)), ActionSpec(env.num_actions), RlaxRainbowParams(seed=s, **base),
                         device="cuda") for s in seeds]

    def window(sess, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            sess.step()
        sess.flush()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1000 / steps

    # `level2`'s sessions, built in its order; the two level-2 sessions run every window twice, with the determinizer's stateless
    # switch on and off: the same session, streams and buffers, and (the moves being the same bits) the same trajectory either way
    from hanabi_hip.selfplay import SelfPlaySession

    def level(depth):
        return lambda e, a: OffBeliefSession(e, a, belief_policy=[frozen_copy(x) for x in a], depth=depth, oversample=4)

    sessions = {}
    for name, make in (("selfplay", lambda e, a: SelfPlaySession(e, a)), ("off_belief_level1", lambda e, a: OffBeliefSession(e, a)),
                       ("depth1", level(1)), ("depth2", level(2))):
        env = hanabi_hip.HanabiEnv("Hanabi-Full", 2, n_games=N, seed=1, packed=True)
        sessions[name] = make(env, agents_for(env, (1, 2)))
        window(sessions[name], WARM)
    runs = [(name, None) for name in ("selfplay", "off_belief_level1")] + [(d, on) for d in ("depth1", "depth2") for on in (True, False)]
    label = lambda name, on: name if on is None else name + ("_stateless" if on else "_scratch_env")
    for name, on in runs[2:]:      # both paths warm (buffers, the partner's scratch)
        sessions[name].cdet.stateless = on
        window(sessions[name], 20)
    ms = {label(*r): [] for r in runs}
    for _ in range(REPS):
        for name, on in runs:
            if on is not None:
                sessions[name].cdet.stateless = on
            ms[label(name, on)].append(round(window(sessions[name], STEPS), 4))
    best = {k: min(v) for k, v in ms.items()}
    spread = {k: round(max(v) - min(v), 4) for k, v in ms.items()}
    step = dict(games=N, steps_per_window=STEPS, oversample=4, ms_per_step_best=best, ms_per_step_runs=ms, window_spread_ms=spread,
                estimate_saved_ms={"depth1": 0.14, "depth2": 0.29}, saved_ms={}, not_slower_within_spread={},
                belief_forwards={k: sessions[k].belief_forwards for k in ("depth1", "depth2")})
    for d in ("depth1", "depth2"):
        on, off = d + "_stateless", d + "_scratch_env"
        step["saved_ms"][d] = round(best[off] - best[on], 4)
        step["not_slower_within_spread"][d] = best[on] - best[off] <= max(spread[on], spread[off])
    out["step"] = step
    print(json.dumps(step), flush=True)
    save()


def sessions_in_a_row(path):
    """The `encode` part's look at a session's place in its process; see the module docstring. Merged into the output file."""
    import torch

    import hanabi_hip
    from hanabi_agents.rlax_dqn import ActionSpec, DQNAgent, ObservationSpec, RlaxRainbowParams
    from hanabi_hip import OffBeliefSession
    from hanabi_hip.obl import frozen_copy

    out = {}
    if os.path.exists(path):
        with open(path) as f:
            out = json.load(f)

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)

    def agents_for(env, seeds):
        base = dict(train_batch_size=256, experience_buffer_size=1 << 19, layers=[512], mask_terminal=True, compute_dtype="bfloat16",
                    packed_obs=True)
        return [DQNAgent(ObservationSpec((env.n, env.obs_len)), ActionSpec(env.num_actions), RlaxRainbowParams(seed=s, **base),
                         device="cuda") for s in seeds]

    def window(sess, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            sess.step()
        sess.flush()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1000 / steps

    def level(depth):
        return lambda e, a: OffBeliefSession(e, a, belief_policy=[frozen_copy(x) for x in a], depth=depth, oversample=4)

    # ---- what the position of a session among the sessions of a process does to it -----------------------------------------------------
    # In a process of its own (--sessions-in-a-row): the effect depends on what the process built before. Four level-2 sessions
    # built one after the other (depth 1, 1, 2, 2), all on the scratch-env path, which is the code as it was
    # before the encoder existed; then the same four with stateless on. Same configuration = same work: any difference between the
    # two sessions of a depth is the session's place in the process, not its path.
    row = {}
    for on in (False, True):
        four = []
        for depth in (1, 1, 2, 2):
            env = hanabi_hip.HanabiEnv("Hanabi-Full", 2, n_games=N, seed=1, packed=True)
            sess = level(depth)(env, agents_for(env, (1, 2)))
            sess.cdet.stateless = on
            window(sess, WARM)
            four.append(sess)
        ms4 = [[] for _ in four]
        for _ in range(2):
            for i, sess in enumerate(four):
                ms4[i].append(round(window(sess, 100), 4))
        row["stateless" if on else "scratch_env"] = {"built_%d_depth%d" % (i, d): ms4[i] for i, d in enumerate((1, 1, 2, 2))}
        del four, sess, env
        torch.cuda.empty_cache()
    out["sessions_in_a_row_ms_per_step"] = row
    print(json.dumps(row), flush=True)
    save()


def level2(path, ladder_steps, skip_learn):
    """The `level2` part; see the module docstring."""
    import torch

    import hanabi_hip
    from hanabi_agents.rlax_dqn import ActionSpec, DQNAgent, ObservationSpec, RlaxRainbowParams
    from hanabi_hip import CrossPlay, OffBeliefSession, PartnerHistory, last_move_uid
    from hanabi_hip.obl import frozen_copy
    from hanabi_hip.search import current_player, running
    from hanabi_hip.selfplay import SelfPlaySession

    if not torch.cuda.is_available():
        raise SystemExit("obl_probe.py measures on the GPU: none found")
    out = {"kernel": kernel_resources("belief.hip", only="history_step")}
    print(json.dumps(out["kernel"]), flush=True)

    def agents_for(env, seeds, **kw):
        base = dict(train_batch_size=256, experience_buffer_size=1 << 19, layers=[512], mask_terminal=True, compute_dtype="bfloat16",
                    packed_obs=True)
        base.update(kw)
        return [DQNAgent(ObservationSpec((env.n, env.obs_len)), ActionSpec(env.num_actions), RlaxRainbowParams(seed=s, **base),
                         device="cuda") for s in seeds]

    def window(sess, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            sess.step()
        sess.flush()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1000 / steps

    def rates(sess):
        c = {k: getattr(sess, k) for k in OffBeliefSession.LEVEL_COUNTERS}
        rows = max(1, c["conditioned_rows"] + c["fallback_rows"] + c["unconditioned_rows"])
        cond = max(1, c["conditioned_rows"])
        return dict(c, belief_forwards=sess.belief_forwards, steps=sess.t,
                    conditioned=round(c["conditioned_rows"] / rows, 4), fallback=round(c["fallback_rows"] / rows, 4),
                    unconditioned=round(c["unconditioned_rows"] / rows, 4), survivors_per_conditioned_row=round(c["survivors"] / cond, 3),
                    depth_used_per_conditioned_row=round(c["depth_used_sum"] / cond, 3),
                    belief_forwards_per_step=round(sess.belief_forwards / max(1, sess.t), 2))

    # ---- step time ----------------------------------------------------------------------------------------------------------
    def level(depth):
        return lambda e, a: OffBeliefSession(e, a, belief_policy=[frozen_copy(x) for x in a], depth=depth, oversample=4)

    sessions = {}
    for name, make in (("selfplay", lambda e, a: SelfPlaySession(e, a)), ("off_belief_level1", lambda e, a: OffBeliefSession(e, a)),
                       ("level2_depth1", level(1)), ("level2_depth2", level(2))):
        env = hanabi_hip.HanabiEnv("Hanabi-Full", 2, n_games=N, seed=1, packed=True)
        sessions[name] = make(env, agents_for(env, (1, 2)))
        window(sessions[name], WARM)
    ms = {k: [] for k in sessions}
    for _ in range(REPS):
        for name, sess in sessions.items():
            ms[name].append(round(window(sess, STEPS), 4))
    best = {k: min(v) for k, v in ms.items()}
    out["step"] = dict(games=N, steps_per_window=STEPS, oversample=4, ms_per_step_best=best, ms_per_step_runs=ms,
                       over_level1_ms={k: round(best[k] - best["off_belief_level1"], 4) for k in ("level2_depth1", "level2_depth2")},
                       estimate_ms={"level2_depth1": 0.36, "level2_depth2": 0.72},
                       counters={k: rates(sessions[k]) for k in ("level2_depth1", "level2_depth2")})
    print(json.dumps(out["step"]), flush=True)
    del sessions
    torch.cuda.empty_cache()

    # ---- the history kernel against the torch path it replaces ------------------------------------------------------------------
    depth = 4
    env = hanabi_hip.HanabiEnv("Hanabi-Full", 2, n_games=N, seed=2, auto_reset=False, packed=True)
    for t in range(7):
        env.step(env.random_legal_actions(seed=3, draw=t))
    prev = env.export_state()
    own = env.random_legal_actions(seed=4, draw=0)
    env.step(env.random_legal_actions(seed=3, draw=7))
    cur = env.export_state()
    reset = (torch.arange(N, device="cuda") % 7 == 0).to(torch.uint8)
    cfg, seat = env.cfg, int(current_player(cur)[0].item())
    hk, ht = PartnerHistory(cfg, N, depth, "cuda"), PartnerHistory(cfg, N, depth, "cuda")

    def torch_path():
        ht.own_move(own)
        w2 = cur[:, 2]
        partner = (w2 >> 1) & 7
        valid = running(cur) & ((w2 & 1) != 0) & (partner != seat) & running(prev) & (current_player(prev) == partner)
        ht.push(prev, last_move_uid(cfg, cur), 1, valid.to(torch.uint8), seat=seat)

    def torch_path_with_reset():
        ht.own_move(own)
        gone = reset != 0
        ht.valid[:, gone] = 0
        ht.alive[:, gone] = 0
        torch_path()

    parts = dict(kernel=lambda: hk.advance(own_moves=own, cur_rows=cur, prev_rows=prev, seat=seat, draw=1),
                 kernel_with_reset=lambda: hk.advance(own_moves=own, reset=reset, cur_rows=cur, prev_rows=prev, seat=seat, draw=1),
                 kernel_no_push=lambda: hk.advance(own_moves=own, reset=reset),
                 torch_path=torch_path, torch_path_with_reset=torch_path_with_reset)
    hist = {}
    for name, fn in parts.items():
        for _ in range(10):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(100):
            fn()
        e1.record()
        torch.cuda.synchronize()
        hist[name] = round(e0.elapsed_time(e1) * 10, 2)
    hist.update(games=N, depth=depth, state_words=env.state_words,
                kernel_bytes=N * (2 * depth * env.state_words * 4 + 2 * depth * (4 + 1 + 1)),   # read + written, from shapes
                torch_over_kernel=round(hist["torch_path"] / hist["kernel"], 1))
    hist["kernel_GBps"] = round(hist["kernel_bytes"] / hist["kernel"] / 1e3, 1)
    out["history_us"] = hist
    print(json.dumps(hist), flush=True)
    del env, hk, ht
    torch.cuda.empty_cache()

    # ---- a short ladder ------------------------------------------------------------------------------------------------------------
    if not skip_learn:
        n, pool, names, runs = 4096, [], [], []
        for seed in (1, 2):
            frozen = None
            for lvl in (1, 2):
                env = hanabi_hip.HanabiEnv("Hanabi-Small", 2, n_games=n, seed=100 * lvl + seed, packed=True)
                team = agents_for(env, (seed + 20 * lvl, seed + 20 * lvl + 10), experience_buffer_size=1 << 17, train_batch_size=128)
                sess = OffBeliefSession(env, team) if lvl == 1 else OffBeliefSession(env, team, belief_policy=frozen, depth=2, oversample=4)
                t0 = time.perf_counter()
                sess.run(ladder_steps)
                torch.cuda.synchronize()
                info = dict(run=f"level{lvl}/{seed}", env_steps=sess.env_steps, grad_steps=sess.grad_steps,
                            seconds=round(time.perf_counter() - t0, 1), train_score=round(sess.mean_score(), 3))
                if lvl == 1:
                    frozen = [frozen_copy(a) for a in team]
                else:
                    info["counters"] = rates(sess)
                print(json.dumps(info), flush=True)
                runs.append(info)
                pool += team
                names.append(info["run"])
        # pool: run 1 level 1 (0, 1), level 2 (2, 3); run 2 level 1 (4, 5), level 2 (6, 7). Per level: own teams, then seats swapped
        teams = [(0, 1), (4, 5), (0, 5), (4, 1), (2, 3), (6, 7), (2, 7), (6, 3)]
        res = CrossPlay("Hanabi-Small", 2, n_games=4096, seed=7, responses=True).run(pool, teams=teams)
        dist = res.convention_distance()
        cell = lambda k: [round(res.results[k].mean, 3), round(res.results[k].stderr, 3)]
        table = {kind: dict(self_play=[cell(b), cell(b + 1)], cross_play=[cell(b + 2), cell(b + 3)],
                            convention_distance=round(float(dist[b, b + 1]), 4)) for kind, b in (("level1", 0), ("level2", 4))}
        out["ladder"] = dict(game="Hanabi-Small", players=2, games=n, steps=ladder_steps, env_steps=n * ladder_steps, depth=2, oversample=4,
                             agents=names, runs=runs, eval_games=4096, teams=teams, table=table)
        print(json.dumps(out["ladder"]["table"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


def level2_soft(path, ladder_steps, skip_learn, resources, measure):
    """The `soft` part; see the module docstring."""
    out = {}
    if os.path.exists(path):
        with open(path) as f:
            out = json.load(f)

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)

    if resources:
        out["kernel"] = kernel_resources("belief.hip", only="select_soft")
        print(json.dumps(out["kernel"]), flush=True)
        save()
    if not measure:
        return
    import torch

    import hanabi_hip
    from hanabi_agents.rlax_dqn import ActionSpec, DQNAgent, ObservationSpec, RlaxRainbowParams
    from hanabi_hip import CrossPlay, OffBeliefSession
    from hanabi_hip.obl import frozen_copy

    if not torch.cuda.is_available():
        raise SystemExit("obl_probe.py measures on the GPU: none found")
    EPS = 0.1   # RlaxRainbowParams.epsilon's default: what the live agents explore with

    def agents_for(env, seeds, **kw):
        base = dict(train_batch_size=256, experience_buffer_size=1 << 19, layers=[512], mask_terminal=True, compute_dtype="bfloat16",
                    packed_obs=True)
        base.update(kw)
        agents = [DQNAgent(ObservationSpec((env.n, env.obs_len)), ActionSpec(env.num_actions), RlaxRainbowParams(seed=s, **base),
                           device="cuda") for s in seeds]
        assert all(float(a.params.epsilon(0)) == EPS for a in agents)
        return agents

    def window(sess, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            sess.step()
        sess.flush()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1000 / steps

    names = OffBeliefSession.LEVEL_COUNTERS + ("ess_sum", "belief_forwards", "t")
    read = lambda sess: {k: getattr(sess, k) for k in names}

    def rates(c):
        rows = max(1, c["conditioned_rows"] + c["fallback_rows"] + c["unconditioned_rows"])
        cond = max(1, c["conditioned_rows"])
        return dict(c, conditioned=round(c["conditioned_rows"] / rows, 4), fallback=round(c["fallback_rows"] / rows, 4),
                    unconditioned=round(c["unconditioned_rows"] / rows, 4), survivors_per_conditioned_row=round(c["survivors"] / cond, 3),
                    depth_used_per_conditioned_row=round(c["depth_used_sum"] / cond, 3), mean_ess=round(c["ess_sum"] / cond, 3),
                    belief_forwards_per_step=round(c["belief_forwards"] / max(1, c["t"]), 2))

    # ---- step time: one session per depth, the switch toggled between its windows ------------------------------------------------
    sessions = {}
    for depth in (1, 2):
        env = hanabi_hip.HanabiEnv("Hanabi-Full", 2, n_games=N, seed=1, packed=True)
        agents = agents_for(env, (1, 2))
        sess = sessions["depth%d" % depth] = OffBeliefSession(env, agents, belief_policy=[frozen_copy(x) for x in agents], depth=depth,
                                                              oversample=4)
        window(sess, WARM)
        sess.belief_epsilon = EPS   # both paths warm
        window(sess, 20)
    legs = [(d, soft) for d in sessions for soft in (False, True)]
    label = lambda d, soft: d + ("_soft" if soft else "_hard")
    ms = {label(*leg): [] for leg in legs}
    sums = {label(*leg): dict.fromkeys(names, 0) for leg in legs}
    for _ in range(REPS):
        for d, soft in legs:
            sess = sessions[d]
            sess.belief_epsilon = EPS if soft else None
            before = read(sess)
            ms[label(d, soft)].append(round(window(sess, STEPS), 4))
            after = read(sess)
            for k in names:
                sums[label(d, soft)][k] += after[k] - before[k]
    out["step"] = dict(games=N, steps_per_window=STEPS, oversample=4, belief_epsilon=EPS, ms_per_step_runs=ms,
                       ms_per_step_best={k: min(v) for k, v in ms.items()},
                       window_spread_ms={k: round(max(v) - min(v), 4) for k, v in ms.items()},
                       counters={k: rates(v) for k, v in sums.items()})
    print(json.dumps(out["step"]), flush=True)
    save()
    del sessions, sess, env, agents
    torch.cuda.empty_cache()

    # ---- the ladder's level-2 session (Hanabi-Small, 4 096 games, batch 128, depth 2), timed the same way: a ladder run's seconds
    # depend on its session's place in the process, the toggled windows of one session do not
    env = hanabi_hip.HanabiEnv("Hanabi-Small", 2, n_games=4096, seed=201, packed=True)
    team = agents_for(env, (41, 51), experience_buffer_size=1 << 17, train_batch_size=128)
    sess = OffBeliefSession(env, team, belief_policy=[frozen_copy(a) for a in team], depth=2, oversample=4)
    window(sess, WARM)
    sess.belief_epsilon = EPS
    window(sess, 20)
    small = {"hard": [], "soft": []}
    for _ in range(REPS):
        for soft in (False, True):
            sess.belief_epsilon = EPS if soft else None
            small["soft" if soft else "hard"].append(round(window(sess, STEPS), 4))
    out["ladder_step"] = dict(game="Hanabi-Small", games=4096, depth=2, oversample=4, steps_per_window=STEPS, ms_per_step_runs=small,
                              ms_per_step_best={k: min(v) for k, v in small.items()})
    print(json.dumps(out["ladder_step"]), flush=True)
    save()
    del sess, env, team
    torch.cuda.empty_cache()

    # ---- `level2`'s short ladder, level 2 with the soft filter ---------------------------------------------------------------------
    if not skip_learn:
        n, pool, runs = 4096, [], []
        for seed in (1, 2):
            frozen = None
            for lvl in (1, 2):
                env = hanabi_hip.HanabiEnv("Hanabi-Small", 2, n_games=n, seed=100 * lvl + seed, packed=True)
                team = agents_for(env, (seed + 20 * lvl, seed + 20 * lvl + 10), experience_buffer_size=1 << 17, train_batch_size=128)
                sess = OffBeliefSession(env, team) if lvl == 1 else OffBeliefSession(env, team, belief_policy=frozen, depth=2, oversample=4,
                                                                                     belief_epsilon=EPS)
                t0 = time.perf_counter()
                sess.run(ladder_steps)
                torch.cuda.synchronize()
                info = dict(run=f"level{lvl}{'_soft' if lvl == 2 else ''}/{seed}", env_steps=sess.env_steps, grad_steps=sess.grad_steps,
                            seconds=round(time.perf_counter() - t0, 1), train_score=round(sess.mean_score(), 3))
                if lvl == 1:
                    frozen = [frozen_copy(a) for a in team]
                else:
                    info["counters"] = rates(read(sess))
                print(json.dumps(info), flush=True)
                runs.append(info)
                pool += team
        # pool and teams as in `level2`: per level its own teams, then the seats swapped between the runs
        teams = [(0, 1), (4, 5), (0, 5), (4, 1), (2, 3), (6, 7), (2, 7), (6, 3)]
        res = CrossPlay("Hanabi-Small", 2, n_games=4096, seed=7, responses=True).run(pool, teams=teams)
        dist = res.convention_distance()
        cell = lambda k: [round(res.results[k].mean, 3), round(res.results[k].stderr, 3)]
        table = {kind: dict(self_play=[cell(b), cell(b + 1)], cross_play=[cell(b + 2), cell(b + 3)],
                            convention_distance=round(float(dist[b, b + 1]), 4)) for kind, b in (("level1", 0), ("level2_soft", 4))}
        out["ladder"] = dict(game="Hanabi-Small", players=2, games=n, steps=ladder_steps, env_steps=n * ladder_steps, depth=2, oversample=4,
                             belief_epsilon=EPS, runs=runs, eval_games=4096, teams=teams, table=table)
        print(json.dumps(out["ladder"]["table"]), flush=True)
        save()


def main():
    import argparse

    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("out", nargs="?", default=None)
    ap.add_argument("--skip-learn", action="store_true")
    ap.add_argument("--learn-steps", type=int, default=4000)
    ap.add_argument("--level2", action="store_true")
    ap.add_argument("--level2-steps", type=int, default=20000)
    ap.add_argument("--soft", action="store_true")
    ap.add_argument("--encode-rows", action="store_true")
    ap.add_argument("--resources-only", action="store_true")
    ap.add_argument("--skip-resources", action="store_true")
    ap.add_argument("--sessions-in-a-row", action="store_true")
    opt = ap.parse_args()
    if opt.sessions_in_a_row:
        return sessions_in_a_row(opt.out or os.path.join(ROOT, "profiles", "obl", "encode_rows_probe.json"))
    if opt.encode_rows:
        return encode_rows_probe(opt.out or os.path.join(ROOT, "profiles", "obl", "encode_rows_probe.json"),
                                 resources=not opt.skip_resources, measure=not opt.resources_only)
    if opt.level2 and opt.soft:
        return level2_soft(opt.out or os.path.join(ROOT, "profiles", "obl", "obl_soft_probe.json"), opt.level2_steps, opt.skip_learn,
                           resources=not opt.skip_resources, measure=not opt.resources_only)
    if opt.level2:
        return level2(opt.out or os.path.join(ROOT, "profiles", "obl", "obl_level2_probe.json"), opt.level2_steps, opt.skip_learn)
    opt.out = opt.out or os.path.join(ROOT, "profiles", "obl", "obl_probe.json")
    path, learn_steps = opt.out, opt.learn_steps
    out = {"kernel": kernel_resources()}
    print(json.dumps(out["kernel"]), flush=True)

    import torch

    import hanabi_hip
    from hanabi_agents.rlax_dqn import ActionSpec, DQNAgent, ObservationSpec, RlaxRainbowParams
    from hanabi_hip import CrossPlay, OffBeliefSession, _capi as K
    from hanabi_hip.search import Determinizer, _ask
    from hanabi_hip.selfplay import SelfPlaySession

    if not torch.cuda.is_available():
        raise SystemExit("obl_probe.py measures on the GPU: none found")

    def agents_for(env, seeds, **kw):
        base = dict(train_batch_size=256, experience_buffer_size=1 << 19, layers=[512], mask_terminal=True, compute_dtype="bfloat16",
                    packed_obs=True)
        base.update(kw)
        return [DQNAgent(ObservationSpec((env.n, env.obs_len)), ActionSpec(env.num_actions), RlaxRainbowParams(seed=s, **base),
                         device="cuda") for s in seeds]

    def window(sess, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            sess.step()
        sess.flush()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1000 / steps

    # ---- step time ----------------------------------------------------------------------------------------------------------
    sessions = {}
    for name, make in (("selfplay", lambda e, a: SelfPlaySession(e, a)),
                       ("selfplay_ordinary_path", lambda e, a: SelfPlaySession(e, a, native_chain=False)),
                       ("off_belief", lambda e, a: OffBeliefSession(e, a))):
        env = hanabi_hip.HanabiEnv("Hanabi-Full", 2, n_games=N, seed=1, packed=True)
        sessions[name] = make(env, agents_for(env, (1, 2)))
        window(sessions[name], WARM)
    ms = {k: [] for k in sessions}
    for _ in range(REPS):
        for name, sess in sessions.items():
            ms[name].append(round(window(sess, STEPS), 4))
    obl = sessions["off_belief"]
    out["step"] = dict(games=N, steps_per_window=STEPS, ms_per_step_best={k: min(v) for k, v in ms.items()}, ms_per_step_runs=ms,
                       ratio_to_selfplay=round(min(ms["off_belief"]) / min(ms["selfplay"]), 3),
                       ratio_to_ordinary_path=round(min(ms["off_belief"]) / min(ms["selfplay_ordinary_path"]), 3),
                       native_steps=sessions["selfplay"].native_steps, dead_rows=obl.dead_rows, grad_steps=obl.grad_steps)
    print(json.dumps(out["step"]), flush=True)

    # ---- the branch, launch by launch ----------------------------------------------------------------------------------------
    env, sc, agent, partner = obl.env, obl.scratch, obl.agents[0], obl.agents[1]
    det = Determinizer(config=env.cfg)
    rows = env.export_state()
    det_rows, det_w = torch.empty_like(rows), torch.empty(N, dtype=torch.int32, device="cuda")
    moves = env.random_legal_actions(seed=3, draw=1)
    scratch = {}
    buf = agent.experience

    def insert_obl():
        K.check(K.lib().hb_obl_insert(K.dptr(env.net_obs), K.dptr(moves), K.dptr(obl._rew), K.dptr(obl._term), K.dptr(sc.net_obs),
                                      K.dptr(sc.legal), K.dptr(buf._obs_tm1_buf), K.dptr(buf._obs_t_buf), K.dptr(buf._act_tm1_buf),
                                      K.dptr(buf._lms_t_buf), K.dptr(buf._rew_t_buf), K.dptr(buf._terminal_t_buf), N, 2,
                                      env.net_obs.shape[1] * 4, env.num_actions, buf.capacity, 0, K.current_stream()))

    def insert_replay():
        hanabi_hip.ops.replay_insert(agent.last_obs, env.net_obs, env.legal, moves, env.agent_reward, env.agent_step_type, buf, 0)

    def scratch_step():
        sc.import_state(det_rows)   # (a finished game would make the step a no-op: start from the same states every time)
        obl._scratch_step(moves, 0)

    parts = dict(export_state=lambda: env.export_state(),
                 determinize=lambda: det.sample(rows, seat=0, replicas=1, seed=1, draw=1, out=(det_rows, det_w)),
                 import_state=lambda: sc.import_state(det_rows),
                 import_and_env_step=scratch_step,
                 partner_forward=lambda: _ask(partner, sc, 1, 1, obl.branch_moves[1], scratch),
                 obl_insert=insert_obl, replay_insert=insert_replay)
    split = {}
    for name, fn in parts.items():
        for _ in range(10):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(100):
            fn()
        e1.record()
        torch.cuda.synchronize()
        split[name] = round(e0.elapsed_time(e1) * 10, 2)
    row = env.net_obs.shape[1] * 4
    split["obl_insert_bytes"] = N * (4 * row + 2 * env.num_actions + 4 + 2 * (4 + 1) + 1 + 4 + 1)   # read + written, from shapes
    split["obl_insert_GBps"] = round(split["obl_insert_bytes"] / split["obl_insert"] / 1e3, 1)
    out["split_us"] = split
    print(json.dumps(split), flush=True)
    del sessions, obl, env, sc, agent, partner, buf
    torch.cuda.empty_cache()

    # ---- a short learning run --------------------------------------------------------------------------------------------------
    if not opt.skip_learn:
        n = 4096
        pool, names = [], []
        for kind, cls in (("off_belief", OffBeliefSession), ("selfplay", SelfPlaySession)):
            for seed in (1, 2):
                env = hanabi_hip.HanabiEnv("Hanabi-Small", 2, n_games=n, seed=100 + seed, packed=True)
                # one agent per seat (an agent keeps one last_obs per game: plain self-play cannot share it between seats)
                team = agents_for(env, (seed, seed + 10), experience_buffer_size=1 << 17, train_batch_size=128)
                sess = cls(env, team)
                t0 = time.perf_counter()
                sess.run(learn_steps)
                torch.cuda.synchronize()
                pool += team
                names.append(f"{kind}/{seed}")
                print(json.dumps(dict(run=names[-1], env_steps=sess.env_steps, grad_steps=sess.grad_steps, seconds=round(time.perf_counter() - t0, 1),
                                      train_score=round(sess.mean_score(), 3))), flush=True)
        # run r's agents are pool[2r], pool[2r + 1] (seats 0, 1). Per kind: the two runs' own teams, then the seats swapped between them
        teams = [(0, 1), (2, 3), (0, 3), (2, 1), (4, 5), (6, 7), (4, 7), (6, 5)]
        res = CrossPlay("Hanabi-Small", 2, n_games=4096, seed=7, responses=True).run(pool, teams=teams)
        dist = res.convention_distance()
        cell = lambda k: [round(res.results[k].mean, 3), round(res.results[k].stderr, 3)]
        table = {kind: dict(self_play=[cell(b), cell(b + 1)], cross_play=[cell(b + 2), cell(b + 3)],
                            convention_distance=round(float(dist[b, b + 1]), 4)) for kind, b in (("off_belief", 0), ("selfplay", 4))}
        out["learn"] = dict(game="Hanabi-Small", players=2, games=n, steps=learn_steps, env_steps=n * learn_steps, agents=names,
                            eval_games=4096, teams=teams, table=table)
        print(json.dumps(out["learn"]["table"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
