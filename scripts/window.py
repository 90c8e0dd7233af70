"""The update's whole-CU window in a rocprofv3 --kernel-trace run of bench.py (DESIGN section 5c "Co-residency"): per step of
the steady-state window (the launches scripts/timeline.py takes), the acting queue's idle time between consecutive launches,
which learner kernels run inside each gap, and the serial chain c51_backward -> dW1 -> Adam as it runs in the loop.
Usage: window.py <dir with *_kernel_trace.csv | the csv itself (.gz allowed)> [first step, last step]"""
import csv
import glob
import gzip
import os
import re
import sys
from collections import defaultdict

src = sys.argv[1]
f = src if os.path.isfile(src) else sorted(glob.glob(os.path.join(src, "**", "*kernel_trace.csv"), recursive=True))[-1]
rows = list(csv.DictReader(gzip.open(f, "rt") if f.endswith(".gz") else open(f)))
t = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Queue_Id"], r["Kernel_Name"]) for r in rows)
STEP = "actor_env_fused_kernel"
steps = [x for x in t if STEP in x[3]]
a, b = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (80, 230)
lo, hi = steps[a][0], steps[b][0]
acting_q = steps[a][2]


def short(n):
    n = re.sub(r"\(anonymous namespace\)::", "", n)
    return re.sub(r"^void ", "", n).split("(")[0].split("<")[0][:28]


def med(v):
    v = sorted(v)
    return v[len(v) // 2] if v else 0.0


act = [x for x in t if x[2] == acting_q and lo <= x[0] <= hi]
learn = [x for x in t if x[2] != acting_q and x[1] >= lo and x[0] <= hi]
print(f"{os.path.basename(f)}: steps {a}..{b} of {len(steps)}, {(hi - lo) / 1e3 / (b - a):.1f} us per step; acting queue {acting_q}")
print("\n-- acting queue: idle gaps between consecutive launches, and the learner kernels that run inside them (us inside the gap)")
per_step_idle, inside_tot, n_gap = defaultdict(float), defaultdict(float), 0
step_no = a
for i in range(len(act) - 1):
    g0, g1 = act[i][1], act[i + 1][0]
    if STEP in act[i][3]:
        step_no += 1
    gap = (g1 - g0) / 1e3
    per_step_idle[step_no] += max(gap, 0.0)
    if gap < 1.0:
        continue
    n_gap += 1
    ins = [(short(x[3]), (min(x[1], g1) - max(x[0], g0)) / 1e3) for x in learn if x[0] < g1 and x[1] > g0]
    for k, v in ins:
        inside_tot[k] += v
    print(f"step {step_no:4d} after {short(act[i][3]):24s} idle {gap:6.1f} us: " + ", ".join(f"{k} {v:.1f}" for k, v in ins))
idle = list(per_step_idle.values())
print(f"\nidle per step: median {med(idle):.1f} us, mean {sum(idle) / max(len(idle), 1):.1f} us, {n_gap} gaps of 1 us or more")
tot_idle = sum(idle)
print("share of the idle time in which each learner kernel runs (kernels overlap each other, so the shares may add to more than 100 %):")
for k, v in sorted(inside_tot.items(), key=lambda kv: -kv[1])[:10]:
    print(f"   {k:30s} {v / max(tot_idle, 1e-9) * 100:5.1f} %   {v / max(len(idle), 1):5.1f} us per step")

print("\n-- serial chain per update: c51_backward -> dW1 (Cijk_* library GEMM or learner_tail_l2_dw1) -> Adam (last launch)")
byq = defaultdict(list)
for x in learn:
    byq[x[2]].append(x)
chains = []
for q, xs in byq.items():
    for i, x in enumerate(xs):
        if "c51_backward" not in x[3]:
            continue
        seq = [x]
        for y in xs[i + 1:]:   # the launches that FOLLOW the backward on its queue: the chain ends at the first other kernel
            if not ("Cijk_" in y[3] or "learner_tail" in y[3] or "noisy_adam" in y[3]):
                break
            seq.append(y)
        if len(seq) >= 3 and x[0] >= lo and seq[-1][1] <= hi:
            chains.append(seq)
chains.sort(key=lambda s: s[0][0])
for s in chains[:12]:
    print(f"   queue {s[0][2]}: " + " | ".join(f"{short(y[3])} {(y[1] - y[0]) / 1e3:.1f} (+{(y[0] - s[j - 1][1]) / 1e3 if j else 0:.1f} wait)"
                                           for j, y in enumerate(s)) + f" = {(s[-1][1] - s[0][0]) / 1e3:.1f} us")
if chains:
    print(f"{len(chains)} updates: chain start -> end median {med([(s[-1][1] - s[0][0]) / 1e3 for s in chains]):.1f} us; "
          f"sum of kernel times median {med([sum(y[1] - y[0] for y in s) / 1e3 for s in chains]):.1f} us; per kernel median: "
          + ", ".join(f"{short(chains[0][j][3])} {med([(s[j][1] - s[j][0]) / 1e3 for s in chains if len(s) > j]):.1f}" for j in range(len(chains[0]))))
    lib = sum(1 for x in t if lo <= x[0] <= hi and "Cijk_" in x[3])
    print(f"library GEMM (Cijk_*) launches in the window: {lib}")
