"""bench.py's own launcher (CPU box, gloo): `python bench.py --gpus 2` with no WORLD_SIZE in the environment starts its two
ranks itself, they rendezvous on 127.0.0.1 and all-reduce; a failing rank makes the parent exit non-zero instead of hanging."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(extra_env=None, args=("--gpus", "2", "--launch-check")):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(HB_DIST_BACKEND="gloo", **(extra_env or {}))
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], env=env, capture_output=True, text=True,
                          timeout=300)


def test_bench_starts_its_own_ranks():
    r = _run()
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout            # exactly one JSON line, from rank 0
    out = json.loads(lines[0])
    assert out == {"launch_check": True, "world": 2, "backend": "gloo", "sum": 3.0}


def test_bench_failed_rank_gives_nonzero_exit():
    r = _run({"HB_BENCH_FAIL_RANK": "1"})
    assert r.returncode != 0
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]


def test_bench_under_a_launcher_keeps_its_world():
    """Started with WORLD_SIZE already set (torch.distributed.run does that), bench.py must NOT spawn again."""
    env = {"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0", "MASTER_PORT": "29999"}
    r = _run(env, args=("--gpus", "1", "--launch-check"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])["world"] == 1


def test_bench_options_parse_and_no_cpu_fallback():
    """The driver's flags and this round's additions parse; without a GPU the benchmark itself refuses to run instead of
    falling back to anything."""
    code = ("import os, sys; sys.argv=['bench.py','--gpus','1','--steps','20','--warmup','5','--actor-lag','1','--event-every','4',"
            "'--no-async-variant','--vanilla','--dump-outputs','out']; import bench; a=bench.parse(); "
            "print(a.steps, a.warmup, a.actor_lag, a.event_every, a.prime, a.vanilla, a.dump_outputs)")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == ["20", "5", "1", "4", "24", "True", "out"]
    import torch

    if not torch.cuda.is_available():
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1"],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and "no CPU fallback" in (r.stderr + r.stdout)


import pytest  # noqa: E402


@pytest.mark.gpu
def test_bench_line_keeps_the_measurement_contract():
    """`python bench.py` on the GPU: exactly one JSON line on stdout with the contract's keys (metric / value / unit / n_gpus /
    steps / warmup / ms_per_step / higher_is_better / scaling / vs_baseline / dtype / data / config.workload), the roofline
    object of the dominant kernel (bound, achieved, peak, unit, frac, traffic) and the CPU baselines; value = games x steps / time."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "6", "--warmup", "2", "--games", "2048",
                        "--cpu-sample-games", "256", "--cpu-sample-steps", "20"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline", "cpu_baseline_learner", "grad_steps_per_sec"):
        assert k in d, k
    assert d["metric"] == "env_steps_per_sec" and d["unit"] == "env-steps/s" and d["n_gpus"] == 1 and d["steps"] == 6 and d["warmup"] == 2
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None and d["data"] == "synthetic"
    assert "workload" in d["config"] and "model" not in d["config"]
    assert abs(d["value"] - 2048 * 6 / (d["ms_per_step"] * 6 / 1e3)) <= 1e-6 * d["value"]
    r_ = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r_, k
    assert r_["bound"] == "hbm" and r_["unit"] == "GB/s" and abs(r_["frac"] - r_["achieved"] / r_["peak"]) < 1e-9
    c = d["cpu_baseline"]
    assert c["kind"] in ("port", "reference") and c["cores"] >= 1 and c["value"] > 0 and "sample" in c
    assert d["async_actor"]["actor_lag"] == 1 and d["async_actor"]["env_steps_per_sec"] > 0


def _fake_run(n, hidden):
    """What dump_outputs reads after the timed steps, as CPU tensors: an env's per-game outputs and one agent's network."""
    import types

    import torch

    g = torch.Generator().manual_seed(5)
    env = types.SimpleNamespace(n=n, players=2, device=torch.device("cpu"),
                                obs=torch.randint(0, 2, (n, 658), generator=g, dtype=torch.int8),
                                legal=torch.randint(0, 2, (n, 20), generator=g, dtype=torch.int8), reward=torch.randn(n, generator=g),
                                terminal=torch.zeros(n, dtype=torch.int8), score=torch.randint(0, 25, (n,), generator=g, dtype=torch.int8),
                                agent_reward=torch.randn(n, generator=g), agent_step_type=torch.ones(n, dtype=torch.int8))
    with torch.random.fork_rng():
        torch.manual_seed(5)
        net = torch.nn.Linear(658, hidden)
    agent = types.SimpleNamespace(online=net, last_loss=torch.tensor(0.25))
    return env, types.SimpleNamespace(agents=[agent, object()]), torch.randint(0, 20, (n,), generator=g, dtype=torch.int32)


def test_dump_outputs_files_budget_and_repeatability(tmp_path):
    """--dump-outputs writes float32 / float64 .npy files within the budget; per-game arrays keep the same seeded game sample and
    arrays too large for the budget the same seeded element sample, so two runs write identical files."""
    import numpy as np

    sys.path.insert(0, ROOT)
    import bench

    budget = 4_000_000
    dumps = []
    for d in ("a", "b"):
        env, session, actions = _fake_run(5000, 1024)
        info = bench.dump_outputs(str(tmp_path / d), env, session, actions, budget=budget)
        files = sorted(os.listdir(tmp_path / d))
        assert info["files"] == len(files) and info["bytes"] == sum(os.path.getsize(tmp_path / d / f) for f in files)
        assert info["bytes"] <= budget + 128 * len(files)
        dumps.append({f: np.load(tmp_path / d / f) for f in files})
    a, b = dumps
    assert a.keys() == b.keys()
    for f in a:
        assert a[f].dtype in (np.float32, np.float64), f
        assert np.array_equal(a[f], b[f]), f
    rows = a["game_rows.npy"].astype(np.int64)
    assert len(rows) == 2048 and np.all(np.diff(rows) > 0) and rows[-1] < 5000
    env, _, actions = _fake_run(5000, 1024)
    assert np.array_equal(a["actions.npy"], actions.numpy()[rows].astype(np.float32))
    assert np.array_equal(a["legal.npy"], env.legal.numpy()[rows].astype(np.float32))
    assert a["agent0_loss.npy"] == np.float32(0.25)
    # the 1024 x 658 weight does not fit: a sorted sample of its elements, with the indices beside it
    el = a["agent0_weight_elems.npy"].astype(np.int64)
    w = _fake_run(5000, 1024)[1].agents[0].online.weight.detach().numpy().reshape(-1)
    assert len(el) < w.size and np.array_equal(a["agent0_weight.npy"], w[el])
    assert "agent0_bias_elems.npy" not in a


@pytest.mark.gpu
def test_bench_dump_outputs(tmp_path):
    """`bench.py --dump-outputs DIR` on the GPU: the timed path's last-step outputs as float32 files under 64 MB, the
    result line still one JSON line whose `steps` is the requested count."""
    import numpy as np

    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "5", "--warmup", "2", "--games", "4096",
                        "--no-cpu-baseline", "--no-async-variant", "--no-nstep-variant", "--no-fp16-variant",
                        "--dump-outputs", str(tmp_path)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 5 and d["ms_per_step"] > 0 and d["dump_outputs"]["dir"] == str(tmp_path)
    files = os.listdir(tmp_path)
    assert sum(os.path.getsize(tmp_path / f) for f in files) <= 64_000_000
    out = {f[:-4]: np.load(tmp_path / f) for f in files}
    assert all(v.dtype == np.float32 for k, v in out.items() if not k.endswith("_elems"))
    assert out["obs"].shape == (2048, 658) and out["legal"].shape == (2048, 20) and out["actions"].shape == (2048,)
    assert set(np.unique(out["obs"])) <= {0.0, 1.0}
    assert out["actions"].min() >= 0 and out["actions"].max() < 20
    assert "agent0_loss" in out and "agent1_loss" in out and np.isfinite(out["agent0_loss"]).all()
