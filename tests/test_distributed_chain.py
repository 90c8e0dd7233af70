"""Data-parallel self-play on the configuration the one-call step (hb_chain_run, SelfPlaySession._chain_for) accepts: packed env,
one-kernel actor ([512] net, 51 atoms), split update, default session options. tests/test_distributed.py runs [256] nets, which
never meet the chain's conditions, so nothing there can see a step that replays the update's two graphs WITHOUT the host-side
all-reduce that belongs between them. Here: (a) a witness that this configuration does reach the chain, (b) every gradient step of
a collective agent meets exactly one all-reduce of its gradient bucket, (c) two gloo ranks on one GPU end bit-identical and equal
to the ordinary path, (d) the one collective form the chain may replay (the all-reduce captured INSIDE the update's graph)."""
import datetime
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_distributed import ROOT, _free_port

N_GAMES, STEPS = 256, 36
PG_TIMEOUT = datetime.timedelta(seconds=90)   # a rank that skips a collective the other enters ends as an error, not a stall


def _child_setup(port=None, backend=None, rank=0, world=1, graph_collective=False):
    for p in (ROOT, os.path.join(ROOT, "hanabi-agents_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["HB_ACTOR_FUSED_MIN_ROWS"] = "0"   # the one-kernel actor at this file's 256 rows
    os.environ["HB_DP_GRAPH_COLLECTIVE"] = "1" if graph_collective else "0"
    torch.cuda.set_device(0)
    if backend is not None:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        kw = dict(device_id=torch.device("cuda", 0)) if backend == "nccl" else {}
        dist.init_process_group(backend, rank=rank, world_size=world, timeout=PG_TIMEOUT, **kw)


def _flat_weights(agent):
    return torch.cat([p.detach().reshape(-1) for p in agent.online.parameters()]).cpu()


def _session(game, rank=0, lag=0, native_chain=True, force_collective=False, local=False):
    """The shared configuration: the smallest at which the chain's conditions hold. Fresh env, agents and session."""
    import hanabi_hip
    from hanabi_agents.rlax_dqn import ActionSpec, DQNAgent, ObservationSpec, RlaxRainbowParams
    from hanabi_hip.selfplay import SelfPlaySession

    n = N_GAMES
    torch.manual_seed(0)
    flags = hanabi_hip.FLAG_AUTO_RESET | hanabi_hip.FLAG_RESET_START_NEXT
    env = hanabi_hip.HanabiEnv(config=hanabi_hip.make_config(game, 2, flags), n_games=n, seed=9, first_game_id=rank * n, packed=True)
    params = RlaxRainbowParams(train_batch_size=64, experience_buffer_size=n * 8, layers=[512], compute_dtype="bfloat16",
                               mask_terminal=True, target_update_period=6, packed_obs=True, actor_lag=lag)
    kw = dict(process_group=False) if local else {}
    agents = [DQNAgent(ObservationSpec((n, env.obs_len)), ActionSpec(env.num_actions), params._replace(seed=40 + s), device="cuda", **kw)
              for s in (0, 1)]
    for a in agents:
        a.first_game_id = rank * n
        a.force_collective = bool(force_collective)
    sess = SelfPlaySession(env, agents) if native_chain else SelfPlaySession(env, agents, native_chain=False)
    return env, agents, sess


def _play(sess, steps=STEPS):
    for _ in range(steps):
        sess.step()
    sess.flush()
    torch.cuda.synchronize()


def _snapshot(env, agents, sess, w0):
    out = dict(rows=env.export_state().cpu(), grad_steps=sess.grad_steps, native_steps=sess.native_steps, illegal=env.illegal_count(),
               fused_step=sorted({bool(ch.fused_step) for ch in sess._chains.values()}), agents=[])
    for a, w in zip(agents, w0):
        fl, buf = a._fl, a.experience
        out["agents"].append(dict(
            w0=w, w=_flat_weights(a), eff=torch.cat([t.reshape(-1) for pair in fl.eff for t in pair]).cpu(),
            state=[t.detach().cpu().clone() for pair in fl.state.values() for t in pair], step=fl.step.cpu().clone(),
            tree=buf.sum_tree.nodes().cpu(), obs_t=buf._obs_t_buf.cpu().clone(), act_tm1=buf._act_tm1_buf.cpu().clone()))
    return out


def _run(game, **kw):
    env, agents, sess = _session(game, **kw)
    w0 = [_flat_weights(a) for a in agents]
    _play(sess)
    return _snapshot(env, agents, sess, w0)


LEARNER_ITEMS = ("w", "eff", "state", "step")                       # what the all-reduce keeps equal across ranks
AGENT_ITEMS = LEARNER_ITEMS + ("tree", "obs_t", "act_tm1")          # what a rank's two paths must agree on, with the env rows


def _differing(x, y, items, session_items=()):
    """Names of the saved items that are not bit-identical between two snapshots, in saved order."""
    bad = [k for k in session_items if not (torch.equal(x[k], y[k]) if isinstance(x[k], torch.Tensor) else x[k] == y[k])]
    for seat, (a, b) in enumerate(zip(x["agents"], y["agents"])):
        for k in items:
            if k == "state":
                bad += [f"agent{seat}.state[{j}]" for j, (s, t) in enumerate(zip(a[k], b[k])) if not torch.equal(s, t)]
            elif not torch.equal(a[k], b[k]):
                bad.append(f"agent{seat}.{k}")
    return bad


# ---- (a) witness: the configuration reaches the chain --------------------------------------------------------------------------
def _witness_worker(rank, out):
    _child_setup()
    res = {game: _run(game) for game in ("Hanabi-Full", "Hanabi-Small")}
    torch.save(res, os.path.join(out, "witness.pt"))


@pytest.mark.gpu
def test_shared_configuration_reaches_the_one_call_step(tmp_path):
    """Without this the tests below can pass vacuously: a configuration the chain never accepts stays in lock step whatever the
    chain does with collectives. One rank, no process group: at least a third of the steps go through hb_chain_run, on the fused
    policy + env launch (Hanabi-Full) and on the two-launch form (Hanabi-Small)."""
    mp.spawn(_witness_worker, args=(str(tmp_path),), nprocs=1, join=True)
    r = torch.load(tmp_path / "witness.pt")
    for game, fused in (("Hanabi-Full", [True]), ("Hanabi-Small", [False])):
        print(f"witness {game}: native_steps {r[game]['native_steps']} of {STEPS}, grad_steps {r[game]['grad_steps']}")
        assert r[game]["native_steps"] >= 12, (game, r[game]["native_steps"])
        assert r[game]["grad_steps"] >= STEPS - 4 and r[game]["illegal"] == 0
        assert r[game]["fused_step"] == fused, (game, r[game]["fused_step"])


# ---- (b) every gradient step meets the all-reduce ------------------------------------------------------------------------------
class _BucketAllReduces:
    """Counts torch.distributed.all_reduce calls on the agents' flat gradient buckets: `steps` for the session's gradient steps,
    `warmup` for the eager updates inside DQNAgent._capture_update_graphs (three real updates per capture, whose effects are
    put back: they are no gradient steps of the session, and sess.grad_steps does not count them)."""

    def __init__(self, agents):
        from hanabi_agents.rlax_dqn import DQNAgent

        self.agents, self.steps, self.warmup, self._capturing = agents, 0, 0, 0
        self._orig_ar, self._cls, self._orig_cap = dist.all_reduce, DQNAgent, DQNAgent._capture_update_graphs
        counter = self

        def all_reduce(tensor, *a, **k):
            if any(ag._fl is not None and tensor.data_ptr() == ag._fl.flat_grad.data_ptr() for ag in counter.agents):
                if counter._capturing:
                    counter.warmup += 1
                else:
                    counter.steps += 1
            return counter._orig_ar(tensor, *a, **k)

        def capture(agent):
            counter._capturing += 1
            try:
                return counter._orig_cap(agent)
            finally:
                counter._capturing -= 1

        dist.all_reduce, DQNAgent._capture_update_graphs = all_reduce, capture

    def remove(self):
        dist.all_reduce, self._cls._capture_update_graphs = self._orig_ar, self._orig_cap


def _count_worker(rank, port, out, lag, native_chain):
    _child_setup(port, "gloo")
    res = {}
    for local in (False, True):
        if local and not native_chain:
            continue    # (the local agents are there to show that they KEEP the one-call step)
        env, agents, sess = _session("Hanabi-Full", lag=lag, native_chain=native_chain, force_collective=True, local=local)
        counter = _BucketAllReduces(agents)
        try:
            _play(sess)
        finally:
            counter.remove()
        res["local" if local else "collective"] = dict(
            allreduces=counter.steps, warmup_allreduces=counter.warmup, grad_steps=sess.grad_steps, native_steps=sess.native_steps,
            illegal=env.illegal_count(), collective=[bool(a._collective()) for a in agents])
    torch.save(res, os.path.join(out, "count.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.parametrize("native_chain", [True, False])
@pytest.mark.parametrize("lag", [0, 1])
def test_every_gradient_step_meets_the_allreduce(tmp_path, lag, native_chain):
    """One-rank gloo group, force_collective: the multi-rank update path. Each of the session's gradient steps must issue exactly
    one all-reduce of that agent's gradient bucket, whichever path the step takes. Agents built with process_group=False inside
    the same job are local on purpose: no all-reduce at all, and they keep the one-call step."""
    mp.spawn(_count_worker, args=(_free_port(), str(tmp_path), lag, native_chain), nprocs=1, join=True)
    r = torch.load(tmp_path / "count.pt")
    c = r["collective"]
    print(f"lag {lag} native_chain {native_chain}: {c}; local: {r.get('local')}")
    assert c["collective"] == [True, True] and c["illegal"] == 0
    assert c["grad_steps"] >= STEPS - 4
    assert c["allreduces"] == c["grad_steps"], (c["allreduces"], c["grad_steps"], c["native_steps"])
    if native_chain:
        loc = r["local"]
        assert loc["collective"] == [False, False] and loc["illegal"] == 0 and loc["grad_steps"] >= STEPS - 4
        assert loc["allreduces"] == 0 and loc["warmup_allreduces"] == 0
        assert loc["native_steps"] >= 12, loc["native_steps"]


# ---- (c) two ranks on one GPU ----------------------------------------------------------------------------------------------------
def _two_rank_worker(rank, world, port, out, game):
    _child_setup(port, "gloo", rank, world)
    res = {"native": _run(game, rank=rank, native_chain=True), "ordinary": _run(game, rank=rank, native_chain=False)}
    torch.save(res, os.path.join(out, f"c{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.parametrize("game", ["Hanabi-Small", "Hanabi-Full"])
def test_two_ranks_stay_identical_on_the_configuration_the_chain_accepts(tmp_path, game):
    """gloo, world size 2, both ranks on one GPU, synchronous agents. Each rank plays its own games (ids by rank); the averaged
    gradient keeps weights, effective weights, Adam moments and step count bit-identical across ranks; and on each rank the default
    session (native_chain=True) equals the ordinary path in everything it leaves behind, as
    test_one_host_call_per_step_gives_identical_training promises for one rank."""
    world = 2
    mp.spawn(_two_rank_worker, args=(world, _free_port(), str(tmp_path), game), nprocs=world, join=True)
    r = [torch.load(tmp_path / f"c{i}.pt") for i in range(world)]
    for run in ("native", "ordinary"):
        a, b = r[0][run], r[1][run]
        print(f"{game} {run}: native_steps {a['native_steps']} / {b['native_steps']}, grad_steps {a['grad_steps']} / {b['grad_steps']}")
        assert a["grad_steps"] == b["grad_steps"] >= STEPS - 4 and a["illegal"] == b["illegal"] == 0
        assert not torch.equal(a["rows"], b["rows"])                       # different games on each rank
        for ag in a["agents"]:
            assert not torch.equal(ag["w"], ag["w0"])                      # and the agents did learn
    for run in ("native", "ordinary"):
        bad = _differing(r[0][run], r[1][run], LEARNER_ITEMS)
        assert not bad, f"{game}, native_chain={run == 'native'}: ranks differ in {bad}"
    for rank in range(world):
        bad = _differing(r[rank]["native"], r[rank]["ordinary"], AGENT_ITEMS, session_items=("rows", "grad_steps", "illegal"))
        assert not bad, f"{game}, rank {rank}: the native_chain=True run differs from the ordinary path in {bad}"


# ---- (d) the collective captured inside the graph ------------------------------------------------------------------------------
def _graph_collective_worker(rank, port, out):
    _child_setup(port, "nccl", graph_collective=True)
    res = {}
    for run, native in (("native", True), ("ordinary", False)):
        env, agents, sess = _session("Hanabi-Full", lag=1, native_chain=native, force_collective=True)
        w0 = [_flat_weights(a) for a in agents]
        _play(sess)
        res[run] = _snapshot(env, agents, sess, w0)
        res[run]["in_graph"] = [bool(a._collective_in_graph()) and a._graph1 is not None and a._graph2 is None for a in agents]
    torch.save(res, os.path.join(out, "d.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
def test_collective_captured_inside_the_graph_may_take_the_one_call_step(tmp_path):
    """One-rank RCCL group, HB_DP_GRAPH_COLLECTIVE=1, actor_lag = 1: the all-reduce sits INSIDE the update's one graph, so a step
    that replays the graph replays the collective: the one collective form the chain may accept. Whatever path the steps take,
    the result equals the ordinary path's."""
    mp.spawn(_graph_collective_worker, args=(_free_port(), str(tmp_path)), nprocs=1, join=True)
    r = torch.load(tmp_path / "d.pt")
    for run in ("native", "ordinary"):
        print(f"in-graph collective, {run}: native_steps {r[run]['native_steps']}, grad_steps {r[run]['grad_steps']}")
        assert r[run]["in_graph"] == [True, True] and r[run]["illegal"] == 0 and r[run]["grad_steps"] >= STEPS - 4
    assert r["ordinary"]["native_steps"] == 0
    if r["native"]["native_steps"] == 0:
        print("in-graph collective: no step reached hb_chain_run; the two runs took the same path, equality not compared")
        return   # (the path is not forced)
    bad = _differing(r["native"], r["ordinary"], AGENT_ITEMS, session_items=("rows", "grad_steps", "illegal"))
    assert not bad, f"the native_chain=True run differs from the ordinary path in {bad}"
