"""GPU: prioritized replay on rings whose capacity is NOT the sum tree's (tests/per_cases.py), against three references at once:
the per-slot PER oracle (oracle/per_oracle.py: no heap in it), OracleTree driven as a ring's tree (per_cases.RingTree: bit for
bit) and the trajectory oracle of the replay ring (oracle/replay_oracle.py).

Safety: a wrong index here is an out-of-bounds device read. So every index is checked on the host (idx < capacity) before
anything gathers with it, and the C-ABI gathers never see the buffer's own rings but copies with T (the tree's size) rows whose
rows past `capacity` hold 0x5A and are checked intact: whatever leaf a broken sampler returned, the gather would read a guard
row, not foreign memory."""
import numpy as np
import pytest

import per_cases as PC
import replay_cases as RC
from oracle.per_oracle import PerOracle
from oracle.replay_oracle import ReplayOracle

pytestmark = pytest.mark.gpu

L, A, GAMMA = 33, 11, 0.99      # 33: the packed row's second word holds one bit
GUARD = 0x5A
RINGS = ("_obs_tm1_buf", "_obs_t_buf", "_act_tm1_buf", "_rew_t_buf", "_terminal_t_buf")


def _cuda(a):
    import torch

    return torch.as_tensor(np.array(a)).cuda()     # (a copy: the case table's arrays are read-only)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


class GuardedRings:
    """Byte copies of a buffer's five gathered rings, T rows each; rows capacity .. T-1 hold GUARD."""

    def __init__(self, buf, T):
        import torch

        self.cap, self.t = buf.capacity, {}
        for name in RINGS:
            src = getattr(buf, name).contiguous()
            row = src.shape[1] * src.element_size()
            g = torch.full((T * row,), GUARD, dtype=torch.uint8, device="cuda")
            g[:self.cap * row] = src.view(torch.uint8).reshape(-1)
            self.t[name] = (g, row)

    def ptrs(self):
        from hanabi_hip import _capi as K

        return [K.dptr(self.t[name][0]) for name in RINGS]

    def assert_intact(self, where):
        for name, (g, row) in self.t.items():
            assert bool((g[self.cap * row:] == GUARD).all()), (where, name, "a guard row changed")


class Truth:
    """What each slot holds and the n-step transition that starts there. Rings with a constant insert size: the trajectory
    oracle (row g of every insert is game g). Varying insert sizes (n_step 1 only): the rows as they were written, placed at
    the slots the PER oracle names."""

    def __init__(self, case, first_obs):
        self.replay = ReplayOracle(case.cap, first_obs) if len(case.n_ins) == 1 else None
        self.rows = {}

    def insert(self, slots, obs_tm1, obs, legal, action, reward, st):
        if self.replay is not None:
            assert np.array_equal(self.replay.last_obs, obs_tm1)
            assert self.replay.insert(obs, legal, action, reward, st) == slots      # two oracles, one ring placement
            return
        for g, s in enumerate(slots):
            self.rows[s] = dict(obs_tm1=obs_tm1[g].copy(), obs_t=obs[g].copy(), legal=legal[g].copy(), action=int(action[g]),
                                R=float(reward[g]), S=abs(float(reward[g])), m=1, disc=float(np.float32(GAMMA)),
                                terminal=bool(st[g] == 2))

    def nstep(self, slot, n_step):
        if self.replay is not None and self.replay.holder[slot] is not None:
            return self.replay.nstep(slot, n_step, GAMMA)
        if self.replay is None and slot in self.rows:
            assert n_step == 1
            return self.rows[slot]
        # a slot nobody wrote yet (only the top-edge key of a partly filled ring ends there): the ring's zeros, no successor
        z = np.zeros(L, np.int8)
        return dict(obs_tm1=z, obs_t=z, legal=np.zeros(A, np.int8), action=0, R=0.0, S=0.0, m=1, disc=float(np.float32(GAMMA)),
                    terminal=False)

    def table(self, idx, n_step):
        rows = [self.nstep(int(k), n_step) for k in idx]
        return dict(R=np.array([r["R"] for r in rows]), S=np.array([r["S"] for r in rows]), m=np.array([r["m"] for r in rows]),
                    disc=np.array([r["disc"] for r in rows]), term=np.array([r["terminal"] for r in rows]),
                    act=np.array([r["action"] for r in rows]), obs_tm1=np.stack([r["obs_tm1"] for r in rows]),
                    obs_t=np.stack([r["obs_t"] for r in rows]), legal=np.stack([r["legal"] for r in rows]))


def _check_gather(tab, n_step, x, act, rew, term, disc, where):
    B = len(act)
    assert np.array_equal(x[:B], tab["obs_tm1"].astype(np.float32)), (where, "obs_tm1 rows")
    assert np.array_equal(x[B:], tab["obs_t"].astype(np.float32)), (where, "obs_t rows")
    assert np.array_equal(act, tab["act"]), (where, "act")
    assert np.array_equal(term, tab["term"].astype(np.float32)), (where, "term")
    RC.check_rew_disc(rew, disc, tab, np.arange(B), n_step, GAMMA, tab["R"].astype(np.float32)[:, None], where)


def _gather_outputs(B):
    import torch

    x = torch.full((2 * B, L), RC.X_SENTINEL, dtype=torch.float32, device="cuda")
    act = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    rew, term, disc = (torch.full((B,), float("nan"), device="cuda") for _ in range(3))
    return x, act, rew, term, disc


def _host(*ts):
    return [t.cpu().numpy() for t in ts]


def _check_tree(buf, per, ref, where):
    nodes = buf.sum_tree.nodes().cpu().numpy()
    assert per.heap_violations(nodes) == dict(out_of_ring=0, leaf=0, inner=0), where
    assert np.array_equal(_bits(nodes[1:]), _bits(ref.nodes()[1:])), (where, "heap differs from OracleTree driven at the ring")
    return nodes


# ---- a. PriorityBuffer over the whole table ------------------------------------------------------------------------------------
@pytest.mark.parametrize("packed", [False, True], ids=["int8", "packed"])
@pytest.mark.parametrize("name", PC.NAMES)
def test_priority_buffer_matches_the_oracles(name, packed):
    """insert -> sample_batch_dev(B, uniforms with both edges forced) -> write-back with duplicate indices, two and a half laps.
    After every insert and every write-back the exported heap meets the slot oracle's three invariants and equals OracleTree's
    bit for bit; indices and probabilities equal OracleTree's bit for bit and are accepted by the slot oracle; max / min
    priority exact; the transitions of hb_replay_gather[_packed], the fused hb_per_sample_gather (uniforms rebuilt on the host
    from Philox) and the torch gathers equal the trajectory oracle's at n_step 1 and 3."""
    import torch

    from hanabi_agents.rlax_dqn.priority_buffer import PriorityBuffer
    from hanabi_hip import _capi as K

    case = PC.BY_NAME[name]
    cap, B, T = case.cap, case.B, PC.tree_capacity(case.cap)
    const = len(case.n_ins) == 1
    n_steps = (1, 3) if const else (1,)
    rng = np.random.default_rng(1000 + PC.NAMES.index(name))
    buf = PriorityBuffer(L, A, 1, cap, alpha=PC.ALPHA, device="cuda", packed=packed)
    assert buf.sum_tree.capacity == T and buf.sum_tree.ring_capacity == cap
    per, ref = PerOracle(cap, PC.ALPHA), PC.RingTree(cap)
    last = RC.make_rows(rng, case.n_ins[0], L, A)[0]
    truth = Truth(case, last)
    gather = K.lib().hb_replay_gather_packed if packed else K.lib().hb_replay_gather
    seed = 0x9E3779B97F4A7C15 ^ cap
    for r, rd in enumerate(PC.rounds(name)):
        where = (name, packed, r)
        # ---- insert
        obs, legal, action, reward = RC.make_rows(rng, rd.n, L, A)
        st = np.where(rng.random(rd.n) < 0.2, 2, 1).astype(np.int8)
        obs_tm1 = last if const else RC.make_rows(rng, rd.n, L, A)[0]
        buf.add_transitions(_cuda(obs_tm1), _cuda(action.reshape(-1, 1)), _cuda(reward.reshape(-1, 1)), _cuda(obs), _cuda(legal),
                            _cuda((st == 2).reshape(-1, 1)))
        truth.insert(per.insert(rd.n), obs_tm1, obs, legal, action, reward, st)
        ref.insert(rd.n)
        last = obs
        assert (buf.oldest_entry, buf.size) == (per.oldest, per.size), where
        _check_tree(buf, per, ref, where + ("insert",))
        # ---- sample: the indices reach the host before anything gathers with them
        u = _cuda(rd.u)
        idx_t, prob_t = buf.sum_tree.per_sample_dev(u)
        idx, prob = _host(idx_t, prob_t)
        assert ((idx >= 0) & (idx < cap)).all(), (where, idx[(idx < 0) | (idx >= cap)])
        want_idx, want_prob = ref.sample(rd.u)
        assert np.array_equal(idx, want_idx), where
        assert np.array_equal(_bits(prob), _bits(want_prob)), where
        keys = PerOracle.keys(B, rd.u)
        for i in range(B):
            assert per.accepts(idx[i], keys[i], T), (where, i, int(idx[i]), keys[i])
            assert abs(prob[i] - per.prob(idx[i])) <= PerOracle.prob_rtol(T) * per.prob(idx[i]), (where, i)
            assert i == B - 1 or idx[i] == per.exact_slot(keys[i]), (where, i)    # (tests/test_per_oracle_cpu.py: share 0)
        i2, p2, tr = buf.sample_batch_dev(B, u)
        assert torch.equal(i2, idx_t) and torch.equal(p2, prob_t), where
        tab1 = truth.table(idx, 1)
        assert np.array_equal(tr.observation_tm1.cpu().numpy(), tab1["obs_tm1"]), where
        assert np.array_equal(tr.observation_t.cpu().numpy(), tab1["obs_t"]), where
        assert np.array_equal(tr.legal_moves_t.cpu().numpy(), tab1["legal"]), where
        assert np.array_equal(tr.action_tm1.cpu().numpy()[:, 0], tab1["act"]), where
        assert np.array_equal(tr.terminal_t.cpu().numpy()[:, 0], tab1["term"]), where
        assert np.array_equal(tr.reward_t.cpu().numpy()[:, 0], tab1["R"].astype(np.float32)), where
        # ---- the three n-step gathers at those indices
        rings = GuardedRings(buf, T)
        size_wp = torch.tensor([per.size, per.oldest], dtype=torch.int64, device="cuda")
        n_ins = case.n_ins[0] if const else 1
        counter = torch.tensor(float(r), dtype=torch.float32, device="cuda")
        u_px = RC.philox_uniforms(seed, r, B)
        px_idx, px_prob = ref.sample(u_px)
        got_idx, got_prob = _host(*buf.sum_tree.per_sample_philox_dev(seed, counter, B))
        assert ((got_idx >= 0) & (got_idx < cap)).all(), where         # the separate launch first: the fused one gathers at once
        assert np.array_equal(got_idx, px_idx) and np.array_equal(_bits(got_prob), _bits(px_prob)), where
        px_keys = PerOracle.keys(B, u_px)
        assert all(per.accepts(px_idx[i], px_keys[i], T) for i in range(B)), where
        for n_step in n_steps:
            tab = tab1 if n_step == 1 else truth.table(idx, n_step)
            x, act, rew, term, disc = _gather_outputs(B)
            K.check(gather(*rings.ptrs(), K.dptr(idx_t), B, L, K.dptr(x), 0, L, K.dptr(act), K.dptr(rew), K.dptr(term), K.dptr(disc),
                           n_step, GAMMA, cap, n_ins, K.dptr(size_wp), K.current_stream()))
            _check_gather(tab, n_step, *_host(x, act, rew, term, disc), where + ("hb_replay_gather", n_step))
            t, d = buf.gather_nstep_dev(idx_t, n_step, GAMMA)
            xt = torch.cat([t.observation_tm1, t.observation_t]).float()
            assert np.array_equal(t.legal_moves_t.cpu().numpy(), tab["legal"]), where
            _check_gather(tab, n_step, *_host(xt, t.action_tm1[:, 0].int(), t.reward_t[:, 0], t.terminal_t[:, 0].float(), d),
                          where + ("gather_nstep_dev", n_step))
            f_idx = torch.full((B,), -1, dtype=torch.int64, device="cuda")
            f_prob = torch.zeros(B, dtype=torch.float64, device="cuda")
            x, act, rew, term, disc = _gather_outputs(B)
            K.check(K.lib().hb_per_sample_gather(buf.sum_tree.h, seed, K.dptr(counter), B, K.dptr(f_idx), K.dptr(f_prob), *rings.ptrs(),
                                                 L, 1 if packed else 0, K.dptr(x), 0, L, K.dptr(act), K.dptr(rew), K.dptr(term),
                                                 K.dptr(disc), n_step, GAMMA, cap, n_ins, K.dptr(size_wp), K.current_stream()))
            assert np.array_equal(f_idx.cpu().numpy(), px_idx) and np.array_equal(_bits(f_prob.cpu().numpy()), _bits(px_prob)), where
            _check_gather(truth.table(px_idx, n_step), n_step, *_host(x, act, rew, term, disc),
                          where + ("hb_per_sample_gather", n_step))
        rings.assert_intact(where)
        # ---- write-back, duplicates among the indices
        wb = PC.writeback_indices(idx)
        assert len(set(wb.tolist())) < len(wb)
        buf.update_priorities_dev(_cuda(wb), _cuda(rd.td))
        per.update(wb, rd.td, PC.ALPHA)
        ref.update(wb, rd.td)
        _check_tree(buf, per, ref, where + ("write-back",))
        assert buf.max_priority == per.max_priority == ref.max_priority, where
        assert buf.min_priority == per.min_priority == ref.min_priority, where
    assert buf.sum_tree.error_count() == 0


def test_set_ring_argument_checks():
    import hanabi_hip
    from hanabi_hip import _capi as K

    tree = hanabi_hip.SumTree(1000)
    L_ = K.lib()
    assert tree.capacity == 1024 and tree.ring_capacity == 1024
    assert L_.hb_tree_set_ring(tree.h, 0) < 0 and b"ring_capacity" in L_.hb_last_error()
    assert L_.hb_tree_set_ring(tree.h, 1025) < 0 and b"ring_capacity" in L_.hb_last_error()
    tree.set_ring_capacity(1000)
    import torch

    v = torch.tensor([0.6], device="cuda")
    assert L_.hb_tree_fill_range(tree.h, 1000, 4, K.dptr(v), K.current_stream()) < 0 and b"start out of range" in L_.hb_last_error()
    tree.fill_range_dev(990, 5000, v)          # n is clipped to the ring: every slot once, nothing past it
    leaves = tree.nodes().cpu().numpy()[1024:]
    assert (leaves[:1000] == np.float32(0.6)).all() and (leaves[1000:] == 0).all()
    tree.set_ring_capacity(1024)               # and back: the tree's own range again
    tree.fill_range_dev(1020, 8, v)
    assert (tree.nodes().cpu().numpy()[1024 + 1000:] == np.array([0] * 20 + [0.6] * 4, np.float32)).all()


# ---- b. the agent's other insert paths ------------------------------------------------------------------------------------------
def _agent(cap, n, obs_len, n_act):
    from hanabi_agents.rlax_dqn import ActionSpec, DQNAgent, ObservationSpec, RlaxRainbowParams

    params = RlaxRainbowParams(train_batch_size=64, experience_buffer_size=cap, mask_terminal=True)
    return DQNAgent(ObservationSpec((n, obs_len)), ActionSpec(n_act), params, device="cuda")


def _agent_rows(rng, n, obs_len, n_act):
    obs = (rng.random((n, obs_len)) < 0.4).astype(np.int8)
    legal = (rng.random((n, n_act)) < 0.6).astype(np.int8)
    return obs, legal, rng.integers(0, n_act, n).astype(np.int32), rng.standard_normal(n).astype(np.float32), \
        np.where(rng.random(n) < 0.2, 2, 1).astype(np.int8)


@pytest.mark.parametrize("cached", [True, False], ids=["cached_call", "fresh_call"])
def test_add_experience_dense_straddles_the_ring_end(cached):
    """Ring 1000, 300 rows per call: the fourth call starts at slot 900 and ends at slot 200 (hb_replay_insert). cached: the
    caller's buffers stay where they are, so calls 2-4 take the remembered-call branch; otherwise every call is a fresh one."""
    import torch

    cap, n, obs_len, n_act = 1000, 300, 658, 20
    a = _agent(cap, n, obs_len, n_act)
    buf = a.experience
    assert buf.capacity == cap and buf.sum_tree.ring_capacity == cap and buf.sum_tree.capacity == 1024
    per, ref, rng = PerOracle(cap, PC.ALPHA), PC.RingTree(cap), np.random.default_rng(5)
    first = _agent_rows(rng, n, obs_len, n_act)
    hold = [torch.empty_like(_cuda(t)) for t in first]
    a.add_experience_first((None, (_cuda(first[0]), _cuda(first[1]))), torch.zeros(n, dtype=torch.int8, device="cuda"))
    last, want, alive = first[0], {}, []
    for call in range(5):
        rows = _agent_rows(rng, n, obs_len, n_act)
        dev = hold if cached else [torch.empty_like(h) for h in hold]
        alive.append(dev)      # (kept, so that no later call's buffers land on an earlier call's addresses)
        for d, t in zip(dev, rows):
            d.copy_(_cuda(t))
        remembered = a._dense_call is not None and a._dense_call[0][0] == dev[0].data_ptr()
        assert remembered == (cached and call > 0), call
        a.add_experience_dense((None, (dev[0], dev[1])), dev[2], dev[3], dev[4])
        slots = per.insert(n)
        ref.insert(n)
        for g, s in enumerate(slots):
            want[s] = (last[g], rows[0][g], rows[1][g], rows[2][g], rows[3][g], rows[4][g] == 2)
        last = rows[0]
        assert (buf.oldest_entry, buf.size) == (per.oldest, per.size)
        _check_tree(buf, per, ref, ("call", call))
    assert per.oldest == 500 and per.size == cap      # calls 4 and 5 passed the ring's end resp. started behind it
    tr = buf[np.arange(cap)]
    for s, (o1, o2, lg, ac, rw, tm) in want.items():
        assert np.array_equal(tr.observation_tm1[s], o1) and np.array_equal(tr.observation_t[s], o2), s
        assert np.array_equal(tr.legal_moves_t[s], lg) and tr.action_tm1[s, 0] == ac and tr.terminal_t[s, 0] == tm, s
        assert np.float32(tr.reward_t[s, 0]) == rw, s


def test_add_transitions_dense_straddles_the_ring_end():
    """hb_obl_insert: calls of 300, 7 and 96 rows in turn into a ring of 1000; the tree's leaves follow the rows round the end."""
    cap, obs_len, n_act = 1000, 658, 20
    a = _agent(cap, 300, obs_len, n_act)
    buf = a.experience
    per, ref, rng, want, wrapped = PerOracle(cap, PC.ALPHA), PC.RingTree(cap), np.random.default_rng(6), {}, 0
    for call in range(9):
        n = (300, 7, 96)[call % 3]
        o1, lg, ac, rw, st = _agent_rows(rng, n, obs_len, n_act)
        o2 = _agent_rows(rng, n, obs_len, n_act)[0]
        wrapped += per.oldest + n > cap
        a.add_transitions_dense(_cuda(o1), _cuda(ac), _cuda(rw[None, :]), _cuda((st == 2).astype(np.int8)[None, :]), _cuda(o2), _cuda(lg))
        for g, s in enumerate(per.insert(n)):
            tm = bool(st[g] == 2)        # an ended branch has no next observation and no legal move
            want[s] = (o1[g], np.zeros_like(o2[g]) if tm else o2[g], np.zeros_like(lg[g]) if tm else lg[g], ac[g], rw[g], tm)
        ref.insert(n)
        assert (buf.oldest_entry, buf.size) == (per.oldest, per.size)
        _check_tree(buf, per, ref, ("call", call))
    assert wrapped == 1 and per.size == cap
    tr = buf[np.arange(cap)]
    for s, (o1, o2, lg, ac, rw, tm) in want.items():
        assert np.array_equal(tr.observation_tm1[s], o1) and np.array_equal(tr.observation_t[s], o2), s
        assert np.array_equal(tr.legal_moves_t[s], lg) and tr.action_tm1[s, 0] == ac and tr.terminal_t[s, 0] == tm, s
        assert np.float32(tr.reward_t[s, 0]) == rw, s


# ---- c. whole sessions -------------------------------------------------------------------------------------------------------
def _session_run(cap, path):
    import torch

    import hanabi_hip
    from hanabi_agents.rlax_dqn import ActionSpec, DQNAgent, ObservationSpec, RlaxRainbowParams
    from hanabi_hip.selfplay import SelfPlaySession

    n = 130
    torch.manual_seed(0)
    flags = hanabi_hip.FLAG_AUTO_RESET | hanabi_hip.FLAG_RESET_START_NEXT
    env = hanabi_hip.HanabiEnv(config=hanabi_hip.make_config("Hanabi-Small", 2, flags), n_games=n, seed=9, packed=True)
    params = RlaxRainbowParams(train_batch_size=64, experience_buffer_size=cap, layers=[512], compute_dtype="bfloat16",
                               use_priority=True, mask_terminal=True, target_update_period=6, packed_obs=True)
    agents = [DQNAgent(ObservationSpec((n, env.obs_len)), ActionSpec(env.num_actions), params._replace(seed=40 + s), device="cuda")
              for s in (0, 1)]
    kw = dict(plain=dict(split_update=False, native_chain=False), split=dict(native_chain=False), chain={})[path]
    sess = SelfPlaySession(env, agents, **kw)
    for _ in range(40):
        sess.step()
    sess.flush()
    torch.cuda.synchronize()
    assert env.illegal_count() == 0 and sess.grad_steps > 20
    assert all(bool(a.split_update) == (path != "plain") for a in agents)
    assert (sess.native_steps > 0) == (path == "chain"), sess.native_steps
    out = []
    for a in agents:
        buf = a.experience
        assert not a._pending_fills and buf.capacity == cap and buf.size == cap      # 20 inserts of 130 rows: 2.6 laps
        T = buf.sum_tree.capacity
        nodes = buf.sum_tree.nodes().cpu().numpy()
        leaves = nodes[T:]
        assert (leaves[cap:] == 0).all(), (path, np.flatnonzero(leaves[cap:])[:8] + cap)
        assert (leaves[:buf.size] > 0).all(), path
        assert np.array_equal(_bits(nodes[1:T]), _bits(nodes[2:2 * T:2] + nodes[3:2 * T:2])), path
        idx = a._g_idx.cpu().numpy()
        assert len(idx) == 64 and ((idx >= 0) & (idx < cap)).all(), (path, idx)
        assert buf.sum_tree.error_count() == 0
        out.append((nodes, buf._obs_t_buf.cpu().numpy(), buf._act_tm1_buf.cpu().numpy(),
                    torch.cat([p.detach().reshape(-1) for p in a.online.parameters()]).cpu().numpy()))
    return out


@pytest.mark.parametrize("cap", [1000, 1024], ids=["ring1000", "ring1024_control"])
def test_sessions_keep_the_tree_inside_the_ring(cap, monkeypatch):
    """Hanabi-Small, 2 players, 130 games, ring 1000 (130 does not divide it: every lap straddles) and 1024 (the control), 40
    steps = 2.6 laps per agent, through the plain update, the split update (queued fills) and the one-call step (the chain's
    fill command). After the session: no leaf past the ring is live, every leaf of a written slot is, every inner node is the
    sum of its children, the learner's last batch lies in the ring. The one-call step and the split update it replays leave
    identical trees, rings and weights (as tests/test_selfplay.py requires of them on 2^k rings)."""
    monkeypatch.setenv("HB_ACTOR_FUSED_MIN_ROWS", "0")
    runs = {path: _session_run(cap, path) for path in ("plain", "split", "chain")}
    for seat, (x, y) in enumerate(zip(runs["split"], runs["chain"])):
        for k, (p, q) in enumerate(zip(x, y)):
            assert np.array_equal(p, q), (cap, seat, k, "split update and one-call step differ")


# ---- d. checkpoints -----------------------------------------------------------------------------------------------------------
def test_checkpoint_round_trip_and_a_stale_heap():
    """state_dict / load_state_dict of a ring of 1000 keeps the heap bit for bit. A heap saved by a build whose fill wrapped at
    the tree's size carries live leaves past the ring: loading it drops them and re-sums every inner node."""
    import torch

    from hanabi_agents.rlax_dqn.priority_buffer import PriorityBuffer

    cap, n, T = 1000, 96, 1024
    rng = np.random.default_rng(7)
    buf = PriorityBuffer(L, A, 1, cap, alpha=PC.ALPHA, device="cuda")
    per, ref = PerOracle(cap, PC.ALPHA), PC.RingTree(cap)
    for r in range(12):       # 1152 rows: the 11th insert straddles
        obs, legal, action, reward = RC.make_rows(rng, n, L, A)
        buf.add_transitions(_cuda(obs), _cuda(action.reshape(-1, 1)), _cuda(reward.reshape(-1, 1)), _cuda(obs), _cuda(legal),
                            _cuda(np.zeros((n, 1), bool)))
        per.insert(n)
        ref.insert(n)
        idx = rng.integers(0, per.size, 64)
        td = rng.standard_normal(64).astype(np.float32)
        buf.update_priorities_dev(_cuda(idx), _cuda(td))
        per.update(idx, td, PC.ALPHA)
        ref.update(idx, td)
    clean = _check_tree(buf, per, ref, "before saving")
    sd = buf.state_dict()
    assert np.array_equal(_bits(sd["tree_nodes"].numpy()), _bits(clean))
    fresh = PriorityBuffer(L, A, 1, cap, alpha=PC.ALPHA, device="cuda")
    fresh.load_state_dict(sd)
    assert (fresh.oldest_entry, fresh.size) == (per.oldest, per.size) and fresh.max_priority == per.max_priority
    _check_tree(fresh, per, ref, "after the round trip")
    # the stale heap: leaves 1000 .. 1023 live, inner nodes consistent with them, as the old fill left it
    stale = clean.copy()
    stale[T + cap:] = rng.random(T - cap).astype(np.float32) + np.float32(0.1)
    w = T // 2
    while w >= 1:
        stale[w:2 * w] = stale[2 * w:4 * w:2] + stale[2 * w + 1:4 * w:2]
        w //= 2
    assert per.heap_violations(stale) == dict(out_of_ring=T - cap, leaf=0, inner=0) and stale[1] != clean[1]
    sd2 = dict(sd, tree_nodes=torch.as_tensor(stale))
    old = PriorityBuffer(L, A, 1, cap, alpha=PC.ALPHA, device="cuda")
    old.load_state_dict(sd2)
    _check_tree(old, per, ref, "after loading the stale heap")
    u = rng.random(64) / 64
    u[-1] = 0.0
    idx = old.sum_tree.per_sample_dev(_cuda(u))[0].cpu().numpy()
    assert (idx < cap).all() and np.array_equal(idx, ref.sample(u)[0])
