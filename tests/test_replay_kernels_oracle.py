"""GPU: hb_replay_insert, hb_replay_gather, hb_replay_gather_packed, hb_per_sample_gather (C ABI, hanabi_hip._capi) and the
torch fallback ExperienceBuffer(device="cuda").gather_nstep_dev against the trajectory oracle (oracle/replay_oracle.py), over
the case table of tests/replay_cases.py. The oracle knows games, not slots: a chain's successors are the next transitions of
the same game. Observations, actions and terminal flags are exact; rew and disc meet the two bounds derived in
replay_cases.check_rew_disc (bit-equal for n_step == 1). No sample is filtered and nothing is retried."""
import numpy as np
import pytest

import replay_cases as RC
from oracle.replay_oracle import ReplayOracle

pytestmark = pytest.mark.gpu

DT = {"f32": 0, "bf16": 1, "f16": 2}
SENT = dict(obs=0x55, act=-3, lms=9, rew=-77.5, term=5)   # what the rings hold before anything is written


def _torch_dtype(name):
    import torch

    return {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[name]


def _cuda(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


class GpuRing:
    """Six rings and last_obs as plain device tensors full of sentinels, written only by hb_replay_insert."""

    def __init__(self, cap, n, L, A, packed, first_obs):
        import torch

        self.cap, self.n, self.L, self.A, self.packed = cap, n, L, A, packed
        self.form = (lambda a: RC.pack_rows(a, L)) if packed else (lambda a: a)
        row, odt, fill = (RC.words_for(L), torch.int32, 0x55555555) if packed else (L, torch.int8, SENT["obs"])
        self.row_bytes = 4 * row if packed else L
        self.obs_tm1 = torch.full((cap, row), fill, dtype=odt, device="cuda")
        self.obs_t = torch.full((cap, row), fill, dtype=odt, device="cuda")
        self.act = torch.full((cap, 1), SENT["act"], dtype=torch.int8, device="cuda")
        self.lms = torch.full((cap, A), SENT["lms"], dtype=torch.int8, device="cuda")
        self.rew = torch.full((cap, 1), SENT["rew"], dtype=torch.float32, device="cuda")
        self.term = torch.full((cap, 1), SENT["term"], dtype=torch.uint8, device="cuda")
        self.last_obs = _cuda(self.form(first_obs))

    def insert(self, start, obs, legal, action, reward, st):
        from hanabi_hip import _capi as K

        args = [_cuda(self.form(obs)), _cuda(legal), _cuda(action), _cuda(reward), _cuda(st)]
        K.check(K.lib().hb_replay_insert(K.dptr(self.last_obs), *(K.dptr(a) for a in args), K.dptr(self.obs_tm1), K.dptr(self.obs_t),
                                         K.dptr(self.act), K.dptr(self.lms), K.dptr(self.rew), K.dptr(self.term), obs.shape[0],
                                         self.row_bytes, self.A, self.cap, start, K.current_stream()))

    def host(self):
        return dict(obs_tm1=self.obs_tm1.cpu().numpy(), obs_t=self.obs_t.cpu().numpy(), act=self.act.cpu().numpy(),
                    lms=self.lms.cpu().numpy(), rew=self.rew.cpu().numpy(), term=self.term.cpu().numpy(),
                    last_obs=self.last_obs.cpu().numpy())

    def assert_equals(self, got, ring, where):
        """Byte-equal to the oracle's ring where a slot has been written, still the sentinel elsewhere."""
        w = ring["written"]
        for key in ("obs_tm1", "obs_t", "act", "lms", "rew", "term"):
            want = self.form(ring[key]) if key.startswith("obs") else ring[key]
            g = got[key]
            assert np.array_equal(g[w].view(np.uint8), np.ascontiguousarray(want[w]).astype(g.dtype).view(np.uint8)), (where, key)
            sent = np.full_like(g[~w], 0x55555555 if g.dtype == np.int32 else SENT["obs" if key.startswith("obs") else key])
            assert np.array_equal(g[~w], sent), (where, key, "a slot nobody wrote has changed")
        assert np.array_equal(got["last_obs"], self.form(ring["last_obs"])), (where, "last_obs")


def _filled(case, upto, check=False):
    """A GpuRing after the case's first `upto` inserts, the oracle fed the same rows. check: compare after every insert."""
    first, inserts = RC.case_inputs(case)
    ring, orc = GpuRing(case.cap, case.n_ins, case.L, case.A, case.packed, first), ReplayOracle(case.cap, first)
    before = ring.host() if check else None
    for k in range(upto):
        ring.insert(orc.write_pointer, *inserts[k])
        written = orc.insert(*inserts[k])
        if check:
            got, keep = ring.host(), np.ones(case.cap, bool)
            ring.assert_equals(got, orc.expected_ring(), (case.name, k))
            keep[written] = False
            for key in ("obs_tm1", "obs_t", "act", "lms", "rew", "term"):
                assert np.array_equal(got[key][keep], before[key][keep]), (case.name, k, key, "a slot outside the insert changed")
            before = got
    return ring, orc


# ---- hb_replay_insert ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in RC.CASES])
def test_insert_stream_matches_oracle_after_every_insert(name):
    """Int8 and packed row forms; partly filled, exactly full, wrapped mid-batch, several laps: after EVERY insert all six rings
    and last_obs are byte-equal to the oracle's and the slots that insert did not write are unchanged."""
    case = RC.BY_NAME[name]
    _, orc = _filled(case, max(case.states), check=True)
    assert orc.n_inserts == max(case.states)


@pytest.mark.parametrize("ic", RC.INSERT_CASES, ids=lambda c: c.name)
def test_insert_shapes(ic):
    """One insert at a chosen start: byte counts that are no multiple of 16, a wrap whose second segment starts unaligned, a
    whole-ring insert, the last slot, one row, more chunks than the grid has threads, the packed call form."""
    rng = np.random.default_rng(ic.cap * 31 + ic.start)
    first = RC.make_rows(rng, ic.n, ic.L, ic.A)[0]
    rows = RC.make_rows(rng, ic.n, ic.L, ic.A) + (rng.integers(0, 3, ic.n).astype(np.int8),)
    ring, orc = GpuRing(ic.cap, ic.n, ic.L, ic.A, ic.packed, first), ReplayOracle(ic.cap, first, first_slot=ic.start)
    ring.insert(ic.start, *rows)
    orc.insert(*rows)
    exp = orc.expected_ring()
    assert exp["written"].sum() == ic.n
    ring.assert_equals(ring.host(), exp, ic.name)


# ---- hb_replay_gather / hb_replay_gather_packed ----------------------------------------------------------------------------
def _check_outputs(case, exp, ring_rew, sel, x, act, rew, term, disc, n_step, where):
    """x [nb, 2B, x_ld] float32, the rest [nb, B], all numpy; sel [nb, B] the gathered slots."""
    B, L = sel.shape[1], case.L
    assert np.array_equal(x[:, :B, :L], exp["obs_tm1"][sel].astype(np.float32)), (where, "obs_tm1 rows")
    assert np.array_equal(x[:, B:, :L], exp["obs_t"][sel].astype(np.float32)), (where, "obs_t rows")
    assert (x[:, :, L:] == RC.X_SENTINEL).all(), (where, "padding columns were written")
    assert np.array_equal(act, exp["act"][sel]), (where, "act")
    assert np.array_equal(term, exp["term"][sel].astype(np.float32)), (where, "term")
    return RC.check_rew_disc(rew.reshape(-1), disc.reshape(-1), exp, sel.reshape(-1), n_step, case.gamma, ring_rew, where)


@pytest.mark.parametrize("name", [c.name for c in RC.CASES])
def test_gather_matches_oracle(name):
    """Every slot in range(size) (plus repeats, in batches of B), n_step 1 / 2 / 3 / 5, at every ring state of the case."""
    import torch

    from hanabi_hip import _capi as K

    case, scen = RC.BY_NAME[name], RC.scenario(name)
    first, inserts = RC.case_inputs(case)
    ring, orc = GpuRing(case.cap, case.n_ins, case.L, case.A, case.packed, first), ReplayOracle(case.cap, first)
    fn = K.lib().hb_replay_gather_packed if case.packed else K.lib().hb_replay_gather
    B, worst = case.B, [0.0, 0.0]
    for k, ins in enumerate(inserts):
        ring.insert(orc.write_pointer, *ins)
        orc.insert(*ins)
        if k + 1 not in scen:
            continue
        s = scen[k + 1]
        size = s["ring"]["size"]
        assert (size, s["ring"]["write_pointer"]) == (orc.size, orc.write_pointer)
        size_wp = torch.tensor([size, orc.write_pointer], dtype=torch.int64, device="cuda")
        sel = RC.index_batches(case, size, k + 1)
        idx, nb = _cuda(sel), sel.shape[0]
        for dname in case.dtypes:
            for n in RC.N_STEPS:
                x = torch.full((nb, 2 * B, case.x_ld), RC.X_SENTINEL, dtype=_torch_dtype(dname), device="cuda")
                act = torch.full((nb, B), -1, dtype=torch.int32, device="cuda")
                rew, term, disc = (torch.full((nb, B), float("nan"), device="cuda") for _ in range(3))
                for b in range(nb):
                    K.check(fn(K.dptr(ring.obs_tm1), K.dptr(ring.obs_t), K.dptr(ring.act), K.dptr(ring.rew), K.dptr(ring.term),
                               K.dptr(idx[b]), B, case.L, K.dptr(x[b]), DT[dname], case.x_ld, K.dptr(act[b]), K.dptr(rew[b]),
                               K.dptr(term[b]), K.dptr(disc[b]), n, case.gamma, case.cap, case.n_ins, K.dptr(size_wp),
                               K.current_stream()))
                d, r = _check_outputs(case, s["nstep"][n], s["ring"]["rew"], sel, x.float().cpu().numpy(), act.cpu().numpy(),
                                      rew.cpu().numpy(), term.cpu().numpy(), disc.cpu().numpy(), n, (name, k + 1, dname, n))
                worst = [max(worst[0], d), max(worst[1], r)]
    print(f"{name}: worst error / bound: disc {worst[0]:.3f}, rew {worst[1]:.3f}")


# ---- hb_per_sample_gather ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pc", [p._replace(lazy=(lz,)) for p in RC.PSG_CASES for lz in p.lazy],
                         ids=lambda p: f"{p.case}-s{p.state}-B{p.B}-n{p.n_step}-{'lazy' if p.lazy[0] else 'eager'}")
def test_per_sample_gather_matches_oracles(pc):
    """idx / prob bit-equal to OracleTree.per_sample on the Philox uniforms rebuilt on the host; everything gathered at those
    indices against the trajectory oracle. tests/test_replay_oracle_cpu.py shows that every such index is a written slot."""
    import torch

    import hanabi_hip
    from hanabi_hip import _capi as K

    case, lazy = RC.BY_NAME[pc.case], pc.lazy[0]
    s = RC.scenario(pc.case)[pc.state]
    size, B = s["ring"]["size"], pc.B
    ring, orc = _filled(case, pc.state)
    otree = RC.psg_oracle_tree(pc, size)
    tree = hanabi_hip.SumTree(case.cap)
    assert tree.capacity == otree.cap and (not lazy or tree.capacity > 1024)
    if lazy:
        tree.set_lazy_top(True)   # before the writes: they leave the levels above the 1024-leaf chunks stale
    tree.fill_range_dev(0, size, torch.tensor([0.6], device="cuda"))
    p_idx, p_val = RC.psg_priorities(pc, size)
    tree.update_dev(_cuda(p_idx), _cuda(p_val))
    size_wp = torch.tensor([size, orc.write_pointer], dtype=torch.int64, device="cuda")
    dname = case.dtypes[0]
    for counter in RC.PSG_COUNTERS:
        want_idx, want_prob = otree.per_sample(RC.philox_uniforms(pc.seed, counter, B))
        assert (want_idx < size).all()
        c = torch.tensor(counter, dtype=torch.float32, device="cuda")
        idx = torch.full((B,), -1, dtype=torch.int64, device="cuda")
        prob = torch.zeros(B, dtype=torch.float64, device="cuda")
        x = torch.full((1, 2 * B, case.x_ld), RC.X_SENTINEL, dtype=_torch_dtype(dname), device="cuda")
        act = torch.full((1, B), -1, dtype=torch.int32, device="cuda")
        rew, term, disc = (torch.full((1, B), float("nan"), device="cuda") for _ in range(3))
        K.check(K.lib().hb_per_sample_gather(tree.h, pc.seed, K.dptr(c), B, K.dptr(idx), K.dptr(prob), K.dptr(ring.obs_tm1),
                                             K.dptr(ring.obs_t), K.dptr(ring.act), K.dptr(ring.rew), K.dptr(ring.term), case.L,
                                             1 if case.packed else 0, K.dptr(x), DT[dname], case.x_ld, K.dptr(act), K.dptr(rew),
                                             K.dptr(term), K.dptr(disc), pc.n_step, case.gamma, case.cap, case.n_ins,
                                             K.dptr(size_wp), K.current_stream()))
        got_idx = idx.cpu().numpy()
        assert np.array_equal(got_idx, want_idx), (counter, got_idx, want_idx)
        assert np.array_equal(prob.cpu().numpy().view(np.uint64), want_prob.view(np.uint64)), counter
        _check_outputs(case, s["nstep"][pc.n_step], s["ring"]["rew"], want_idx[None, :], x.float().cpu().numpy(), act.cpu().numpy(),
                       rew.cpu().numpy(), term.cpu().numpy(), disc.cpu().numpy(), pc.n_step, (pc, counter))
    if lazy:
        tree.set_lazy_top(False)
        assert tree.get_total_val() == otree.total()


# ---- the torch fallback on the device ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in RC.CASES])
def test_torch_fallback_on_device_matches_oracle(name):
    """ExperienceBuffer(device="cuda").add_transitions / gather_nstep_dev on the same table rows: the third implementation of
    the walk against the same reference."""
    import torch

    from hanabi_agents.rlax_dqn.experience_buffer import ExperienceBuffer

    case, scen = RC.BY_NAME[name], RC.scenario(name)
    first, inserts = RC.case_inputs(case)
    buf = ExperienceBuffer(case.L, case.A, 1, case.cap, device="cuda", packed=case.packed)
    form = (lambda a: RC.pack_rows(a, case.L)) if case.packed else (lambda a: a)
    last = first
    for k, (obs, legal, action, reward, st) in enumerate(inserts):
        buf.add_transitions(_cuda(last), _cuda(action.reshape(-1, 1)), _cuda(reward.reshape(-1, 1)), _cuda(obs), _cuda(legal),
                            _cuda((st == 2).reshape(-1, 1)))
        last = obs
        if k + 1 not in scen:
            continue
        s = scen[k + 1]
        ring, size = s["ring"], s["ring"]["size"]
        assert (buf.size, buf.oldest_entry) == (size, ring["write_pointer"])
        w = ring["written"]
        for attr, key in (("_obs_tm1_buf", "obs_tm1"), ("_obs_t_buf", "obs_t"), ("_act_tm1_buf", "act"), ("_lms_t_buf", "lms"),
                          ("_rew_t_buf", "rew"), ("_terminal_t_buf", "term")):
            want = form(ring[key]) if key.startswith("obs") else ring[key]
            assert np.array_equal(getattr(buf, attr).cpu().numpy()[w], want[w]), (name, k + 1, key)
        idx = torch.arange(size, device="cuda")
        for n in RC.N_STEPS:
            exp, where = s["nstep"][n], (name, k + 1, n)
            tr, disc = buf.gather_nstep_dev(idx, n, case.gamma)
            assert np.array_equal(tr.observation_tm1.cpu().numpy(), exp["obs_tm1"]), where
            assert np.array_equal(tr.observation_t.cpu().numpy(), exp["obs_t"]), where
            assert np.array_equal(tr.legal_moves_t.cpu().numpy(), exp["legal"]), where
            assert np.array_equal(tr.action_tm1.cpu().numpy()[:, 0], exp["act"]), where
            assert np.array_equal(tr.terminal_t.cpu().numpy()[:, 0], exp["term"]), where
            RC.check_rew_disc(tr.reward_t.cpu().numpy()[:, 0], disc.cpu().numpy(), exp, np.arange(size), n, case.gamma, ring["rew"], where)
