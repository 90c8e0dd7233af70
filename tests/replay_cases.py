"""The one case table of the replay tests (tests/test_replay_oracle_cpu.py on the host, tests/test_replay_kernels_oracle.py on
the GPU) and the helpers both share: the inputs of a case, the trajectory oracle's answers for it (computed once per process
and never modified), numpy bit-packing, the host-side Philox uniforms and the two derived error bounds.

Every shape is small and is there for a reason:

* row length L: 1; 31 / 32 / 33 (the packed row's last word is partly used, exactly full, one bit into the next); 171 (shorter
  than the gathers' 256-thread stride); 658 (longer than it; once with x_ld = 704, the padded GEMM operand);
* action count A: 11, 20, 48;
* ring (capacity, rows per insert): (40, 8) a multiple; (37, 5) not a multiple: every insert after the 7th wraps mid-batch and
  the oldest insert is partly overwritten; (8, 8) capacity == insert size: the successor slot would be the slot itself;
  (16, 8); (2000, 48): tree capacity 2048 = two 1024-leaf chunks, so the tree's lazy top levels are real;
* ring states (the `states` of a case are insert counts, all reached by real inserts in one stream): partly filled after 1, 2
  and 3 inserts; exactly full with the write pointer at 0; wrapped with the write pointer mid-ring; wrapped several laps;
* n_step 1, 2, 3, 5 on every case; gamma 0.99, 0.9, 1.0; float32 rewards that are not integers;
* terminals by hand (`step_types`): game 0 every fourth insert (so a chain meets it at its first, middle and last step), game 1
  on two consecutive inserts, game 2 in the newest insert of every state, game 3 never; random ones on the other games;
* gather batches B 1, 5, 64 over every slot in range(size) plus repeats (`index_batches`).
"""
import collections
import functools

import numpy as np

from oracle.replay_oracle import ReplayOracle

N_STEPS = (1, 2, 3, 5)
U = 2.0 ** -24          # unit roundoff of float32
X_SENTINEL = 7.0        # written into the whole x operand before a gather: columns L..x_ld must still hold it afterwards

Case = collections.namedtuple("Case", "name cap n_ins L x_ld A packed dtypes gamma B states arbitrary")


def _c(name, ring, L, A, packed, dtypes, gamma, B, states, x_ld=None, arbitrary=False):
    return Case(name, ring[0], ring[1], L, x_ld or L, A, packed, tuple(dtypes), gamma, B, tuple(states), arbitrary)


# states: (40, 8): 5 inserts = exactly full, wp 0; 7: wp 16; 23: 4.6 laps, wp 24.   (37, 5): 7 = 35 of 37 slots; 8: the first
# wrap, mid-batch, wp 3; 20: 2.7 laps, wp 26; 37: five laps, wp back at 0.   (8, 8): full with wp 0 after every insert.
# (16, 8): 2 = full, wp 0; 3: wp 8; 7: laps.   (2000, 48): 41 = 1968 slots; 42: wrapped mid-batch, wp 16; 46: wp 208.
CASES = (
    _c("m40_i8_L658_pad", (40, 8), 658, 20, False, ["bf16"], 0.99, 64, (1, 2, 3, 5, 7, 23), x_ld=704),
    _c("m40_pk_L658", (40, 8), 658, 20, True, ["f16"], 0.99, 5, (1, 2, 3, 5, 7, 23)),
    _c("m40_i8_L33", (40, 8), 33, 11, False, ["f32"], 0.9, 1, (1, 2, 3, 5, 7, 23)),
    _c("o37_i8_L171", (37, 5), 171, 11, False, ["f32"], 0.9, 5, (1, 2, 3, 7, 8, 20, 37)),
    _c("o37_pk_L171", (37, 5), 171, 20, True, ["bf16"], 0.99, 64, (1, 2, 3, 7, 8, 20, 37)),
    _c("o37_pk_L33", (37, 5), 33, 48, True, ["bf16"], 1.0, 64, (1, 2, 3, 7, 8, 20, 37)),
    _c("e8_i8_L1", (8, 8), 1, 11, False, ["f16"], 0.9, 1, (1, 2, 3, 9)),
    _c("e8_pk_L31", (8, 8), 31, 20, True, ["f32"], 0.99, 5, (1, 2, 3, 9)),
    _c("h16_pk_L32", (16, 8), 32, 20, True, ["bf16"], 0.9, 64, (1, 2, 3, 7)),
    _c("h16_pk_L31", (16, 8), 31, 11, True, ["f16"], 1.0, 5, (1, 2, 3, 7)),
    _c("h16_i8_L31_any", (16, 8), 31, 48, False, ["f32", "bf16", "f16"], 0.99, 5, (1, 2, 3, 7), arbitrary=True),
    _c("t2000_i8_L33", (2000, 48), 33, 20, False, ["bf16"], 0.99, 64, (1, 2, 3, 41, 42, 46)),
    _c("t2000_pk_L31", (2000, 48), 31, 11, True, ["f16"], 0.9, 64, (1, 2, 3, 41, 42, 46)),
)
BY_NAME = {c.name: c for c in CASES}

# hb_per_sample_gather: (case, state, B, n_step, seed, lazy-top modes). Partly filled (state 3 and, at the large ring, 41) and
# wrapped rings, int8 and packed, B 1 / 2 / 5 / 64; each runs with the Philox counters PSG_COUNTERS.
PsgCase = collections.namedtuple("PsgCase", "case state B n_step seed lazy")
PSG_COUNTERS = (0.0, 7.0)
PSG_CASES = (
    PsgCase("m40_i8_L33", 3, 1, 3, 0x1234ABCD5, (False,)),
    PsgCase("o37_pk_L171", 20, 2, 1, 99, (False,)),
    PsgCase("h16_pk_L31", 3, 5, 3, 0xABCDEF12345, (False,)),
    PsgCase("m40_i8_L658_pad", 7, 64, 3, 5, (False,)),
    PsgCase("e8_i8_L1", 2, 2, 1, 17, (False,)),
    PsgCase("t2000_pk_L31", 3, 64, 3, 31, (False, True)),
    PsgCase("t2000_i8_L33", 41, 5, 1, 77, (False, True)),
    PsgCase("t2000_i8_L33", 46, 64, 3, 2024, (False, True)),
)

# hb_replay_insert alone: (name, capacity, rows, row length, A, start, packed). One insert into a ring of sentinels.
InsertCase = collections.namedtuple("InsertCase", "name cap n L A start packed")
INSERT_CASES = (
    InsertCase("bytes_not_x16", 37, 5, 33, 11, 0, False),              # 165 bytes: ten 16-byte chunks and a 5-byte tail
    InsertCase("wrap_unaligned_2nd_segment", 37, 5, 33, 20, 35, False),  # rows 0-1 at byte 1155, rows 2-4 from batch byte 66
    InsertCase("n_eq_cap_from_0", 8, 8, 31, 20, 0, False),
    InsertCase("n_eq_cap_wrapping", 8, 8, 31, 48, 3, False),
    InsertCase("start_last_slot", 40, 8, 171, 11, 39, False),
    InsertCase("one_row_L658", 16, 1, 658, 20, 15, False),
    InsertCase("one_row_L1", 16, 1, 1, 11, 7, False),
    InsertCase("under_16_bytes", 16, 8, 1, 11, 12, False),             # no 16-byte chunk at all in either segment
    # 12 800 x 658 bytes = 526 400 chunks > 2048 workgroups x 256 threads: the grid-stride loop takes a second turn
    InsertCase("grid_cap", 12800, 12800, 658, 20, 5, False),
    InsertCase("packed_rows", 37, 5, 171, 20, 35, True),                # row bytes = 4 * 6 words
)


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def words_for(L):
    return (L + 31) // 32


def pack_rows(obs, L):
    """[n, L] 0/1 -> [n, ceil(L/32)] int32: element i = bit (i & 31) of word i >> 5, pad bits zero."""
    n, w = obs.shape[0], words_for(L)
    bits = np.zeros((n, w * 32), np.uint8)
    bits[:, :L] = obs != 0
    return np.packbits(bits, axis=1, bitorder="little").view("<u4").astype(np.uint32).view(np.int32).reshape(n, w)


def step_types(k, n_ins, states, rng):
    """dm_env step types of insert k's rows (0 FIRST never ends anything, 1 MID, 2 LAST = terminal)."""
    st = np.where(rng.random(n_ins) < 0.2, 2, rng.integers(0, 2, n_ins)).astype(np.int8)
    hand = {0: k % 4 == 2, 1: k % 6 in (3, 4), 2: (k + 1) in states, 3: False}
    for g, terminal in hand.items():
        if g < n_ins:
            st[g] = 2 if terminal else 1
    return st


def make_rows(rng, n, L, A, arbitrary=False):
    obs = rng.integers(-128, 128, (n, L)).astype(np.int8) if arbitrary else (rng.random((n, L)) < 0.4).astype(np.int8)
    legal = (rng.random((n, A)) < 0.6).astype(np.int8)
    action = rng.integers(0, A, n).astype(np.int32)
    reward = (rng.standard_normal(n) * 1.5).astype(np.float32)
    reward[rng.random(n) < 0.2] = 1.0    # and some of the game's own integer rewards
    return obs, legal, action, reward


def case_inputs(case):
    """(first_obs, [insert 0, insert 1, ...]); an insert is (obs, legal, action, reward, step_type), all numpy."""
    rng = np.random.default_rng(sum(case.name.encode()) * 1000 + case.cap)
    first = make_rows(rng, case.n_ins, case.L, case.A, case.arbitrary)[0]
    inserts = []
    for k in range(max(case.states)):
        inserts.append(make_rows(rng, case.n_ins, case.L, case.A, case.arbitrary) + (step_types(k, case.n_ins, case.states, rng),))
    return first, inserts


def index_batches(case, size, state):
    """Every slot in range(size) and at least one batch worth of repeats, shuffled, as [batches, B] int64."""
    rng = np.random.default_rng(state * 7919 + case.cap)
    total = (size + case.B - 1) // case.B * case.B + case.B
    idx = np.concatenate([np.arange(size), rng.integers(0, size, total - size)])
    rng.shuffle(idx)
    return idx.reshape(-1, case.B).astype(np.int64)


# ---- the oracle's answers, once ------------------------------------------------------------------------------------------
def nstep_table(orc, size, n_step, gamma):
    """The oracle's n-step transition of every slot in range(size), as arrays over the slot."""
    rows = [orc.nstep(s, n_step, gamma) for s in range(size)]
    return dict(R=np.array([r["R"] for r in rows]), S=np.array([r["S"] for r in rows]), m=np.array([r["m"] for r in rows]),
                disc=np.array([r["disc"] for r in rows]), term=np.array([r["terminal"] for r in rows]),
                act=np.array([r["action"] for r in rows]), obs_tm1=np.stack([r["obs_tm1"] for r in rows]),
                obs_t=np.stack([r["obs_t"] for r in rows]), legal=np.stack([r["legal"] for r in rows]),
                last=[r["last"] for r in rows])


@functools.lru_cache(maxsize=None)
def scenario(name):
    """{state: dict(ring=expected_ring(), holder=[...], nstep={n_step: nstep_table})} of a case. Read-only by convention."""
    case = BY_NAME[name]
    first, inserts = case_inputs(case)
    orc, out = ReplayOracle(case.cap, first), {}
    for k, ins in enumerate(inserts):
        orc.insert(*ins)
        if k + 1 in case.states:
            ring = orc.expected_ring()
            out[k + 1] = dict(ring=ring, holder=list(orc.holder),
                              nstep={n: nstep_table(orc, ring["size"], n, case.gamma) for n in N_STEPS})
    return out


# ---- the two derived bounds ---------------------------------------------------------------------------------------------
def check_rew_disc(rew, disc, exp, sel, n_step, gamma, ring_rew, where):
    """rew / disc: float32 arrays [B] of a gather at slots `sel`; exp: nstep_table. Prints the worst ratio to its bound.

    n_step == 1: nothing is computed, both are bit-equal to float32(gamma) and to the ring's value.
    n_step > 1:  disc is gamma multiplied m - 1 times, one rounding each: |disc - gamma^m| <= m u gamma^m to first order (this
                 also pins the step count m unless gamma == 1). rew: the running discount carries at most m - 1 roundings,
                 each product one more (none if the multiply-add is contracted), each addition one against a partial sum of
                 at most S = sum gamma^i |r_i|: |rew - R| <= 2 n_step u S."""
    rew, disc = np.asarray(rew, np.float32), np.asarray(disc, np.float32)
    if n_step == 1:
        assert np.array_equal(disc.view(np.uint32), np.full(len(sel), gamma, np.float32).view(np.uint32)), where
        assert np.array_equal(rew.view(np.uint32), ring_rew[sel, 0].view(np.uint32)), where
        return 0.0, 0.0
    m, d, R, S = exp["m"][sel], exp["disc"][sel], exp["R"][sel], exp["S"][sel]
    d_err, d_bound = np.abs(disc.astype(np.float64) - d), m * U * d
    r_err, r_bound = np.abs(rew.astype(np.float64) - R), 2 * n_step * U * S
    assert (d_err <= d_bound).all(), (where, "disc", float((d_err / d_bound).max()))
    assert (r_err <= r_bound).all(), (where, "rew", float(np.max(r_err - r_bound)))
    return float((d_err / d_bound).max()), float((r_err / np.maximum(r_bound, 1e-300)).max())


# ---- hb_per_sample_gather: priorities and host-side uniforms --------------------------------------------------------------
def psg_priorities(pc, size):
    """The writes both trees receive: the ring's inserts as fill_range(0, size, 0.6), then 200 (or size, if fewer) distinct
    slots updated to random priorities (at the large ring: the 96..1024-entry update path that leaves lazy top levels stale).
    Slots >= size keep priority zero. Returns (indices int64, values float32)."""
    rng = np.random.default_rng(pc.seed % 2 ** 32 + size)
    idx = np.sort(rng.permutation(size)[:min(size, 200)]).astype(np.int64)
    return idx, (rng.random(len(idx)) ** 2 + 0.01).astype(np.float32)


def philox_uniforms(seed, counter, batch):
    """u_i of hb_per_sample_philox (include/hanabi_hip.h): bits53(Philox4x32-10(key = seed; counter = (i, counter))) 2^-53 / B."""
    from oracle import oracle_py as O

    u = np.empty(batch, np.float64)
    for i in range(batch):
        w = O.philox([i, 0, int(counter), 0], [seed & 0xFFFFFFFF, seed >> 32])
        u[i] = float((int(w[0]) >> 5) << 26 | (int(w[1]) >> 6)) * 2.0 ** -53 / batch
    return u


def psg_oracle_tree(pc, size):
    from oracle import oracle_py as O

    cap = BY_NAME[pc.case].cap
    tree = O.OracleTree(cap)
    tree.fill_range(0, size, np.float32(0.6))
    tree.update(*psg_priorities(pc, size))
    return tree
