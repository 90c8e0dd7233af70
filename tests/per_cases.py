"""The one case table of the prioritized-replay ring tests (tests/test_per_oracle_cpu.py on the host, tests/test_per_ring_gpu.py
on the GPU) and what both share: the rounds of a case (insert size, stratified uniforms, TD errors of the write-back), the
write-back's indices, and OracleTree driven the way a tree that serves a ring must be driven.

A ring has `capacity` slots, its sum tree T = 2^ceil(log2(capacity)) leaves. A case is (capacity, rows per insert, batch):

* (1000, 96, 64), (1025, 300, 64): T = 1024 / 2048; capacity one past a power of two makes T almost twice the ring;
* (5000, 1536, 256): T = 8192 = eight 1024-leaf chunks, the ring ends mid-chunk (5000 = 4 * 1024 + 904), an insert spans more
  than one chunk, and a 256-entry write-back takes the per-chunk update path (the others take the one-workgroup path);
* (700, 699, 32): an insert one short of the ring: every insert but the first straddles the ring's end;
* (3, 2, 4): a 4-leaf tree, more strata than slots;
* (384, 64, 128), (2500, 2500, 256), (1024, 96, 64): the controls. The insert divides the ring, is the ring, or the ring is a
  power of two: a fill that wraps at T instead of at the ring does no harm in the first two, and is right in the third;
* (1000, [96, 7, 300], 64): insert sizes that vary from call to call (the compacting add_experience and the off-belief insert).

Every round is insert -> stratified sample -> write-back, for ceil(2.5 * capacity / n) + 1 rounds (n: the mean insert size),
i.e. two and a half laps. Uniforms come from default_rng(case index) with the two edges forced in every round: u[-1] = 0 (the
top key is exactly 1.0; in alternate rounds u[-1] = 2^-26, which still rounds to float32 key 1.0; 2^-24 would not) and
u[0] = nextafter(1/B, 0) (the bottom key is the smallest positive one).
"""
import collections
import functools
import math

import numpy as np

ALPHA = 0.6
Case = collections.namedtuple("Case", "name cap n_ins B")
Round = collections.namedtuple("Round", "n u td")


def _c(cap, n_ins, B):
    ns = n_ins if isinstance(n_ins, tuple) else (n_ins,)
    return Case(f"c{cap}_n{'_'.join(map(str, ns))}_B{B}", cap, ns, B)


CASES = (_c(1000, 96, 64), _c(1025, 300, 64), _c(5000, 1536, 256), _c(700, 699, 32), _c(3, 2, 4),
         _c(384, 64, 128), _c(2500, 2500, 256), _c(1024, 96, 64), _c(1000, (96, 7, 300), 64))
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]


def tree_capacity(cap):
    return 1 << max(0, (cap - 1).bit_length())


def is_pow2(cap):
    return cap & (cap - 1) == 0


def n_rounds(case):
    return math.ceil(2.5 * case.cap * len(case.n_ins) / sum(case.n_ins)) + 1


def straddles(case):
    """Does some insert of the case cross the ring's end on a ring that is no power of two? (Derived from the ring's
    arithmetic alone: the write pointer advances by n modulo capacity.)"""
    wp, hit = 0, False
    for r in range(n_rounds(case)):
        n = case.n_ins[r % len(case.n_ins)]
        hit = hit or wp + n > case.cap
        wp = (wp + n) % case.cap
    return hit and not is_pow2(case.cap)


@functools.lru_cache(maxsize=None)
def rounds(name):
    """The rounds of a case: Round(n rows inserted, u float64 [B] in [0, 1/B), td float32 [B]). Read-only by convention."""
    case = BY_NAME[name]
    rng, B, out = np.random.default_rng(NAMES.index(name)), case.B, []
    for r in range(n_rounds(case)):
        u = rng.random(B) / B
        u[0] = np.nextafter(1.0 / B, 0.0)
        u[-1] = 2.0 ** -26 if r % 2 else 0.0
        td = (rng.standard_normal(B) * 2.0).astype(np.float32)
        if r % 3 == 1:
            td[B // 2] = 0.0            # the smallest priority there is: 1e-10 ** alpha (the running minimum moves)
        if r % 4 == 2:
            td[1] = 40.0 + r            # and a new maximum, which the next insert's leaves then take
        u.setflags(write=False)
        td.setflags(write=False)
        out.append(Round(case.n_ins[r % len(case.n_ins)], u, td))
    return tuple(out)


def writeback_indices(idx):
    """The indices of a round's write-back: the sampled ones, with the first max(1, B // 8) of them repeated further on, so
    every write-back carries duplicate indices with different TD errors (the last occurrence must win)."""
    idx = np.array(idx, np.int64)
    B = len(idx)
    k = max(1, B // 8)
    idx[B // 2:B // 2 + k] = idx[:k]
    return idx


class RingTree:
    """OracleTree (the C flat-array tree that tests/test_hip_tree.py holds the kernels bit-equal to) driven as the tree of a
    ring of `cap` slots: a fill is split at the ring's end, a sampled index past the ring becomes the ring's last slot with
    that leaf's priority. split=False / clamp=False: one fill_range(oldest, n) that wraps at the TREE's size and the raw
    index — what the product did before it knew the ring (the tests' teeth)."""

    def __init__(self, cap, split=True, clamp=True):
        from oracle import oracle_py as O

        self.cap, self.split, self.clamp = cap, split, clamp
        self.tree = O.OracleTree(cap)
        self.T = self.tree.cap
        self.oldest = 0
        self.max_priority = self.min_priority = float(np.float32(ALPHA))

    def insert(self, n):
        v, first = np.float32(self.max_priority), min(n, self.cap - self.oldest)
        if self.split:
            self.tree.fill_range(self.oldest, first, v)
            if n > first:
                self.tree.fill_range(0, n - first, v)
        else:
            self.tree.fill_range(self.oldest, n, v)
        self.oldest = (self.oldest + n) % self.cap

    def sample(self, u):
        idx, prob = self.tree.per_sample(u)
        if self.clamp and (idx >= self.cap).any():
            over = idx >= self.cap
            idx[over] = self.cap - 1
            leaf = np.float64(self.tree.leaves()[self.cap - 1])
            prob[over] = (leaf + 1e-10) / np.float64(np.float32(self.tree.total()))
        return idx, prob

    def update(self, idx, td):
        self.max_priority, self.min_priority = self.tree.per_update(idx, td, ALPHA, self.max_priority, self.min_priority)

    def nodes(self):
        return self.tree.nodes()
