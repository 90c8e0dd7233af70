"""Per-slot oracle of prioritized replay (PER). TEST INFRASTRUCTURE ONLY.

Written from what PER MEANS on a replay ring of `capacity` slots, not from how the sum tree stores it: one priority per
ring slot, a cumulative sum over the slots, and a sample is the slot whose share of that sum holds the key. There is no
heap, no tree capacity, no chunk and no descent in here, and no arithmetic is shared with csrc/sum_tree.hip or with
oracle_py.OracleTree (the C flat-array tree). All sums are float64; a priority is held as the float32 value the kernels
store (reference: hanabi_agents/rlax_dqn/priority_buffer.py:29-52).

What the oracle states about a sum tree of T = 2^d >= capacity leaves that serves this ring (`heap_violations`):
  1. leaves capacity .. T-1 are all zero (they are no ring slots: nothing may ever give them a priority);
  2. leaf s equals the slot model's priority for every s < capacity;
  3. every inner node equals fl(left + right) in float32.

The product never imports this module (tests/test_capi_symbols.py::test_product_never_touches_the_oracle).
"""
import math

import numpy as np

U = 2.0 ** -24   # unit roundoff of float32


class PerOracle:
    def __init__(self, capacity, alpha=0.6):
        self.capacity = int(capacity)
        self.p = np.zeros(self.capacity, np.float32)     # one priority per ring slot
        self.oldest = 0                                  # the slot the next inserted row goes to
        self.size = 0
        self.max_priority = float(np.float32(alpha))     # priority_buffer.py:21-22
        self.min_priority = float(np.float32(alpha))

    # ---- writes ---------------------------------------------------------------------------------------------------------
    def insert(self, n):
        """n new rows: slots (oldest + i) % capacity take max_priority (priority_buffer.py:29-32 with the ring's own
        get_update_indices). Returns the slots, in row order."""
        assert 0 <= n <= self.capacity
        slots = [(self.oldest + i) % self.capacity for i in range(n)]
        for s in slots:
            self.p[s] = np.float32(self.max_priority)
        self.oldest = (self.oldest + n) % self.capacity
        self.size = min(self.size + n, self.capacity)
        return slots

    @staticmethod
    def priority(td, alpha):
        """(|td| + 1e-10) ** alpha on float32 data: the sum in float32, the exponent rounded to float32, the power in double
        rounded once to float32 (priority_buffer.py:48-49; hb_per_update)."""
        x = np.float32(abs(np.float32(td))) + np.float32(1e-10)
        return np.float32(math.pow(float(x), float(np.float32(alpha))))

    def update(self, idx, td, alpha):
        """Write-back of a batch: in order, so the LAST occurrence of a duplicate index wins; max / min over every entry."""
        for k, t in zip(idx, td):
            k = int(k)
            assert 0 <= k < self.capacity, f"index {k} is no slot of a ring of {self.capacity}"
            p = self.priority(t, alpha)
            self.max_priority = max(self.max_priority, float(p))
            self.min_priority = min(self.min_priority, float(p))
            self.p[k] = p

    # ---- reads ----------------------------------------------------------------------------------------------------------
    @property
    def total(self):
        return float(self.cum()[-1])

    def cum(self):
        """cum[k] = sum of the priorities of slots 0 .. k-1 in float64 (cum[0] = 0, cum[capacity] = total)."""
        return np.concatenate([[0.0], np.cumsum(self.p.astype(np.float64))])

    @staticmethod
    def keys(B, u):
        """The stratified keys linspace(1/B, 1, B) - u in float64 (priority_buffer.py:37-40), u[i] in [0, 1/B)."""
        return np.linspace(1.0 / B, 1.0, B) - np.asarray(u, np.float64)

    def exact_slot(self, key):
        """The slot an exact cumulative sum selects: cum[k] <= key * total < cum[k + 1] (the descent goes left on a strict
        <). key * total == total selects nothing: `capacity` is returned (the top edge; see `accepts`)."""
        return int(np.searchsorted(self.cum(), key * self.total, side="right")) - 1

    def slack(self, T):
        """E = (3 d + 2) u total with d = log2(T), u = 2^-24: how far a float32 sum tree of T leaves may be from this
        model when it places a key. A derived bound, not a measurement:
          * every inner node is fl(left + right), one rounding per level, so a node d levels above the leaves is within
            d u (relative, to first order) of the exact sum of its leaves, and so is every partial sum the descent
            meets: at most d u total;
          * the key takes two roundings before the descent starts, the cast float32(key) and the product with the
            float32 total, whose own error is the root's d u: (d + 2) u total in all;
          * each of the at most d right turns subtracts a rounded left child from the running query and rounds the
            difference once; the left children's errors are counted in the first item, the roundings add d u total.
        """
        d = int(round(math.log2(T)))
        assert 2 ** d == T
        return (3 * d + 2) * U * self.total

    def accepts(self, k, key, T):
        """Is slot k a right answer for `key` from a float32 tree of T leaves? Yes iff key * total lies within E of slot
        k's share [cum[k], cum[k + 1]] of the cumulative sum.
        Clamp rule at the top edge: a key with key * total >= cum[capacity] - E may run off the end of the ring (the
        reference quirk C-8: the key float32(1 - u) * total == total ends on the tree's last leaf). On a ring that is a
        power of two that leaf is slot capacity - 1; on any other ring the sampler must clamp to it. So slot
        capacity - 1 is accepted for such a key, whatever its own priority; an index >= capacity never is."""
        k = int(k)
        if not 0 <= k < self.capacity:
            return False
        cum, x, E = self.cum(), key * self.total, self.slack(T)
        if x >= cum[self.capacity] - E and k == self.capacity - 1:
            return True
        return cum[k] - E <= x <= cum[k + 1] + E

    def prob(self, k):
        """(p[k] + 1e-10) / total (priority_buffer.py:42). A float32 tree's value differs by its root's error only:
        compare at the relative tolerance `prob_rtol(T)`."""
        return (float(self.p[int(k)]) + 1e-10) / self.total

    @staticmethod
    def prob_rtol(T):
        return (int(round(math.log2(T))) + 2) * U

    # ---- the invariants of a heap that serves this ring -------------------------------------------------------------------
    def heap_violations(self, nodes):
        """nodes[0 .. 2T): an exported heap, root at 1, leaves at [T, 2T). Returns the counts of entries that break each
        of the three invariants: dict(out_of_ring=, leaf=, inner=). All zero = the heap is this ring's."""
        nodes = np.asarray(nodes, np.float32)
        T = len(nodes) // 2
        assert T >= self.capacity and T & (T - 1) == 0
        leaves = nodes[T:]
        inner = nodes[1:T]
        sums = nodes[2:2 * T:2] + nodes[3:2 * T:2]        # float32 + float32 -> one float32 rounding
        return dict(out_of_ring=int(np.count_nonzero(leaves[self.capacity:])),
                    leaf=int(np.count_nonzero(leaves[:self.capacity].view(np.uint32) != self.p.view(np.uint32))),
                    inner=int(np.count_nonzero(inner.view(np.uint32) != sums.view(np.uint32))))
