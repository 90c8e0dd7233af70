"""No GPU: the per-slot PER oracle (oracle/per_oracle.py) by hand, then against OracleTree over the case table of
tests/per_cases.py, and the teeth: a tree that is filled as if the ring had the tree's size, or sampled without the clamp,
breaks the oracle's invariants in exactly the cases where ring and tree differ and an insert straddles the ring's end.
tests/test_hip_tree.py holds the kernels bit-equal to OracleTree; tests/test_per_ring_gpu.py runs the same table on the GPU."""
import numpy as np
import pytest

import per_cases as PC
from oracle.per_oracle import PerOracle

A32 = float(np.float32(PC.ALPHA))
# |td| = 32 -> 32 ** float32(0.6) = 8.00000066 -> the float32 above 8 (the exponent is 0.6 rounded to float32, a little more)
P32 = np.float32(np.float64(np.float32(32.0)) ** np.float64(np.float32(0.6)))
assert P32 == np.float32(8.0) + np.float32(2.0 ** -20)


# ---- the oracle by hand: a ring of three slots -----------------------------------------------------------------------------
def test_insert_wraps_at_the_ring():
    o = PerOracle(3, PC.ALPHA)
    assert o.insert(2) == [0, 1] and (o.oldest, o.size) == (2, 2)
    assert o.p.tolist() == [np.float32(0.6), np.float32(0.6), 0.0]
    o.update([0], [32.0], 0.6)                       # a new maximum
    assert o.max_priority == float(P32)
    assert o.insert(2) == [2, 0] and (o.oldest, o.size) == (1, 3)     # slot 2, then slot 0 again: NOT a fourth slot
    assert o.p.tolist() == [P32, np.float32(0.6), P32]
    assert abs(o.total - (2 * float(P32) + A32)) < 1e-12
    assert o.cum().tolist() == [0.0, float(P32), float(P32) + A32, o.total]


def test_update_last_duplicate_wins_and_tracks_max_min():
    o = PerOracle(3, PC.ALPHA)
    o.insert(3)
    o.update([1, 2, 1], [32.0, 0.0, 1.0], 0.6)
    assert o.p[1] == np.float32(1.0)                 # (1 + 1e-10 in float32 = 1) ** 0.6: the later entry, not P32
    assert o.p[2] == PerOracle.priority(0.0, 0.6) and 0 < o.p[2] < 2e-6      # 1e-10 ** 0.6 = 1e-6
    assert o.max_priority == float(P32)              # the overwritten entry still counted (priority_buffer.py:50-51)
    assert o.min_priority == float(o.p[2])
    o.update([0], [-32.0], 0.6)
    assert o.p[0] == P32                             # |td|
    with pytest.raises(AssertionError):
        o.update([3], [1.0], 0.6)                    # no fourth slot


def test_keys_exact_slot_and_the_top_edge():
    o = PerOracle(3, PC.ALPHA)
    o.insert(3)
    o.update([0, 1, 2], [1.0, 32.0, 1.0], 0.6)       # priorities 1, P32, 1: total 10.000001
    assert o.total == 2.0 + float(P32)
    keys = PerOracle.keys(4, [0.0, 0.0, 0.0, 0.0])
    assert keys.tolist() == [0.25, 0.5, 0.75, 1.0]
    assert [o.exact_slot(k) for k in keys] == [1, 1, 1, 3]      # 2.5, 5, 7.5 fall into slot 1's [1, 9); 10 is past the ring
    assert o.exact_slot(0.05) == 0 and o.exact_slot(0.1) == 1 and o.exact_slot(0.95) == 2
    assert o.accepts(2, 1.0, 4) and not o.accepts(3, 1.0, 4) and not o.accepts(1, 1.0, 4)   # the clamp: slot 2, never 3
    assert o.accepts(1, 0.5, 4) and not o.accepts(0, 0.5, 4) and not o.accepts(2, 0.5, 4)
    assert o.accepts(0, 0.1, 4) and o.accepts(1, 0.1, 4)         # on the border both neighbours are within E
    assert o.prob(1) == (float(P32) + 1e-10) / o.total
    assert o.slack(4) == 8 * 2.0 ** -24 * o.total


def test_heap_invariants_by_hand():
    o = PerOracle(3, PC.ALPHA)
    o.insert(3)
    p = np.float32(0.6)
    good = np.array([0, (p + p) + p, p + p, p, p, p, p, 0], np.float32)
    assert o.heap_violations(good) == dict(out_of_ring=0, leaf=0, inner=0)
    bad = good.copy()
    bad[7] = 1.0                                     # the fourth leaf is no slot
    assert o.heap_violations(bad) == dict(out_of_ring=1, leaf=0, inner=1)
    bad = good.copy()
    bad[4] = 0.0
    assert o.heap_violations(bad) == dict(out_of_ring=0, leaf=1, inner=1)


# ---- the oracle against OracleTree over the table ---------------------------------------------------------------------------
def _run(name, split=True, clamp=True):
    """Drives RingTree and PerOracle through the case. Returns what the teeth count; with split and clamp it also asserts the
    whole agreement (leaves exact, invariants, every index accepted, prob within its bound, max / min exact)."""
    case, right = PC.BY_NAME[name], split and clamp
    tree, orc = PC.RingTree(case.cap, split=split, clamp=clamp), PerOracle(case.cap, PC.ALPHA)
    T = tree.T
    assert T == PC.tree_capacity(case.cap)
    out = dict(out_of_ring=0, over=0, edge_over=0, ordinary=0, inexact=0, worst=0.0, edge=set())
    for r, rd in enumerate(PC.rounds(name)):
        tree.insert(rd.n)
        orc.insert(rd.n)
        v = orc.heap_violations(tree.nodes())
        out["out_of_ring"] += v["out_of_ring"]
        if right:
            assert v == dict(out_of_ring=0, leaf=0, inner=0), (name, r, "after the insert", v)
        idx, prob = tree.sample(rd.u)
        out["over"] += int((idx >= case.cap).sum())
        out["edge_over"] += int(idx[-1] >= case.cap)
        out["edge"].add(int(idx[-1]))
        if right:
            keys, cum, total = PerOracle.keys(case.B, rd.u), orc.cum(), orc.total
            for i, (k, key) in enumerate(zip(idx, keys)):
                assert orc.accepts(k, key, T), (name, r, i, int(k), key)
                assert abs(prob[i] - orc.prob(k)) <= PerOracle.prob_rtol(T) * orc.prob(k), (name, r, i)
                if i < case.B - 1:                   # every stratum but the forced top edge
                    out["ordinary"] += 1
                    out["inexact"] += int(k != orc.exact_slot(key))
                    x = key * total                  # how far outside slot k's own share, as a fraction of E
                    out["worst"] = max(out["worst"], max(cum[k] - x, x - cum[k + 1], 0.0) / orc.slack(T))
        idx = np.minimum(idx, case.cap - 1)          # (only the teeth runs still carry larger ones)
        wb = PC.writeback_indices(idx)
        tree.update(wb, rd.td)
        orc.update(wb, rd.td, PC.ALPHA)
        v = orc.heap_violations(tree.nodes())
        out["out_of_ring"] += v["out_of_ring"]
        if right:
            assert v == dict(out_of_ring=0, leaf=0, inner=0), (name, r, "after the write-back", v)
            assert (tree.max_priority, tree.min_priority) == (orc.max_priority, orc.min_priority), (name, r)
    return out


@pytest.mark.parametrize("name", PC.NAMES)
def test_ring_driven_tree_equals_the_slot_oracle(name):
    """Fills split at the ring's end, indices clamped: every leaf exact and the three invariants after every insert and every
    write-back, every index accepted, prob within (d + 2) u, max / min exact. Every sample but the forced top edge is the
    slot the exact float64 cumulative sum selects (share that differs: 0; largest deviation / E: 0)."""
    case, out = PC.BY_NAME[name], _run(name)
    print(f"{name}: T {PC.tree_capacity(case.cap)}, {out['ordinary']} ordinary samples, {out['inexact']} not the exact slot, "
          f"worst deviation / E {out['worst']:.3f}, top-edge indices {sorted(out['edge'])}")
    assert out["ordinary"] == PC.n_rounds(case) * (case.B - 1)
    assert out["inexact"] == 0 and out["over"] == 0 and out["out_of_ring"] == 0
    assert out["edge"] == {case.cap - 1}             # key 1.0: the ring's last slot, on every ring


@pytest.mark.parametrize("name", PC.NAMES)
def test_teeth_a_fill_that_wraps_at_the_tree_breaks_the_invariant(name):
    """One fill_range(oldest, n), as the product called it before the tree knew its ring: leaves past the ring become live
    exactly where the ring is no power of two and an insert straddles its end, and then samples land there."""
    case, out = PC.BY_NAME[name], _run(name, split=False, clamp=False)
    print(f"{name}: out-of-ring leaf observations > 0: {out['out_of_ring']}, sampled indices >= capacity: {out['over']}")
    if PC.straddles(case):
        assert out["out_of_ring"] > 0
    else:
        assert out["out_of_ring"] == 0 and out["over"] == out["edge_over"]


def test_teeth_cases_are_the_listed_ones():
    assert [PC.straddles(c) for c in PC.CASES] == [True, True, True, True, True, False, False, False, True]


@pytest.mark.parametrize("name", PC.NAMES)
def test_teeth_without_the_clamp_the_top_edge_leaves_the_ring(name):
    """Right fills, raw indices: the u = 0 stratum returns T - 1, an index past the ring on every ring that is no power of
    two and on none that is; nothing else ever leaves the ring."""
    case, out = PC.BY_NAME[name], _run(name, split=True, clamp=False)
    assert out["out_of_ring"] == 0 and out["over"] == out["edge_over"]
    # (root - left child, rounded, can come out a little below the right child: then the key ends on the last LIVE leaf, in the
    #  ring, and not on the tree's last one; c1000_n96_B64 has such rounds)
    print(f"{name}: top-edge indices {sorted(out['edge'])}, {out['edge_over']} of {PC.n_rounds(case)} rounds past the ring")
    assert {e for e in out["edge"] if e >= case.cap} == (set() if PC.is_pow2(case.cap) else {PC.tree_capacity(case.cap) - 1})
    assert (out["edge_over"] > 0) == (not PC.is_pow2(case.cap))
