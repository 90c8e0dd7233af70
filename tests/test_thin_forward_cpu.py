"""Host: the contract and the launch sizing of hb_thin_forward as oracle/thin_forward_oracle.py states them (no GPU).

1. npair = (K + 14) // 16 + 1 column tiles per gathered row group suffice for K atoms at every start column, and some start
   column needs that many: the formula is sufficient and tight.
2. B // 32 + min(A, B) row groups suffice for every action histogram: sum_a ceil(count_a / 32) never exceeds it.
3. The need / may masks equal the expressions tests/test_thin_forward.py asserts on the device, at its shapes.
tests/test_thin_forward_f64.py holds the kernel to these masks and recomputes its walking launch from these formulas."""
import numpy as np
import pytest

from oracle import thin_forward_oracle as TF
from thin_forward_cases import BF, HF, LAYER2_CASES, WALKING


def test_npair_covers_every_alignment_and_is_reached():
    for K in range(1, 65):
        for a in range(64):              # the start columns a launch really has: a * K
            assert TF.tiles_touched(a * K, K) <= TF.npair(K), (K, a)
        per_start = [TF.tiles_touched(s, K) for s in range(16)]       # every alignment of a start column within its tile
        assert max(per_start) == TF.npair(K), (K, per_start)
        # with a * K as the only starts: an odd K meets every alignment (a * K % 16 runs through all 16), so the maximum is needed
        # (K = 51: action 5 starts at column 255); K = 16, 32, 48, 64 start aligned and the group's last tile finds no column
        reached = max(TF.tiles_touched(a * K, K) for a in range(64))
        if K % 2:
            assert reached == TF.npair(K), K
        if K % 16 == 0:
            assert reached == TF.npair(K) - 1, K
    assert TF.npair(51) == 5 and TF.tiles_touched(5 * 51, 51) == 5 and TF.npair(1) == 1 and TF.npair(64) == 5


def _histograms(B, A):
    """adversarial action vectors of a batch of B over A actions"""
    rng = np.random.default_rng(B * 100 + A)
    out = {"one id": np.full(B, A - 1), "first id": np.zeros(B, int)}
    each = np.zeros(B, int)
    each[:min(A, B)] = np.arange(min(A, B))                  # one sample per action, the rest on action 0
    out["each once"] = each
    out["uniform"] = rng.integers(0, A, B)
    out["round robin"] = np.arange(B) % A                     # every action with a partial group, as many as fit
    for c in (31, 32, 33):
        if B >= c:                                            # c on one action, the rest spread one by one, then on the last
            v = np.full(B, A - 1)
            v[:c] = 0
            rest = np.arange(B - c)
            v[c:] = np.minimum(1 + rest, A - 1) if A > 1 else 0
            out[f"{c} on one"] = v
    if A >= 4 and B >= 97:
        v = np.full(B, 3)
        v[:31], v[31:63], v[63:96] = 0, 1, 2
        out["31/32/33"] = rng.permutation(v)
    # as many actions as possible with 1 sample beyond a multiple of 32
    v, a, i = np.zeros(B, int), 0, 0
    while i < B and a < A:
        take = min(33 if (B - i) >= 33 and a % 2 == 0 else 1, B - i)
        v[i:i + take] = a
        i, a = i + take, a + 1
    v[i:] = A - 1
    out["33s and 1s"] = v
    return out


@pytest.mark.parametrize("A", [1, 2, 20, 48, 64])
@pytest.mark.parametrize("B", list(range(32, 257, 32)))
def test_group_bound_covers_every_histogram(B, A):
    for name, act in _histograms(B, A).items():
        assert act.shape == (B,) and act.min() >= 0 and act.max() < A, name
        assert TF.row_groups(act, A) <= TF.group_bound(B, A), (name, TF.row_groups(act, A))
    # the bound's two terms are each met: B / 32 full groups (one id), and one partial group per action that occurs
    assert TF.row_groups(np.zeros(B, int), A) == B // 32
    if A <= B // 33:          # A actions of 33 samples each: 2 A groups, within B // 32 + A and above either term alone
        v = np.zeros(B, int)
        v[:33 * A] = np.repeat(np.arange(A), 33)
        assert TF.row_groups(v, A) >= 2 * A


def test_unit_counts_at_the_learners_shapes():
    """the figures csrc/learner2.hip quotes for 2 players, B = 256"""
    assert TF.n_units(1, 256, 1024) == 768
    assert TF.group_bound(256, 20) * TF.npair(51) == 140
    assert TF.n_units(2, 256, 1024, 20, 51) == 140 + 1024 > TF.MAX_WORKGROUPS
    assert TF.workgroups(768) == 768 and TF.workgroups(1164) == 582 and TF.workgroups(1024) == 1024 and TF.workgroups(1025) == 513


def test_the_walking_case_is_in_the_device_table():
    """tests/test_thin_forward_f64.py keeps, for both dtypes, a layer-2 case whose launch exceeds 1 024 units"""
    A, K, B, n = WALKING
    hits = [c for c in LAYER2_CASES if (c[0], c[1], c[3], (c[0] * c[1] + c[5] - 1) // c[5] * c[5]) == WALKING]
    assert {c[4] for c in hits} == {BF, HF}
    assert TF.n_units(2, B, n, A, K) > TF.MAX_WORKGROUPS


@pytest.mark.parametrize("kind", ["one", "each", "uniform"])
@pytest.mark.parametrize("B", [256, 96])
@pytest.mark.parametrize("players", [2, 5])
def test_masks_equal_the_device_tests_expressions(players, B, kind):
    """tests/test_thin_forward.py, test_bit_equal_to_thin_gemm_where_it_writes: wrote1, need and may, restated in numpy term by
    term at that test's shapes (hidden 512, 51 atoms, 658 bits / 20 actions and 1 280 bits / 48 actions, columns padded to 64)."""
    K51, H = 51, 512
    A = {2: 20, 5: 48}[players]
    Np = (A * K51 + 63) // 64 * 64
    rng = np.random.default_rng(players * 1000 + B)
    if kind == "one":
        act = np.full(B, A - 1)
    elif kind == "each":
        act = np.zeros(B, int)
        n = min(A, B)
        act[rng.permutation(B)[:n]] = np.arange(n)
    else:
        act = rng.integers(0, A, B)
    # layer 1
    wrote1 = np.ones((2 * B, 2 * H), bool)
    wrote1[:B, H:] = False
    need1, may1 = TF.masks(1, B, 2 * H)
    assert np.array_equal(need1, wrote1) and np.array_equal(may1, wrote1)
    # layer 2
    cols = np.arange(Np)
    need = (cols[None, :] >= (act * K51)[:, None]) & (cols[None, :] < ((act + 1) * K51)[:, None])
    tile_lo, tile_hi = (act * K51) // 16 * 16, ((act + 1) * K51 - 1) // 16 * 16 + 16
    may = (cols[None, :] >= tile_lo[:, None]) & (cols[None, :] < tile_hi[:, None])
    need2, may2 = TF.masks(2, B, Np, act, A, K51)
    assert np.array_equal(need2[0, :B], need) and np.array_equal(may2[0, :B], may)
    assert need2[:, B:].all() and may2[:, B:].all()                    # obs_t: both networks, dense
    assert not need2[1, :B].any() and not may2[1, :B].any()            # target on obs_tm1: never
    assert (need2 <= may2).all()
    assert (may2[0, :B].sum(1) == [16 * TF.tiles_touched(a * K51, K51) for a in act]).all()
