"""The epsilon-aware soft likelihood filter of the conditioned belief, the parts that need no GPU: hb_belief_select_soft is
declared, exported and bound and checks its arguments before any launch, soft_table's values, and the numpy restatement
hanabi_hip.belief_select_soft_ref on a hand-worked root, against the exact-match restatement of tests/test_search_depth_cpu.py
under a 1 / 0 table, and as a sampler (frequencies against W_k / T). tests/test_belief_soft_gpu.py holds the kernel to the
restatement bit for bit."""
import ctypes as C
import os
import types

import numpy as np
import pytest

from test_search_belief_cpu import _labelled
from test_search_cpu import philox_np
from test_search_depth_cpu import select_depth_ref

A_FULL = 20   # Hanabi-Full, 2 players


# ---- declarations and argument validation ---------------------------------------------------------------------------------------------
def test_the_symbol_is_declared_exported_and_bound():
    import hanabi_hip
    from hanabi_hip import _capi

    for name in ("belief_select_soft", "belief_select_soft_ref", "soft_table"):
        assert hasattr(hanabi_hip, name) and name in hanabi_hip.__all__
    assert "hb_belief_select_soft" in _capi.SIGNATURES and len(_capi.SIGNATURES["hb_belief_select_soft"][1]) == 23
    L = hanabi_hip.lib()
    assert L.hb_belief_select_soft and L.hb_abi_version() == 1
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "hanabi_hip.h")).read()
    assert "int hb_belief_select_soft(const hb_config* cfg, const uint32_t* src_rows_dev" in header


def test_argument_validation_needs_no_gpu():
    import torch

    import hanabi_hip

    L = hanabi_hip.lib()
    cfg = hanabi_hip.make_config()
    ref, one = C.byref(cfg), C.c_void_p(16)
    err = lambda: L.hb_last_error()

    def soft(ptrs=None, m=4, k=8, r=3, d=2, cfg_ref=ref):
        p = [one] * 14 if ptrs is None else list(ptrs)
        return L.hb_belief_select_soft(cfg_ref, *p[:8], m, k, r, d, 1, 2, 0, *p[8:], None)

    assert soft(cfg_ref=None) < 0 and b"null" in err()
    assert soft(cfg_ref=C.byref(hanabi_hip.HbConfig(6, 5, 5, 5, 8, 3, 0))) < 0 and b"players" in err()
    for bad in range(14):
        if bad == 6:   # valid may be NULL
            continue
        p = [one] * 14
        p[bad] = None
        assert soft(p) < 0 and b"null" in err(), bad
    assert soft(k=4097) < 0 and b"n_cand" in err() and b"4096" in err()
    assert soft(k=0) < 0 and b"n_cand" in err()
    assert soft(d=9) < 0 and b"depth" in err()
    assert soft(d=0) < 0 and b"depth" in err()
    assert soft(r=0) < 0 and b"replicas" in err()
    assert soft(m=-1) < 0
    assert soft(m=1 << 20, k=64) < 0 and b"2^31" in err()
    assert soft(m=1 << 20, k=1, r=64) < 0 and b"2^31" in err()
    assert soft(m=0) == 0 and soft(m=0, k=4096, d=8) == 0 and soft(m=0, k=2, r=5) == 0   # (more replicas than candidates: allowed)
    assert soft([one] * 6 + [None] + [one] * 7, m=0) == 0
    if not torch.cuda.is_available():   # a real call without a device: refused, nothing computed on the CPU
        assert soft() == -2


class _Agent:
    def eval_moves(self, *a, **k):
        raise AssertionError("not called")


def test_python_arguments_are_checked():
    import torch

    import hanabi_hip
    from hanabi_hip import OffBeliefSession, RolloutSearch, SearchPlayer, belief_select_soft, soft_table

    cfg = hanabi_hip.make_config()
    z = lambda *shape, dtype=torch.int32: torch.zeros(shape, dtype=dtype)

    def call(m=2, Kn=4, D=2):
        return belief_select_soft(cfg, z(m, 32), z(m * Kn, 32), z(m * Kn), z(D, Kn, m), z(D, Kn, m), z(D, m), None,
                                  soft_table(0.1, A_FULL), 1, 1, 0)

    with pytest.raises(ValueError, match="4096"):
        call(Kn=4097)
    with pytest.raises(ValueError, match="depth"):
        call(D=9)
    with pytest.raises(hanabi_hip.HbError):   # tensors that are not on a GPU: no CPU path
        call()
    for eps in (0.0, 1e-7, 1.0001, -0.1, float("nan")):
        with pytest.raises(ValueError, match="epsilon"):
            soft_table(eps, A_FULL)
        with pytest.raises(ValueError, match="epsilon"):
            SearchPlayer([_Agent(), _Agent()], 0, condition=True, epsilon=eps)
        with pytest.raises(ValueError, match="epsilon"):
            RolloutSearch(epsilon=eps)
    with pytest.raises(ValueError, match="condition=True"):
        SearchPlayer([_Agent(), _Agent()], 0, epsilon=0.1)
    with pytest.raises(ValueError, match="4096"):
        SearchPlayer([_Agent(), _Agent()], 0, condition=True, epsilon=0.1, replicas=1024, oversample=8)
    sp = SearchPlayer([_Agent(), _Agent()], 1, condition=True, depth=2, epsilon=0.25)
    assert sp.epsilon == 0.25 and SearchPlayer([_Agent(), _Agent()], 0).epsilon is None
    assert sp.depth_stats() == dict(reached=[0, 0], survivors=[0, 0], used=[0, 0], shallow=[0, 0], ess=0.0)
    assert "ess" not in SearchPlayer([_Agent(), _Agent()], 1, condition=True, depth=2).depth_stats()
    env = types.SimpleNamespace(players=2, color_shuffled=False)
    with pytest.raises(ValueError, match="belief_epsilon"):
        OffBeliefSession(env, [_Agent(), _Agent()], belief_epsilon=0.1)
    with pytest.raises(ValueError, match="epsilon"):
        OffBeliefSession(env, [_Agent(), _Agent()], belief_policy=[_Agent(), _Agent()], belief_epsilon=2.0)


def test_soft_table_values():
    from hanabi_hip import soft_table

    t = soft_table(0.5, A_FULL).numpy()
    assert t.shape == (2, A_FULL + 1) and t.dtype == np.float64 and t[0, 0] == 0 and t[1, 0] == 0
    # eps = 1/2 and n a power of two: exact binary fractions
    assert [t[0, n] for n in (1, 2, 4, 8)] == [1.0, 0.75, 0.625, 0.5625] and [t[1, n] for n in (1, 2, 4, 8)] == [0.5, 0.25, 0.125, 0.0625]
    t = soft_table(0.1, 5).numpy()
    assert t.shape == (2, 6) and t[0, 5] == 1.0 - 0.1 + 0.1 / 5 and t[1, 5] == 0.1 / 5 and abs(t[0, 5] - 0.92) < 1e-15
    for n in range(1, 6):   # a distribution over the n legal moves: one policy move, n - 1 others
        assert abs(t[0, n] + (n - 1) * t[1, n] - 1.0) < 1e-15
    one = soft_table(1.0, 4).numpy()   # a uniformly random partner: the move tells nothing
    assert np.array_equal(one[0], one[1]) and one[0, 4] == 0.25
    assert soft_table(1e-6, 3)[1, 3] > 0


# ---- the hand-worked root --------------------------------------------------------------------------------------------------------------
def test_hand_worked_root():
    """Root 0: K = 4, depth 2, eps = 1/2 (table: match 1/2 + 1/(2n), miss 1/(2n)); the real moves are 7 (newest), 8.

        k  w  entry 0          entry 1          lik                  q = floor(lik / mx * 2^24)   W = w * q
        0  3  7, n 2: 3/4      8, n 4: 5/8      15/32 = mx           16777216                     50331648
        1  0  -                -                0                    0                            0
        2  5  1, n 2: 1/4      8, n 2: 3/4      3/16                 floor(0.4 * 2^24) = 6710886  33554430
        3  2  7, n 4: 5/8      9, n 8: 1/16     5/128                floor(2^24 / 12) = 1398101   2796202

    T = 86682280; prefix sums 50331648, 50331648, 83886078, 86682280. Root 1 is finished (L = 0, candidates of weight 0): dead copies."""
    from hanabi_hip import belief_select_soft_ref, soft_table

    m, K, R, D = 2, 4, 64, 2
    src, det = _labelled(m, K)
    src[1, 0] = 1 << 19
    w = np.array([3, 0, 5, 2, 0, 0, 0, 0], np.uint32)   # (a finished root's candidates weigh nothing: hb_belief_determinize)
    hyp = np.zeros((D, K, m), np.int64)
    nl = np.ones((D, K, m), np.int64)
    hyp[0, :, 0], nl[0, :, 0] = [7, 7, 1, 7], [2, 3, 2, 4]
    hyp[1, :, 0], nl[1, :, 0] = [8, 8, 8, 9], [4, 3, 2, 8]
    actual = np.array([[7, 0], [8, 0]])
    seed, draw, first = 0x1234567800000005, 0x300000007, 1000
    rows, ow, n_surv, used, fb, ess, x = belief_select_soft_ref(src, det, w, hyp, nl, actual, None, soft_table(0.5, A_FULL).numpy(), R,
                                                                seed, draw, first_row_id=first, details=True)
    assert x["lik"][0].tolist() == [15 / 32, 0.0, 3 / 16, 5 / 128]
    assert x["q"][0].tolist() == [16777216, 0, 6710886, 1398101]
    assert x["W"][0].tolist() == [50331648, 0, 33554430, 2796202] and int(x["T"][0]) == 86682280
    assert n_surv[:, 0].tolist() == [2, 1] and used.tolist() == [2, 0] and fb.tolist() == [0, 2]
    want_ess = 86682280 ** 2 / (50331648 ** 2 + 33554430 ** 2 + 2796202 ** 2)
    assert abs(float(ess[0]) - want_ess) < 1e-6 * want_ess and 1.0 < want_ess < 3.0 and ess[1] == 0 and ess.dtype == np.float32
    # the targets from an independent Philox: counter (0x10000 + r, draw, row id), key (seed low, seed high ^ draw high)
    r = np.arange(R)
    o = philox_np(0x10000 + r, draw & 0xFFFFFFFF, first, 0, seed & 0xFFFFFFFF, ((seed >> 32) ^ (draw >> 32)) & 0xFFFFFFFF)
    target = [(((int(a) << 32) | int(b)) * 86682280) >> 64 for a, b in zip(o[0], o[1])]
    assert x["target"][0].tolist() == target
    picks = [0 if t < 50331648 else 2 if t < 83886078 else 3 for t in target]
    assert x["pick"][0].tolist() == picks and set(picks) == {0, 2, 3}   # (64 draws: each of the three is drawn, candidate 1 never)
    for j, k in enumerate(picks):
        assert np.array_equal(rows[j], det[k]) and ow[j] == 1
    assert (rows[R:] == src[1]).all() and not ow[R:].any() and (x["pick"][1] == -1).all()
    # an n_legal outside 1 .. A makes the candidate weigh nothing
    for bad in (0, A_FULL + 1, -3):
        nl2 = nl.copy()
        nl2[1, 0, 0] = bad
        x2 = belief_select_soft_ref(src, det, w, hyp, nl2, actual, None, soft_table(0.5, A_FULL).numpy(), R, seed, draw, details=True)[-1]
        assert x2["W"][0, 0] == 0 and x2["q"][0].tolist() == [0, 0, 1 << 24, 3495253] and 0 not in x2["pick"][0]
    # an invalid newest entry: nothing is read, the draws follow the importance weights alone
    valid = np.array([[0, 1], [1, 1]], np.uint8)
    out = belief_select_soft_ref(src, det, w, hyp, nl, actual, valid, soft_table(0.5, A_FULL).numpy(), R, seed, draw, details=True)
    assert out[3].tolist() == [0, 0] and out[4].tolist() == [2, 2] and not out[2].any()
    assert out[-1]["W"][0].tolist() == [3 << 24, 0, 5 << 24, 2 << 24]


# ---- a 1 / 0 table is the exact-match filter at full depth --------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(4))
def test_a_one_zero_table_keeps_the_full_depth_survivors(seed):
    from hanabi_hip import belief_select_soft_ref

    rng = np.random.default_rng(seed)
    m, K, R, D = 40, 9, 5, 3
    src, det = _labelled(m, K)
    src[2, 0] = 1 << 19
    w = rng.integers(0, 3, m * K).astype(np.uint32)
    hyp, actual = rng.integers(0, 2, (D, K, m)), rng.integers(0, 2, (D, m))
    hyp[:, :, 4] = 1 - actual[:, None, 4]   # a root nobody explains
    hyp[:, :, 5] = actual[:, None, 5]       # ... and one everybody does
    valid = (rng.integers(0, 4, (D, m)) != 0).astype(np.uint8)
    valid[:, 4:6] = 1
    nl = rng.integers(1, A_FULL + 1, (D, K, m))
    table = np.zeros((2, A_FULL + 1))
    table[0, 1:] = 1.0
    rows, ow, n_surv, used, fb, ess, x = belief_select_soft_ref(src, det, w, hyp, nl, actual, valid, table, R, 3, 4, details=True)
    h_rows, h_w, h_surv, h_used, h_fb = select_depth_ref(src, det, w, hyp, actual, valid, K, K)   # every survivor: R = K
    assert np.array_equal(n_surv, h_surv) and np.array_equal(fb == 2, h_fb == 2)
    seen = {"full": 0, "none": 0, "L0": 0}
    for i in range(m):
        L = int(used[i])
        label = det[i * K:(i + 1) * K, 1]
        if L == 0:   # no usable move (root 2 is finished: its candidates would weigh 0 from the determinizer; here they do not)
            assert fb[i] == 2 and x["W"][i].tolist() == [int(v) << 24 for v in w[i * K:(i + 1) * K]]
            seen["L0"] += 1
            continue
        assert fb[i] == 0
        if h_used[i] == L:   # the deepest filter has survivors: they are the soft filter's support, and every draw is one of them
            hard = {int(r[1]) for r, wt in zip(h_rows[i * K:(i + 1) * K], h_w[i * K:(i + 1) * K]) if wt != 0}
            assert hard == {int(label[k]) for k in range(K) if x["W"][i, k] > 0} and len(hard) == n_surv[L - 1, i]
            assert {int(r[1]) for r in rows[i * R:(i + 1) * R]} <= hard and ow[i * R:(i + 1) * R].all()
            for k in x["pick"][i]:
                assert all(hyp[d, k, i] == actual[d, i] for d in range(L)) and w[i * K + k] != 0
            seen["full"] += 1
        else:        # nobody reproduces all L moves: dead, where the exact-match filter falls back
            assert x["T"][i] == 0 and not ow[i * R:(i + 1) * R].any() and (rows[i * R:(i + 1) * R] == src[i]).all() and ess[i] == 0
            seen["none"] += 1
    assert min(seen.values()) >= 1 and used[4] == D and x["T"][4] == 0 and n_surv[D - 1, 5] == np.count_nonzero(w[5 * K:6 * K])


# ---- the draws follow W_k / T ---------------------------------------------------------------------------------------------------------
N_DRAWS = 20_000


def _frequencies(W_of_lik, L_valid, first):
    """One root with 6 candidates drawn under N_DRAWS distinct row ids (the root repeated: root i draws with row id first + i)."""
    from hanabi_hip import belief_select_soft_ref, soft_table

    K, D = 6, 1
    src, det = _labelled(1, K)
    src, det = np.repeat(src, N_DRAWS, 0), np.tile(det, (N_DRAWS, 1))
    w = np.tile(np.array([1, 2, 0, 3, 4, 5], np.uint32), N_DRAWS)
    hyp = np.tile(np.array([7, 1, 7, 7, 1, 7]).reshape(1, K, 1), (1, 1, N_DRAWS))
    nl = np.tile(np.array([2, 2, 2, 4, 4, 8]).reshape(1, K, 1), (1, 1, N_DRAWS))
    valid = np.full((D, N_DRAWS), L_valid, np.uint8)
    out = belief_select_soft_ref(src, det, w, hyp, nl, np.full((D, N_DRAWS), 7), valid, soft_table(0.5, A_FULL).numpy(), 1, 11, 5,
                                 first_row_id=first, details=True)
    x = out[-1]
    assert (x["W"] == x["W"][0]).all() and x["W"][0].tolist() == W_of_lik
    # a single-root call with that row id draws the same candidate
    for i in (0, 1, 777, N_DRAWS - 1):
        one = belief_select_soft_ref(src[:1], det[:K], w[:K], hyp[:, :, :1], nl[:, :, :1], np.full((D, 1), 7), valid[:, :1],
                                     soft_table(0.5, A_FULL).numpy(), 1, 11, 5, first_row_id=first + i, details=True)[-1]
        assert one["pick"][0, 0] == x["pick"][i, 0] and one["target"][0, 0] == x["target"][i, 0]
    return np.bincount(x["pick"][:, 0], minlength=K), out


def _within_5_sigma(counts, W):
    """Every candidate's count within 5 binomial standard deviations of N * W_k / T: under the null a two-sided 5-sigma miss has
    probability 6e-7 per candidate, so a sound sampler fails this about once in 3e5 seeds; a candidate of weight 0 is never drawn."""
    T = sum(W)
    for k, Wk in enumerate(W):
        p = Wk / T
        sd = (N_DRAWS * p * (1 - p)) ** 0.5
        print(f"candidate {k}: drawn {counts[k]}, expected {N_DRAWS * p:.1f}, sd {sd:.1f}")
        assert abs(counts[k] - N_DRAWS * p) <= 5 * sd, (k, counts[k], N_DRAWS * p, sd)


def test_the_draws_follow_weight_times_likelihood():
    # lik: 3/4, 1/4, -, 5/8, 1/8, 9/16 -> mx 3/4 -> q = 2^24 * (1, 1/3 floored, -, 5/6 floored, 1/6 floored, 3/4)
    W = [1 << 24, 2 * 5592405, 0, 3 * 13981013, 4 * 2796202, 5 * 12582912]
    counts, out = _frequencies(W, 1, first=1 << 33)   # (row ids past 2^32: the high counter word is used)
    assert out[3][0] == 1 and out[4][0] == 0 and counts.sum() == N_DRAWS
    _within_5_sigma(counts, W)


def test_no_usable_move_draws_by_the_importance_weights_alone():
    W = [v << 24 for v in (1, 2, 0, 3, 4, 5)]
    counts, out = _frequencies(W, 0, first=0)
    assert (out[3] == 0).all() and (out[4] == 2).all() and not out[2].any() and counts.sum() == N_DRAWS
    _within_5_sigma(counts, W)
    assert abs(float(out[5][0]) - 15 ** 2 / 55) < 1e-5   # ess of the weights 1, 2, 3, 4, 5
