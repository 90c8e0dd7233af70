"""CPU: the float64 actor oracle (oracle/actor_oracle.py) pinned by itself — against the learner oracle's network, hand-worked
expectations, the C Philox of oracle/hanabi_oracle.c and the Random123 known answers, hand-worked selections, and each error
bound (a perturbation of the bound's size stays inside it, one of 3x the bound lands outside)."""
import numpy as np
import pytest

from oracle import actor_oracle as AO
from oracle import learner_oracle as LO
from oracle import oracle_py as O


# ---- forward ------------------------------------------------------------------------------------------------------------------
def test_forward_equals_learner_oracle_network_plus_softmax():
    rng = np.random.default_rng(0)
    obs = (rng.random((9, 37)) < 0.4).astype(float)
    A, K, H = 3, 7, 16
    w1, b1 = rng.standard_normal((37, H)), rng.standard_normal(H)
    w2, b2 = rng.standard_normal((H, A * K)), rng.standard_normal(A * K)
    support = np.linspace(-5, 5, K)
    zero = lambda s: np.zeros(s)
    layers = [dict(w=w1, b=b1, w_mu=zero(w1.shape), b_mu=zero(b1.shape), w_sigma=zero(w1.shape), b_sigma=zero(b1.shape),
                   eps_w=zero(w1.shape), eps_b=zero(b1.shape)),
              dict(w=w2, b=b2, w_mu=zero(w2.shape), b_mu=zero(b2.shape), w_sigma=zero(w2.shape), b_sigma=zero(b2.shape),
                   eps_w=zero(w2.shape), eps_b=zero(b2.shape))]
    ref = LO.noisy_mlp_forward(obs, layers).reshape(9, A, K)
    f = AO.forward(obs, w1, b1, w2, b2, support, A)
    np.testing.assert_allclose(f["logits"], ref, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(f["q"], (LO.softmax(ref) * support).sum(-1) / K, rtol=1e-12, atol=1e-14)
    np.testing.assert_array_equal(f["h"], np.maximum(obs @ w1 + b1, 0))


def test_expectation_hand_worked():
    K = 51
    lin = np.linspace(-25, 25, K)
    # equal logits: uniform p, q = mean(support) / K
    asym = np.concatenate([np.linspace(-3, 0, 20), np.linspace(0.5, 40, 31)])
    for s in (lin, asym):
        assert AO.expectation(np.full(K, 3.25), s) == pytest.approx(s.mean() / K, rel=1e-14, abs=1e-15)
    # one atom 1 000 above the rest: q = support[j] / K
    for j in (0, 17, 50):
        l = np.zeros(K)
        l[j] = 1000.0
        assert AO.expectation(l, asym) == pytest.approx(asym[j] / K, rel=1e-14)
    # two atoms, asymmetric support: p = (e^1, 1) / (e + 1)
    s2 = np.array([-1.0, 4.0])
    assert AO.expectation(np.array([1.0, 0.0]), s2) == pytest.approx((np.e * -1 + 4) / (np.e + 1) / 2, rel=1e-14)


# ---- Philox ---------------------------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    kats = [([0, 0, 0, 0], [0, 0], [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]),
            ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]),
            ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0],
             [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1])]
    for c, k, want in kats:
        assert list(AO.philox4x32_10(np.array(c), np.array(k))) == want


def test_philox_equals_c_oracle_on_random_words():
    rng = np.random.default_rng(1)
    ctr = rng.integers(0, 1 << 32, (200, 4), dtype=np.uint64)
    key = rng.integers(0, 1 << 32, (200, 2), dtype=np.uint64)
    ctr[:20, 1] = ctr[:20, 3] = 0xFFFFFFFF                 # high words set
    key[:20, 1] = 0xFFFFFFFF
    got = AO.philox4x32_10(ctr, key)
    for i in range(200):
        assert list(got[i]) == list(O.philox(ctr[i].astype(np.uint32), key[i].astype(np.uint32))), i


def test_selection_draws_use_high_words():
    r0, r1 = AO.selection_draws((7 << 32) | 5, (3 << 32) | 9, np.array([(1 << 32) + 4, 4], np.uint64))
    want = O.philox([9, 3, 4, 1], [5, 7])
    assert (r0[0], r1[0]) == (want[0], want[1])
    assert (r0[1], r1[1]) != (want[0], want[1])


# ---- selection ------------------------------------------------------------------------------------------------------------------
def _draws(seed, draw, g):
    r = O.philox([draw & 0xFFFFFFFF, draw >> 32, g & 0xFFFFFFFF, g >> 32], [seed & 0xFFFFFFFF, seed >> 32])
    return int(r[0]), int(r[1])


def test_select_hand_worked():
    seed, draw = 11, 4
    # a tie between actions 1 and 3 (action 0 is larger but illegal): greedy picks tie[umulhi(r1, 2)]
    q = np.array([[5.0, 2.0, 1.0, 2.0]], np.float32)
    legal = np.array([[0, 1, 1, 1]])
    r0, r1 = _draws(seed, draw, 0)
    assert AO.select(q, legal, 0.0, seed, draw, 0)[0] == [1, 3][(r1 * 2) >> 32]
    # epsilon = 1: every u < 1, so the pool is every legal action
    assert AO.select(q, legal, 1.0, seed, draw, 0)[0] == [1, 2, 3][(r1 * 3) >> 32]
    # all illegal: 0
    assert AO.select(q, np.zeros((1, 4)), 0.5, seed, draw, 0)[0] == 0
    # one legal action at index 63 of 64, whatever epsilon
    l64 = np.zeros((1, 64))
    l64[0, 63] = 1
    for eps in (0.0, 0.25, 1.0):
        assert AO.select(np.zeros((1, 64), np.float32), l64, eps, seed, draw, 0)[0] == 63
    # A = 1
    assert AO.select(np.array([[0.3]], np.float32), np.ones((1, 1)), 0.25, seed, draw, 0)[0] == 0


def test_select_epsilon_uses_word0_and_game_id():
    """u = (r0 >> 8) / 2^24 against epsilon, per game id (first_gid + row, 64-bit): rows whose u is just below / above epsilon
    explore / exploit, and the id's high word changes the draws."""
    seed, draw, g0 = 5, (1 << 33) + 2, (1 << 32) - 5
    n = 400
    q = np.tile(np.arange(8, dtype=np.float32), (n, 1))      # unique arg-max 7
    legal = np.ones((n, 8))
    for eps in (0.0, 0.25, 1.0):
        got = AO.select(q, legal, eps, seed, draw, g0)
        for g in range(n):
            r0, r1 = _draws(seed, draw, g0 + g)
            u = (r0 >> 8) / 2.0 ** 24
            assert got[g] == (((r1 * 8) >> 32) if u < eps else 7)
    assert 0 < (AO.select(q, legal, 0.25, seed, draw, g0) != 7).sum() < n


# ---- bounds ---------------------------------------------------------------------------------------------------------------------
def test_h_interval_contains_perturbations_of_the_bound():
    rng = np.random.default_rng(2)
    z = rng.standard_normal(4000) * 3
    e = np.abs(z) * 1e-5 + 1e-7
    for dt in ("bfloat16", "float16"):
        lo, hi = AO.h_interval(z, e, dt)
        for sgn in (-1.0, 1.0):
            v = AO.round_to(AO.relu(z + sgn * e * rng.random(z.shape)), dt)
            assert ((v >= lo) & (v <= hi)).all()
        # 3x the ulp-scale perturbation leaves the interval wherever it is pinned to one value and far from the rounding edge
        big = AO.round_to(AO.relu(z + 3 * AO.half_ulp(z, dt) * 2), dt)
        pinned = (lo == hi) & (z > 0)
        assert ((big[pinned] > hi[pinned]) | (big[pinned] < lo[pinned])).mean() > 0.9


def test_logit_err_covers_any_h_in_the_interval():
    rng = np.random.default_rng(3)
    Hn, n = 64, 20
    z = rng.standard_normal((n, Hn))
    w2, b2 = rng.standard_normal((Hn, 30)), rng.standard_normal(30)
    e_z = np.full_like(z, 0.02)                               # wide on purpose: many two-value H
    lo, hi = AO.h_interval(z, e_z, "bfloat16")
    mid = AO.round_to(AO.relu(z), "bfloat16")
    e_l = AO.logit_err(lo, hi, mid, w2, b2)
    for _ in range(10):
        pick = np.where(rng.random(z.shape) < 0.5, lo, hi)
        assert (np.abs((pick @ w2 + b2) - (mid @ w2 + b2)) <= e_l).all()
    # the worst H choice: per hidden unit the end of the interval farther from mid, on the side that moves the logit the same way
    # as every other unit (one logit at a time). It stays inside; H moved 3x as far in the same direction lands outside.
    dev = np.maximum(hi - mid, mid - lo)
    for k in range(w2.shape[1]):
        move = dev * np.sign(w2[:, k])
        worst = np.abs(((mid + move) @ w2[:, k] + b2[k]) - (mid @ w2[:, k] + b2[k]))
        assert (worst <= e_l[:, k]).all()
        far = np.abs(((mid + 3 * move) @ w2[:, k] + b2[k]) - (mid @ w2[:, k] + b2[k]))
        assert (far > e_l[:, k]).all()


def test_q_bound_inside_and_outside():
    rng = np.random.default_rng(4)
    K = 51
    for s in (np.linspace(-25, 25, K), -np.linspace(1, 30, K), np.concatenate([np.zeros(50), [400.0]])):
        l = rng.standard_normal((200, K)) * 4
        e_l = np.full_like(l, 1e-3)
        e = AO.q_bound(l, e_l, s)
        q = AO.expectation(l, s)
        # inside: logits moved by up to e_l in the worst-case direction (sign of dq/dl) stay within the bound
        p = AO.softmax(l)
        E = (p * s).sum(-1, keepdims=True)
        worst = AO.expectation(l + e_l * np.sign(s - E), s)
        assert (np.abs(worst - q) <= e).all()
        # outside: the same move made 3x larger leaves the bound (its rounding terms are far below the input term here)
        assert (np.abs(AO.expectation(l + 3 * e_l * np.sign(s - E), s) - q) > e).mean() > 0.9


def test_stage_f16_clamps_and_rounds():
    l = np.array([0.1, 1000.3, -7e4, 7e4, 64999.0, 64768.0, 1000.25])
    e_l = np.array([1e-3, 1e-3, 1.5, 1.5, 1e-3, 1.5, 0.01])
    c, e = AO.stage_f16(l, e_l)
    # beyond the clamp: exactly the fp16 rounding of +-65 000 (64 992); 64 768 is an fp16 value whose interval holds no
    # rounding edge: exact; 1000.25 +- 0.01 straddles the edge between 1000.0 and 1000.5: a two-value interval
    np.testing.assert_array_equal(c[[2, 3, 5]], [-64992.0, 64992.0, 64768.0])
    np.testing.assert_array_equal(e[[2, 3, 5]], 0.0)
    assert (c[6], e[6]) == (1000.25, 0.25)
    # inside: any fp32 accumulator within e_l stages into [c - e, c + e]
    rng = np.random.default_rng(7)
    for _ in range(20):
        v = l + e_l * rng.uniform(-1, 1, l.shape)
        staged = AO.round_to(np.clip(v, -65000, 65000), "float16")
        assert (np.abs(staged - c) <= e).all()
    # outside: a perturbation of 3x the bound (at least an fp16 ulp) moves the staged value out of the interval
    step = 3 * np.maximum(e, 2 * AO.half_ulp(c, "float16"))
    moved = AO.round_to(np.clip(c + step, -65000, 65000), "float16")
    inner = np.abs(c) < 60000
    assert (np.abs(moved - c)[inner] > e[inner]).all()


def test_thin_gemm_and_colsum_bounds():
    rng = np.random.default_rng(5)
    x = AO.round_to(rng.standard_normal((64, 96)), "bfloat16")
    wt = AO.round_to(rng.standard_normal((32, 96)), "bfloat16")
    b = AO.round_to(rng.standard_normal(32), "bfloat16")
    out, err = AO.thin_gemm(x, wt, b, False)
    # inside: an fp32 accumulation (numpy's order) is within the bound
    f32 = (x.astype(np.float32) @ wt.T.astype(np.float32) + b.astype(np.float32)).astype(float)
    assert (np.abs(f32 - out) <= err).all()
    # outside: the same sum moved by 3x the bound leaves it, and so does the sum with one product term dropped (the bound is far
    # below a single term of this product)
    assert (np.abs(f32 + 3 * err - out) > err).all() and (np.abs(f32 - 3 * err - out) > err).all()
    dropped = f32 - x[:, [5]] * wt[:, 5][None, :]
    big = np.abs(x[:, [5]] * wt[:, 5][None, :]) > 1e-2
    assert (np.abs(dropped - out)[big] > err[big]).all()
    r, _ = AO.thin_gemm(x, wt, b, True)
    np.testing.assert_array_equal(r, np.maximum(out, 0))
    y = rng.standard_normal((1000, 7))
    s, e = AO.colsum(y)
    y32 = y.astype(np.float32).sum(0, dtype=np.float32).astype(float)
    assert (np.abs(y32 - s) <= e).all()
    assert (np.abs(y32 + 3 * e - s) > e).all() and (np.abs(y32 - 3 * e - s) > e).all()
    one_row_short = y32 - y[999]
    big = np.abs(y[999]) > 0.1
    assert (np.abs(one_row_short - s)[big] > e[big]).all()
    act = np.array([[0.0, -0.0, 1.0], [2.0, -1.0, np.float64(-0.0)]])
    m, s2, _ = AO.relu_bwd_colsum(np.ones((2, 3)), act)
    np.testing.assert_array_equal(m, [[0, 0, 1], [1, 0, 0]])
    np.testing.assert_array_equal(s2, [1, 0, 1])


def test_round_to_matches_torch():
    import torch

    x = np.random.default_rng(6).standard_normal(10000) * 100
    for dt in ("bfloat16", "float16"):
        want = torch.from_numpy(x).float().to(getattr(torch, dt)).double().numpy()
        np.testing.assert_array_equal(AO.round_to(x, dt), want)
