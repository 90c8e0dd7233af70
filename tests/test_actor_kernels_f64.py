"""GPU: the actor's kernels (csrc/actor_fused.hip, csrc/actor.hip, csrc/policy.hip) and the learner's forward GEMM and column sums
(csrc/learner2.hip hb_thin_gemm, csrc/learner.hip hb_colsum / hb_relu_bwd_colsum) called directly through the C-ABI on crafted
inputs and held against the float64 oracle (oracle/actor_oracle.py) run on exactly the same values: 16-bit inputs are upcast to
float64 before the oracle sees them, so the input dtype never enters a tolerance.

Every tolerance is a per-element bound of the kernel's fp32 arithmetic computed from the oracle's own intermediates and doubled
(oracle/actor_oracle.py derives each one next to its code):
  H        = round_T(relu(z)) pinned to the interval [round_T(relu(z - e_z)), round_T(relu(z + e_z))] (AO.h_interval)
  logits   = b2 + H @ W2 within e_l: which H of its interval the kernel holds, plus fp32 accumulation (AO.logit_err);
             the two-kernel actor then clamps to +-65 000 and stages them as fp16 (AO.stage_f16)
  q        within AO.q_bound of the expectation of those logits: dq/dl_k = p_k (s_k - E) / K times e_l, the exp2 argument's
             rounding (grows with |l - max|), v_exp_f32, the sums and the reciprocal
  actions  exactly AO.select of the kernel's own q (the selection rule is exact arithmetic: the q it reads decides)
For launches of 4 096 rows or more the oracle runs on the first tile, the last tile and a random sample of rows."""
import ctypes as C

import numpy as np
import pytest

from oracle import actor_oracle as AO

pytestmark = pytest.mark.gpu

HID, K51 = 512, 51
CODE = {"float32": 0, "bfloat16": 1, "float16": 2}
HB_ERR_INVALID = -1
# A bound that means something: on the moderate cases with tolerance.py's setting (logits within about +-5, support
# linspace(-25, 25): |q| <= 0.49) the largest q bound stays below tolerance.py's q_abs by a recorded margin. The bounds are
# computed on the host from the oracle (deterministic for these seeds); their largest values on those cases:
#   bf16: 6.2e-3 (658 bits, 20 actions) against q_abs 0.012: margin 1.9, asserted >= BOUND_MARGIN (1.5) up to 1 280 bits
#   fp16: 7.5e-4 (33 bits, 48 actions) against q_abs 0.003: margin 4.0, asserted >= BOUND_MARGIN up to 171 bits
# Beyond those sizes the bound (rigorous for every summation order of the fp32 accumulators, so linear in the number of set bits)
# grows past the fp16 q_abs (7.7e-3 at 1 280 bits) while the measured error stays at ~1e-7 (printed by the test).
BOUND_MARGIN = 1.5
MARGIN_MAX_BITS = {"bfloat16": 1280, "float16": 171}


def _q_abs(dtype):
    from hanabi_agents.rlax_dqn.tolerance import TOLERANCE

    return TOLERANCE[dtype]["q_abs"]


def _K():
    from hanabi_hip import _capi as K

    return K


def _lib():
    return _K().lib()


def _check(rc):
    _K().check(rc)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _tdt(name):
    import torch

    return getattr(torch, name)


def _dev(x, dtype="float32"):
    """float64 numpy -> device tensor of `dtype` and the values the kernel sees back in float64."""
    import torch

    t = torch.as_tensor(np.ascontiguousarray(x, np.float64)).to(_tdt(dtype)).cuda()
    return t, t.double().cpu().numpy()


def _host(t):
    return t.double().cpu().numpy()


def _stream():
    return _K().current_stream()


def _inside(got, lo, hi, what):
    got = np.asarray(got, float)
    ok = (got >= lo) & (got <= hi)
    if not ok.all():
        i = np.unravel_index(np.argmin(ok), ok.shape)
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.size} outside; first at {i}: got {got[i]!r} not in "
                             f"[{lo[i]!r}, {hi[i]!r}]")


def _close(got, ref, err, what):
    got = np.asarray(got, float)
    ok = np.abs(got - ref) <= err
    if not ok.all():
        i = np.unravel_index(np.argmin(ok), ok.shape)
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.size} outside the bound; first at {i}: got {got[i]!r}, "
                             f"ref {ref[i]!r}, err {err[i]!r}")


def _sample_rows(n, tile, seed):
    """every row of a small launch; else the first tile, the last tile and 256 random rows"""
    if n < 4096:
        return np.arange(n)
    rng = np.random.default_rng(seed)
    return np.unique(np.concatenate([np.arange(tile), np.arange(n - tile, n), rng.integers(0, n, 256)]))


def _bits_rows(n, obs_len, seed, garbage):
    """random bit rows [n, words] u32 (density 1/4) with every padding bit of the last word set when `garbage`, cleared
    otherwise; returns the words and a function giving the 0/1 observation rows of selected rows."""
    rng = np.random.default_rng(seed)
    words = (obs_len + 31) // 32
    w = rng.integers(0, 1 << 32, (n, words), dtype=np.uint64) & rng.integers(0, 1 << 32, (n, words), dtype=np.uint64)
    tail = obs_len % 32
    if tail:
        pad = np.uint64(((1 << 32) - 1) ^ ((1 << tail) - 1))
        w[:, -1] = (w[:, -1] | pad) if garbage else (w[:, -1] & ~pad & np.uint64(0xFFFFFFFF))
    w = w.astype(np.uint32)

    def obs_of(rows):
        b = (w[rows][:, :, None] >> np.arange(32, dtype=np.uint32)) & 1
        return b.reshape(len(rows), words * 32)[:, :obs_len].astype(float)

    return w, obs_of


SUPPORTS = {
    "lin": np.linspace(-25.0, 25.0, K51),
    "asym": np.concatenate([np.linspace(-3.0, 0.0, 20), np.linspace(0.5, 40.0, 31)]),
    "neg": -np.linspace(1.0, 30.0, K51)[::-1],
    "spike": np.concatenate([np.zeros(50), [400.0]]),
}


def _fused_net(obs_len, A, dtype, regime, seed):
    """W1 [obs_len + 3, 520] / W2 [512, A * 51 + 13] / b2 with NaN in every entry the packer must not read (rows >= obs_len,
    columns >= 512 of W1; columns >= A * 51 of W2 and b2). Logit regimes, each within an action: moderate (about +-2), wide
    (bias spread +-60), dominant (one atom 30 above the rest), equal (identical W2 columns and biases in an action), quarter (atoms
    of quarter a % 4 of action a (13 f .. 13 f + 12; quarter 3 holds the 12-atom tail 39..50) 40 above the rest, its last atom 5
    more: the maximum sits in the quarter's shared register 13 f + 12 for f < 3). fp16 keeps |H| < 10 and |logits| < 200:
    well inside its range."""
    rng = np.random.default_rng(seed)
    AK = A * K51
    w1 = np.full((obs_len + 3, HID + 8), np.nan)
    w1[:obs_len, :HID] = rng.standard_normal((obs_len, HID)) * (0.6 / np.sqrt(0.25 * obs_len + 1))
    b1 = rng.standard_normal(HID) * 0.1
    w2 = np.full((HID, AK + 13), np.nan)
    b2 = np.full(AK + 13, np.nan)
    w2[:, :AK] = rng.standard_normal((HID, AK)) * 0.1
    b2[:AK] = rng.standard_normal(AK) * 0.5
    bb = b2[:AK].reshape(A, K51)
    if regime == "wide":
        bb[:] = rng.uniform(-60, 60, (A, K51))
    elif regime == "dominant":
        bb[np.arange(A), rng.integers(0, K51, A)] += 30.0
    elif regime == "equal":
        for a in range(A):
            w2[:, a * K51:(a + 1) * K51] = w2[:, [a * K51]]
            bb[a] = bb[a, 0]
    elif regime == "quarter":
        for a in range(A):
            f = a % 4
            atoms = np.arange(13 * f, min(13 * f + 13, K51))
            bb[a, atoms] += 40.0
            bb[a, atoms[-1]] += 5.0
    b2[:AK] = bb.reshape(-1)
    if A >= 3 and regime != "equal":            # an exact tie: action 1 duplicates action 0 (both whole actions of one pass)
        w2[:, K51:2 * K51] = w2[:, :K51]
        b2[K51:2 * K51] = b2[:K51]
    return w1, b1, w2, b2


class _Fused:
    """fragment-major copies of one network (hb_actor_fused_pack_thin), with the k-contiguous copies checked to be exact."""

    def __init__(self, obs_len, A, dtype, regime, seed):
        import torch

        self.obs_len, self.A, self.dtype, self.code = obs_len, A, dtype, CODE[dtype]
        w1, b1, w2, b2 = _fused_net(obs_len, A, dtype, regime, seed)
        self.w1_d, self.w1 = _dev(w1, dtype)
        self.b1_d, self.b1 = _dev(b1, dtype)
        self.w2_d, self.w2 = _dev(w2, dtype)
        self.b2_d, self.b2 = _dev(b2, dtype)
        f1, f2, fb = C.c_int64(), C.c_int64(), C.c_int32()
        _check(_lib().hb_actor_fused_sizes(obs_len, HID, A, K51, C.byref(f1), C.byref(f2), C.byref(fb)))
        self.w1f = torch.zeros(f1.value, dtype=torch.uint8, device="cuda")
        self.w2f = torch.zeros(f2.value, dtype=torch.uint8, device="cuda")
        self.b1f = torch.zeros(HID, device="cuda")
        self.b2f = torch.zeros(fb.value, device="cuda")
        kp = (obs_len + 63) // 64 * 64
        w1t = torch.full((HID, kp + 8), 7.0, dtype=_tdt(dtype), device="cuda")
        w2t = torch.full((A * K51, HID + 8), 7.0, dtype=_tdt(dtype), device="cuda")
        _check(_lib().hb_actor_fused_pack_thin(_ptr(self.w1_d), HID + 8, _ptr(self.b1_d), _ptr(self.w2_d), A * K51 + 13,
                                              _ptr(self.b2_d), obs_len, HID, A, K51, _ptr(self.w1f), _ptr(self.b1f),
                                              _ptr(self.w2f), _ptr(self.b2f), _ptr(w1t), kp + 8, _ptr(w2t), HID + 8, self.code,
                                              _stream()))
        torch.cuda.synchronize()
        # the thin copies: exact transposes, zero K padding, the stride's tail untouched
        t1, t2 = _host(w1t), _host(w2t)
        np.testing.assert_array_equal(t1[:, :obs_len], self.w1[:obs_len, :HID].T)
        assert (t1[:, obs_len:kp] == 0).all() and (t1[:, kp:] == 7).all()
        np.testing.assert_array_equal(t2[:, :HID], self.w2[:, :A * K51].T)
        assert (t2[:, HID:] == 7).all()
        np.testing.assert_array_equal(_host(self.b1f), self.b1)

    def oracle(self, obs, support):
        """q reference and bound for 0/1 observation rows obs [r, obs_len]"""
        w1, b1 = self.w1[:self.obs_len, :HID], self.b1
        w2, b2 = self.w2[:, :self.A * K51], self.b2[:self.A * K51]
        z = obs @ w1 + b1
        lo, hi = AO.h_interval(z, AO.layer1_err(obs, w1, b1), self.dtype)
        h = AO.round_to(AO.relu(z), self.dtype)
        logits = h @ w2 + b2
        e_l = AO.logit_err(lo, hi, h, w2, b2)
        r = obs.shape[0]
        logits, e_l = logits.reshape(r, self.A, K51), e_l.reshape(r, self.A, K51)
        return AO.expectation(logits, support), AO.q_bound(logits, e_l, support), logits

    def q(self, bits_d, n, support_d, q):
        _check(_lib().hb_actor_fused_q_dt(_ptr(bits_d), n, self.obs_len, _ptr(self.w1f), _ptr(self.b1f), _ptr(self.w2f),
                                         _ptr(self.b2f), _ptr(support_d), HID, self.A, K51, _ptr(q), self.code, _stream()))

    def act(self, bits_d, legal_d, n, support_d, q, eps, seed, draw, gid, actions):
        _check(_lib().hb_actor_fused_act_dt(_ptr(bits_d), _ptr(legal_d), n, self.obs_len, _ptr(self.w1f), _ptr(self.b1f),
                                           _ptr(self.w2f), _ptr(self.b2f), _ptr(support_d), HID, self.A, K51, _ptr(q), eps,
                                           seed, draw, gid, _ptr(actions), self.code, _stream()))


REGIMES = ["moderate", "wide", "dominant", "equal", "quarter"]
SUPS = ["lin", "asym", "neg", "spike"]
A_LIST = [1, 8, 9, 10, 11, 19, 20, 30, 38, 48, 64, 79, 80]
OBS_LIST = [1, 31, 32, 33, 63, 64, 65, 171, 658, 1280, 4096]
ROWS_LIST = [1, 127, 128, 129, 4133, 32768]
# every A with both dtypes; obs_len, rows, regime and support cycle so that every value of each list is met
FUSED_CASES = []
for _i, _A in enumerate(A_LIST):
    for _d, _dt in enumerate(("bfloat16", "float16")):
        _rows = ROWS_LIST[(2 * _i + _d) % 6]
        _obs = OBS_LIST[(_i + 5 * _d) % 11]
        if _rows == 32768 and _obs > 1280:
            _obs = 658                           # (the 4 096-bit rows are met at 4 133 rows: 16 MB of bits is enough)
        FUSED_CASES.append((_dt, _A, _obs, _rows, REGIMES[(_i + _d) % 5], SUPS[(_i + 3 * _d) % 4]))
# the moderate regime at the two benched shapes, for the bound-meaning check
FUSED_CASES += [("bfloat16", 20, 658, 4133, "moderate", "lin"), ("float16", 48, 1280, 129, "moderate", "lin"),
                ("bfloat16", 2, 171, 129, "moderate", "lin"), ("float16", 2, 658, 4133, "wide", "asym"),
                ("bfloat16", 63, 658, 127, "quarter", "neg"), ("float16", 63, 33, 129, "moderate", "lin"),
                ("bfloat16", 48, 1280, 129, "quarter", "asym"), ("float16", 20, 658, 128, "quarter", "spike")]


@pytest.mark.parametrize("dtype,A,obs_len,n,regime,sup", FUSED_CASES)
def test_fused_actor_q_equals_f64_oracle(dtype, A, obs_len, n, regime, sup):
    """hb_actor_fused_pack_thin + hb_actor_fused_q_dt (and hb_actor_fused_act_dt for A <= 64) on crafted networks: q within the
    oracle's bound for every checked row; garbage in the padding bits of each row's last word and NaN in every weight entry the
    packer must skip change nothing (q finite and bit-identical to clean padding); act_dt writes bit-identical q and exactly the
    oracle's selection on it (epsilon 0, 0.25 and 1; seeds, draws and game ids with their high words set)."""
    import torch

    net = _Fused(obs_len, A, dtype, regime, seed=A * 7919 + obs_len + n)
    support = SUPPORTS[sup]
    sup_d, sup_v = _dev(support)
    bits, obs_of = _bits_rows(n, obs_len, seed=n + A, garbage=True)
    clean, _ = _bits_rows(n, obs_len, seed=n + A, garbage=False)
    bits_d = torch.from_numpy(bits.view(np.int32)).cuda()
    clean_d = torch.from_numpy(clean.view(np.int32)).cuda()
    q = torch.full((n, A), float("nan"), device="cuda")
    q_clean = torch.full((n, A), float("nan"), device="cuda")
    net.q(bits_d, n, sup_d, q)
    net.q(clean_d, n, sup_d, q_clean)
    torch.cuda.synchronize()
    qh = _host(q)
    assert np.isfinite(qh).all()
    assert torch.equal(q, q_clean), "padding bits of the last word changed q"
    rows = _sample_rows(n, 128, seed=n)
    ref, err, logits = net.oracle(obs_of(rows), sup_v)
    _close(qh[rows], ref, err, f"fused q {dtype} A={A} obs_len={obs_len} {regime}")
    print(f"fused {dtype} A={A} obs_len={obs_len} n={n} {regime} {sup}: max |dq| {np.abs(qh[rows] - ref).max():.3e}, "
          f"max bound {err.max():.3e}")
    if regime == "moderate" and sup == "lin" and obs_len <= MARGIN_MAX_BITS[dtype]:
        assert err.max() * BOUND_MARGIN <= _q_abs(dtype), (err.max(), _q_abs(dtype))
    if regime == "quarter":   # the branch is forced: each action's maximum quarter is >= 30 above its other quarters
        for a in range(2 if A >= 3 else 0, A):
            inq = np.arange(13 * (a % 4), min(13 * (a % 4) + 13, K51))
            gap = logits[:, a, inq].max(-1) - np.delete(logits[:, a], inq, axis=-1).max(-1)
            assert (gap >= 30).all(), (a, gap.min())
    if A >= 3 and regime != "equal":
        assert np.array_equal(qh[:, 0], qh[:, 1]), "duplicated actions must give equal q"
    if A <= 64:
        rng = np.random.default_rng(n)
        legal = (rng.random((n, A)) < 0.6).astype(np.int8)
        legal[::7] = 0                                   # every action illegal
        legal[3::11, :] = 0
        legal[3::11, A - 1] = 1                          # one legal action, the last
        legal[1::5, :2] = 1                              # the tie 0 / 1 legal
        legal_d = torch.from_numpy(legal).cuda()
        for eps, seed, draw, gid in ((0.0, 5, 1, 0), (0.25, (0xABCD << 32) | 17, (5 << 32) | 3, (1 << 32) - 5),
                                     (1.0, (3 << 32) | 2, 9, (1 << 40) + 7)):
            acts = torch.full((n,), -7, dtype=torch.int32, device="cuda")
            q2 = torch.full((n, A), float("nan"), device="cuda")
            net.act(bits_d, legal_d, n, sup_d, q2, eps, seed, draw, gid, acts)
            torch.cuda.synchronize()
            assert torch.equal(q2, q)
            np.testing.assert_array_equal(acts.cpu().numpy(), AO.select(qh, legal, eps, seed, draw, gid), f"eps {eps}")


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_fused_actor_grouped_uses_each_tiles_network(dtype):
    """hb_actor_fused_act_grouped with two networks over five tiles (one inactive): every active tile's q within its own
    network's oracle bound and bit-identical to hb_actor_fused_act_dt over the tile's rows; actions exactly the oracle's selection
    with the tile's game id (one of them 2^32 - 5); the inactive tile's outputs untouched."""
    import torch

    obs_len, A, n = 171, 11, 5 * 128
    nets = [_Fused(obs_len, A, dtype, "moderate", seed=1), _Fused(obs_len, A, dtype, "wide", seed=2)]
    sups = [_dev(SUPPORTS["lin"]), _dev(SUPPORTS["asym"])]
    bits, obs_of = _bits_rows(n, obs_len, seed=3, garbage=True)
    bits_d = torch.from_numpy(bits.view(np.int32)).cuda()
    legal = _legal_cases(n, A, np.random.default_rng(4))
    legal_d = torch.from_numpy(legal).cuda()
    plan = [(0, 100, 1), (1, (1 << 32) - 5, 1), (0, 7, 0), (1, 1 << 40, 1), (1, 0, 1)]   # (network, first game id, active)
    Tile = _K().HbFusedTile
    tiles = (Tile * 5)()
    for t, (k, g, on) in enumerate(plan):
        nt = nets[k]
        tiles[t] = Tile(nt.w1f.data_ptr(), nt.b1f.data_ptr(), nt.w2f.data_ptr(), nt.b2f.data_ptr(), sups[k][0].data_ptr(), g, on, 0)
    tiles_d = torch.frombuffer(bytearray(bytes(tiles)), dtype=torch.uint8).cuda()
    for eps, seed, draw in ((0.0, 2, 3), (0.25, (9 << 32) | 1, (1 << 32) | 6), (1.0, 4, (2 << 32) | 1)):
        q = torch.full((n, A), -3.0, device="cuda")
        acts = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        _check(_lib().hb_actor_fused_act_grouped(_ptr(tiles_d), n, _ptr(bits_d), _ptr(legal_d), obs_len, HID, A, K51, _ptr(q),
                                                 eps, seed, draw, _ptr(acts), CODE[dtype], _stream()))
        torch.cuda.synchronize()
        qh, ah = _host(q), acts.cpu().numpy()
        for t, (k, g, on) in enumerate(plan):
            r = np.arange(128 * t, 128 * t + 128)
            if not on:
                assert (qh[r] == -3.0).all() and (ah[r] == -7).all()
                continue
            ref, err, _ = nets[k].oracle(obs_of(r), sups[k][1])
            _close(qh[r], ref, err, f"grouped tile {t}")
            np.testing.assert_array_equal(ah[r], AO.select(qh[r], legal[r], eps, seed, draw, g), f"tile {t} eps {eps}")
            q1 = torch.empty((128, A), device="cuda")
            a1 = torch.empty((128,), dtype=torch.int32, device="cuda")
            nets[k].act(bits_d[128 * t:].contiguous(), legal_d[128 * t:].contiguous(), 128, sups[k][0], q1, eps, seed, draw, g, a1)
            torch.cuda.synchronize()
            assert torch.equal(q1, q[128 * t:128 * t + 128]) and torch.equal(a1, acts[128 * t:128 * t + 128])


# ---- two-kernel actor -----------------------------------------------------------------------------------------------------------
def _pack(w, bias, k_rows, n_cols, w_ld, group_cols, k_pad, n_out):
    """hb_actor_pack_weights on one job into zeroed outputs wt [n_out, k_pad] bf16 / bias_out [n_out] fp32"""
    import torch

    wt = torch.zeros((n_out, k_pad), dtype=torch.bfloat16, device="cuda")
    bo = torch.zeros(n_out, device="cuda")
    job = _K().HbPackJob(w.data_ptr(), bias.data_ptr(), wt.data_ptr(), bo.data_ptr(), k_rows, n_cols, w_ld, group_cols, k_pad)
    _check(_lib().hb_actor_pack_weights(C.byref(job), 1, _stream()))
    torch.cuda.synchronize()
    return wt, bo


def _phys(n, group_cols):
    n = np.asarray(n)
    return n if group_cols == 0 else (n // group_cols) * 256 + n % group_cols


@pytest.mark.parametrize("k_rows,n_cols,group_cols,k_pad", [(658, 512, 0, 704), (512, 1020, 255, 512), (64, 147, 252, 64),
                                                            (1, 256, 0, 64), (192, 2 * 129, 129, 192), (64, 64 * 4, 256, 64)])
def test_pack_weights_is_an_exact_transpose(k_rows, n_cols, group_cols, k_pad):
    """hb_actor_pack_weights: wt[n', k] == W[k, n] and bias_out[n'] == float(bias[n]) bit for bit with n' = (n / group_cols) * 256
    + n % group_cols; every entry no input maps to stays zero; W's row-stride tail (NaN) is never read."""
    rng = np.random.default_rng(k_rows + n_cols)
    w = np.full((k_rows, n_cols + 5), np.nan)
    w[:, :n_cols] = rng.standard_normal((k_rows, n_cols)) * 3
    w_d, w_v = _dev(w, "bfloat16")
    b_d, b_v = _dev(rng.standard_normal(n_cols) * 100, "bfloat16")
    n_out = int(_phys(n_cols - 1, group_cols)) + 1
    wt, bo = _pack(w_d, b_d, k_rows, n_cols, n_cols + 5, group_cols, k_pad, n_out)
    want = np.zeros((n_out, k_pad))
    wantb = np.zeros(n_out)
    ph = _phys(np.arange(n_cols), group_cols)
    want[ph, :k_rows] = w_v[:, :n_cols].T
    wantb[ph] = b_v
    np.testing.assert_array_equal(_host(wt), want)
    np.testing.assert_array_equal(_host(bo), wantb)


HIDDEN_CASES = [(256, 1, 1), (512, 31, 255), (1024, 32, 256), (256, 33, 257), (512, 63, 4133), (1024, 64, 1),
                (256, 65, 255), (512, 171, 256), (1024, 658, 257), (512, 1280, 4133), (256, 4096, 257)]


@pytest.mark.parametrize("hidden,obs_len,n", HIDDEN_CASES)
def test_actor_hidden_pinned_to_the_h_interval(hidden, obs_len, n):
    """hb_actor_hidden (int8 rows) and hb_actor_hidden_packed (bit rows) on weights from hb_actor_pack_weights: every H inside
    [round_bf16(relu(z - e_z)), round_bf16(relu(z + e_z))], i.e. exact wherever that interval is one value; the two forms
    bit-identical, and garbage padding bits in the last word of a bit row leave H bit-identical (the packer's zero K rows)."""
    import torch

    rng = np.random.default_rng(hidden + obs_len + n)
    kp = (obs_len + 63) // 64 * 64
    w1 = rng.standard_normal((obs_len, hidden)) * (0.6 / np.sqrt(0.25 * obs_len + 1))
    w_d, w_v = _dev(w1, "bfloat16")
    b_d, b_v = _dev(rng.standard_normal(hidden) * 0.1, "bfloat16")
    w1t, b1f = _pack(w_d, b_d, obs_len, hidden, hidden, 0, kp, hidden)
    bits, obs_of = _bits_rows(n, obs_len, seed=n, garbage=True)
    clean, _ = _bits_rows(n, obs_len, seed=n, garbage=False)
    obs8 = torch.from_numpy(obs_of(np.arange(n)).astype(np.int8)).cuda()
    outs = []
    for src, packed in ((obs8, False), (torch.from_numpy(bits.view(np.int32)).cuda(), True),
                        (torch.from_numpy(clean.view(np.int32)).cuda(), True)):
        h = torch.full((n, hidden), float("nan"), dtype=torch.bfloat16, device="cuda")
        fn = _lib().hb_actor_hidden_packed if packed else _lib().hb_actor_hidden
        _check(fn(_ptr(src), n, obs_len, _ptr(w1t), kp, _ptr(b1f), hidden, _ptr(h), _stream()))
        outs.append(h)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[1], outs[2])
    rows = _sample_rows(n, 256, seed=n)
    obs = obs_of(rows)
    z = obs @ w_v + b_v
    lo, hi = AO.h_interval(z, AO.layer1_err(obs, w_v, b_v), "bfloat16")
    _inside(_host(outs[0])[rows], lo, hi, "H")
    # the interval pins most H exactly; fewer once a row holds hundreds of set bits (the bound allows every summation order)
    assert (lo == hi).mean() > (0.9 if obs_len <= 171 else 0.5)


ACTOR_Q_SUPPORTS = {"lin": lambda K: np.linspace(-25.0, 25.0, K), "skew": lambda K: np.linspace(-3.0, 40.0, K)}


def _actor_q_setup(A, K, hidden, n, regime, sup, seed, dup=True):
    """H bf16 [n, hidden] and an output layer of A actions x K atoms packed with group_cols = (256 / K) K; support
    ACTOR_Q_SUPPORTS[sup]. Regimes: moderate; f16 (logits about 1 000 +- 8: fp16 staging (half an ulp = 0.25) dominates the
    bound); clamp (action 0 reads no H (zero W2 columns) and its atoms cycle through biases 70 000, 64 768, -70 000, 64 512, 0:
    the +-70 000 atoms lie beyond the +-65 000 clamp and stage exactly to +-64 992, the others are fp16 values staged exactly,
    so the clamped maximum decides q and the bound stays small)."""
    rng = np.random.default_rng(seed)
    AK = A * K
    h_d, h_v = _dev(np.maximum(rng.standard_normal((n, hidden)), 0) * 0.7, "bfloat16")
    w2 = rng.standard_normal((hidden, AK)) * (0.5 / np.sqrt(hidden))
    b2 = rng.standard_normal(AK) * 0.5
    if regime == "f16":
        b2 += 1000.0
        w2 *= 8.0
    if regime == "clamp":
        w2[:, :K] = 0.0
        b2[:K] = np.array([70000.0, 64768.0, -70000.0, 64512.0, 0.0])[np.arange(K) % 5]
    if dup and A >= 2:
        w2[:, K:2 * K], b2[K:2 * K] = w2[:, :K], b2[:K]
    w2_d, w2_v = _dev(w2, "bfloat16")
    b2_d, b2_v = _dev(b2, "bfloat16")
    gc = (256 // K) * K
    n_out = (-(-A // (256 // K))) * 256
    w2t, b2f = _pack(w2_d, b2_d, hidden, AK, AK, gc, hidden, n_out)
    sup_d, sup_v = _dev(ACTOR_Q_SUPPORTS[sup](K))

    def oracle(rows):
        l = h_v[rows] @ w2_v + b2_v
        e_l = AO.dot_err(np.abs(h_v[rows]), np.abs(w2_v), np.abs(b2_v), hidden + 1)
        c, e = AO.stage_f16(l, e_l)
        r = len(rows)
        c, e = c.reshape(r, A, K), e.reshape(r, A, K)
        return AO.expectation(c, sup_v), AO.q_bound(c, e, sup_v), c

    return h_d, w2t, b2f, sup_d, oracle


# (n_atoms, n_actions, hidden, regime, support); A = 2, 63 and 64 reach hb_actor_q_select's selection limits
ACTOR_Q_CASES = [(2, 1, 64, "moderate", "lin"), (7, 5, 192, "f16", "skew"), (21, 6, 512, "moderate", "lin"),
                 (51, 11, 64, "clamp", "skew"), (64, 20, 192, "moderate", "lin"), (85, 48, 512, "f16", "skew"),
                 (128, 5, 64, "moderate", "lin"), (129, 6, 192, "clamp", "lin"), (256, 11, 512, "moderate", "skew"),
                 (51, 20, 512, "f16", "lin"), (51, 48, 512, "moderate", "skew"), (2, 48, 192, "clamp", "lin"),
                 (51, 2, 192, "moderate", "lin"), (51, 63, 64, "clamp", "skew"), (51, 64, 512, "f16", "lin"),
                 (4, 64, 192, "moderate", "skew")]


@pytest.mark.parametrize("K,A,hidden,regime,sup", ACTOR_Q_CASES)
def test_actor_q_equals_f64_oracle(K, A, hidden, regime, sup):
    """hb_actor_q: 1 .. 128 actions per 256-column group and the unrolled 51-atom epilogue; q within the bound of the clamped,
    fp16-staged logits (atoms beyond +-65 000 staged exactly to the clamp's fp16 value); hb_actor_q_select with its tickets
    (called three times: each call must re-arm them) writes bit-identical q and exactly the oracle's selection for epsilon 0,
    0.25 and 1, rows with every action illegal, a single legal action at A - 1, and every action legal."""
    import torch

    n = 300
    h_d, w2t, b2f, sup_d, oracle = _actor_q_setup(A, K, hidden, n, regime, sup, seed=K * 100 + A)
    q = torch.full((n, A), float("nan"), device="cuda")
    _check(_lib().hb_actor_q(_ptr(h_d), n, hidden, _ptr(w2t), _ptr(b2f), _ptr(sup_d), A, K, _ptr(q), _stream()))
    torch.cuda.synchronize()
    qh = _host(q)
    assert np.isfinite(qh).all()
    ref, err, staged = oracle(np.arange(n))
    _close(qh, ref, err, f"actor_q K={K} A={A} {regime}")
    if regime == "clamp":      # the beyond-range atoms stage exactly, and the bound on action 0 is far below |q|'s scale
        assert (np.abs(staged[:, 0]) <= 64992).all() and (staged[:, 0].max(-1) == 64992).all()
        assert err[:, 0].max() < 0.05, err[:, 0].max()
    if A >= 2:
        assert np.array_equal(qh[:, 0], qh[:, 1])
    if A > 64:
        return
    legal = _legal_cases(n, A, np.random.default_rng(A))
    legal[1::6, :2] = 1
    legal_d = torch.from_numpy(legal).cuda()
    tickets = torch.zeros(-(-n // 256), dtype=torch.int32, device="cuda")
    for eps, seed, draw, gid in ((0.0, 3, 1, 0), (0.25, (1 << 32) | 3, (7 << 32) | 2, (1 << 32) - 5), (1.0, 8, (1 << 33) | 5, 77)):
        q2 = torch.full((n, A), float("nan"), device="cuda")
        acts = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        _check(_lib().hb_actor_q_select(_ptr(h_d), n, hidden, _ptr(w2t), _ptr(b2f), _ptr(sup_d), A, K, _ptr(q2), _ptr(legal_d),
                                        eps, seed, draw, gid, _ptr(acts), _ptr(tickets), _stream()))
        torch.cuda.synchronize()
        assert torch.equal(q2, q)
        np.testing.assert_array_equal(acts.cpu().numpy(), AO.select(qh, legal, eps, seed, draw, gid), f"eps {eps}")
        assert (tickets.cpu().numpy() == 0).all(), "tickets not re-armed"


# ---- selection --------------------------------------------------------------------------------------------------------------------
def _legal_cases(n, A, rng):
    legal = (rng.random((n, A)) < 0.5).astype(np.int8)
    legal[::13] = 0                          # every action illegal
    legal[5::13] = 0
    legal[5::13, A - 1] = 1                  # a single legal action at A - 1
    legal[7::13] = 1                         # every action legal
    return legal


@pytest.mark.parametrize("A", [1, 2, 63, 64])
def test_policy_select_equals_oracle_rule(A):
    """hb_policy_select on crafted q (few distinct values: exact ties everywhere) for epsilon 0, 0.25 and 1, seeds, draws and game
    ids with their high words set: every action exactly the oracle's."""
    import torch

    n = 3000
    rng = np.random.default_rng(A)
    q = rng.integers(-2, 3, (n, A)).astype(np.float32) * np.float32(0.125)
    legal = _legal_cases(n, A, rng)
    q_d, legal_d = torch.from_numpy(q).cuda(), torch.from_numpy(legal).cuda()
    for eps in (0.0, 0.25, 1.0):
        for seed, draw, gid in ((1, 2, 0), ((5 << 32) | 1, (3 << 32) | 8, (1 << 32) - 5)):
            acts = torch.full((n,), -7, dtype=torch.int32, device="cuda")
            _check(_lib().hb_policy_select(_ptr(q_d), _ptr(legal_d), n, A, eps, seed, draw, gid, _ptr(acts), _stream()))
            torch.cuda.synchronize()
            np.testing.assert_array_equal(acts.cpu().numpy(), AO.select(q, legal, eps, seed, draw, gid), f"eps {eps}")


@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
@pytest.mark.parametrize("A,K,pad", [(1, 51, 0), (2, 51, 5), (63, 51, 0), (64, 51, 0), (64, 64, 3), (20, 51, 4)])
def test_policy_act_equals_oracle(dtype, A, K, pad):
    """hb_policy_act (logits [n, A * K + pad] in fp32 / bf16 / fp16, NaN in the padding): q within the oracle's bound of the
    exact logits and the actions exactly the oracle's selection on that q. A = 64 is the C-ABI's limit: its per-game action mask
    must not be built with a 64-bit shift by 64 (which left the mask empty and every row's action 0)."""
    import torch

    n = 700
    rng = np.random.default_rng(A * K + pad)
    AK, rs = A * K, A * K + pad
    lg = np.full((n, rs), np.nan)
    lg[:, :AK] = rng.standard_normal((n, AK)) * 2
    lg[::3, :AK] += rng.uniform(-40, 40, (len(lg[::3]), AK))
    if A >= 2:
        lg[:, K:2 * K] = lg[:, :K]                         # exact q ties between actions 0 and 1
    lg_d, lg_v = _dev(lg, dtype)
    support = np.linspace(-25.0, 25.0, K)
    sup_d, sup_v = _dev(support)
    legal = _legal_cases(n, A, rng)
    legal[2::13, :2] = 1
    legal_d = torch.from_numpy(legal).cuda()
    l = lg_v[:, :AK].reshape(n, A, K)
    ref, err = AO.expectation(l, sup_v), AO.q_bound(l, np.zeros_like(l), sup_v)
    for eps, seed, draw, gid in ((0.0, 4, 1, 0), (0.25, (1 << 33) | 4, (1 << 32) | 1, (1 << 32) - 5), (1.0, 6, 2, 9)):
        q = torch.full((n, A), float("nan"), device="cuda")
        acts = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        _check(_lib().hb_policy_act(_ptr(lg_d), CODE[dtype], _ptr(legal_d), _ptr(sup_d), n, A, K, rs, eps, seed, draw, gid,
                                    _ptr(acts), _ptr(q), _stream()))
        torch.cuda.synchronize()
        qh = _host(q)
        _close(qh, ref, err, f"policy_act q {dtype}")
        np.testing.assert_array_equal(acts.cpu().numpy(), AO.select(qh, legal, eps, seed, draw, gid), f"eps {eps}")


def test_policy_act_64_actions_picks_the_only_legal_action():
    """regression: with 64 actions and only action 63 legal, hb_policy_act must choose 63 in every row, greedy or exploring."""
    import torch

    n, A, K = 64, 64, 2
    lg_d, _ = _dev(np.random.default_rng(0).standard_normal((n, A * K)))
    sup_d, _ = _dev([-1.0, 1.0])
    legal = np.zeros((n, A), np.int8)
    legal[:, 63] = 1
    for eps in (0.0, 1.0):
        acts = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        _check(_lib().hb_policy_act(_ptr(lg_d), 0, _ptr(torch.from_numpy(legal).cuda()), _ptr(sup_d), n, A, K, A * K, eps, 1, 2,
                                    0, _ptr(acts), None, _stream()))
        torch.cuda.synchronize()
        assert (acts.cpu().numpy() == 63).all()


def test_selection_entry_points_refuse_more_than_64_actions():
    """refused by the host-side checks, before any launch"""
    import torch

    x = torch.zeros(64 * 65 * 2, device="cuda")
    a = torch.zeros(64, dtype=torch.int32, device="cuda")
    L, s = _lib(), _stream()
    assert L.hb_policy_act(_ptr(x), 0, _ptr(a), _ptr(x), 1, 65, 2, 130, 0.0, 0, 0, 0, _ptr(a), None, s) == HB_ERR_INVALID
    assert L.hb_policy_select(_ptr(x), _ptr(a), 1, 65, 0.0, 0, 0, 0, _ptr(a), s) == HB_ERR_INVALID
    assert L.hb_policy_select(_ptr(x), _ptr(a), 1, 0, 0.0, 0, 0, 0, _ptr(a), s) == HB_ERR_INVALID
    assert L.hb_actor_fused_act_dt(_ptr(a), _ptr(a), 1, 40, _ptr(x), _ptr(x), _ptr(x), _ptr(x), _ptr(x), HID, 65, K51, _ptr(x),
                                   0.0, 0, 0, 0, _ptr(a), 1, s) == HB_ERR_INVALID


# ---- learner forward: hb_thin_gemm ----------------------------------------------------------------------------------------------
THIN_CASES = [  # m, n, k, batch, dtype, fp32 out, relu, bias ("none" | "one" | "per")
    (32, 16, 32, 1, "bfloat16", False, True, "one"),
    (64, 48, 64, 2, "float16", True, False, "per"),
    (256, 1024, 704, 2, "bfloat16", True, False, "per"),
    (256, 1040, 1280, 1, "float16", False, True, "none"),
    (64, 1040, 32, 2, "bfloat16", False, False, "per"),
    (32, 48, 1280, 2, "float16", False, True, "per"),
    (32768, 1040, 64, 2, "bfloat16", False, True, "per"),
    (32768, 48, 704, 1, "float16", True, True, "one"),
]


@pytest.mark.parametrize("m,n,k,batch,dtype,out32,relu,bias", THIN_CASES)
def test_thin_gemm_equals_f64_product(m, n, k, batch, dtype, out32, relu, bias):
    """hb_thin_gemm with bf16 / fp16 operands (bit 2), 16-bit / fp32 output (bit 1), ReLU (bit 0) on and off, bias absent, one
    row or one per batch entry; a strided {online, target} pair of batch entries; ldx > k with NaN beyond k and ldo > n with
    sentinel columns that must stay untouched; row 0 of x zero and some biases -0 (pre-activations exactly +-0). fp32 outputs
    within the accumulation bound of the f64 product; rounded outputs pinned to [round(ref - e), round(ref + e)]. At m = 32 768
    the launch splits into one launch per column tile."""
    import torch

    rng = np.random.default_rng(m + n + k)
    ldx, ldw, ldo = k + 8, k + 16, n + 4
    x = np.full((batch, m, ldx), np.nan)
    x[:, :, :k] = rng.standard_normal((batch, m, k)) * 0.5
    x[:, 0, :k] = 0.0
    wt = np.full((batch, n, ldw), np.nan)
    wt[:, :, :k] = rng.standard_normal((batch, n, k)) * (1.0 / np.sqrt(k))
    x_d, x_v = _dev(x, dtype)
    w_d, w_v = _dev(wt, dtype)
    b_v = None
    if bias != "none":
        bb = rng.standard_normal((batch, n)) * 0.3
        if bias == "one":
            bb[:] = bb[0]
        bb[:, ::5] = -0.0
        b_d, b_v = _dev(bb, dtype)
    odt = "float32" if out32 else dtype
    sentinel = 12.5
    out = torch.full((batch, m, ldo), sentinel, dtype=_tdt(odt), device="cuda")
    flags = (1 if relu else 0) | (2 if out32 else 0) | (4 if dtype == "float16" else 0)
    _check(_lib().hb_thin_gemm(_ptr(x_d), _ptr(w_d), _ptr(b_d) if b_v is not None else None, _ptr(out), m, n, k, ldx, ldw, ldo,
                               batch, m * ldx, n * ldw, m * ldo, flags, _stream()))
    torch.cuda.synchronize()
    rows = _sample_rows(m, 32, seed=m + n)
    o = _host(out[:, torch.as_tensor(rows, device="cuda")])
    assert (o[:, :, n:] == sentinel).all(), "columns beyond n written"
    for z in range(batch):
        ref, err = AO.thin_gemm(x_v[z][rows, :k], w_v[z][:, :k], None if b_v is None else b_v[z], relu)
        if out32:
            _close(o[z, :, :n], ref, err, f"thin fp32 batch {z}")
        else:
            pre_lo, pre_hi = ref - err, ref + err
            _inside(o[z, :, :n], AO.round_to(pre_lo, dtype), AO.round_to(pre_hi, dtype), f"thin {dtype} batch {z}")
        if 0 in rows:
            r0 = o[z, list(rows).index(0), :n]
            want0 = np.zeros(n) if b_v is None else b_v[z]
            np.testing.assert_array_equal(r0, np.maximum(want0, 0) if relu else want0)


# ---- column sums ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
@pytest.mark.parametrize("rows,cols", [(1, 1), (17, 63), (1000, 64), (4133, 65), (256, 520)])
def test_colsum_and_relu_bwd_colsum_equal_f64(dtype, rows, cols):
    """hb_colsum: column sums within the bound of its fixed fp32 order. hb_relu_bwd_colsum (act rows act_ld = cols + 3 apart):
    dy masked in place exactly where act > 0 — act = +0 and -0 mask, NaN never appears — and its column sums within the same
    bound."""
    import torch

    rng = np.random.default_rng(rows * 7 + cols)
    x = rng.standard_normal((rows, cols)) * np.exp(rng.uniform(-3, 3, (rows, 1)))
    x_d, x_v = _dev(x, dtype)
    out = torch.full((cols,), float("nan"), device="cuda")
    _check(_lib().hb_colsum(_ptr(x_d), CODE[dtype], rows, cols, _ptr(out), _stream()))
    act = rng.standard_normal((rows, cols + 3))
    sel = rng.random((rows, cols)) < 0.3
    act[:, :cols][sel] = np.where(rng.random(sel.sum()) < 0.5, 0.0, -0.0)
    act_d, act_v = _dev(act, dtype)
    dy_d, dy_v = _dev(x, dtype)
    out2 = torch.full((cols,), float("nan"), device="cuda")
    _check(_lib().hb_relu_bwd_colsum(_ptr(dy_d), _ptr(act_d), cols + 3, CODE[dtype], rows, cols, _ptr(out2), _stream()))
    torch.cuda.synchronize()
    s, e = AO.colsum(x_v)
    _close(_host(out), s, e, "colsum")
    masked, s2, e2 = AO.relu_bwd_colsum(dy_v, act_v[:, :cols])
    np.testing.assert_array_equal(_host(dy_d), masked)
    _close(_host(out2), s2, e2, "relu_bwd_colsum")
