"""GPU: the learner kernels (csrc/learner.hip, csrc/learner2.hip, csrc/sum_tree.hip) called directly through the C-ABI on
crafted inputs and held against the float64 oracle (oracle/learner_oracle.py) run on exactly the same values: 16-bit inputs
are upcast to float64 before the oracle sees them, so the input dtype never enters a tolerance.

Tolerances are first-order error bounds of the kernel's fp32 arithmetic (unit roundoff u = 2^-24), computed per element from
the oracle's own intermediate values and doubled to cover products of first-order terms; each is derived next to its use.
An output the kernel rounds to a dtype T is checked as an interval: the fp32 value v satisfies |v - ref| <= e, rounding is
monotone, so round_T(ref - e) <= round_T(v) <= round_T(ref + e). Where both ends round alike this pins the bits exactly."""
import ctypes as C

import numpy as np
import pytest

from oracle import learner_oracle as LO

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
DTYPES = ["float32", "bfloat16", "float16"]
CODE = {"float32": 0, "bfloat16": 1, "float16": 2}
HB_ERR_INVALID = -1


def _K():
    from hanabi_hip import _capi as K

    return K


def _tdt(name):
    import torch

    return getattr(torch, name)


def _dev(x, dtype="float32"):
    """float64 numpy -> device tensor of `dtype` (the values the kernel sees) and those values back in float64."""
    import torch

    t = torch.as_tensor(np.asarray(x, np.float64)).to(_tdt(dtype)).cuda()
    return t, t.double().cpu().numpy()


def _host(t):
    return t.double().cpu().numpy()


def _within(got, ref, err, dtype="float32"):
    """round_T(ref - err) <= got <= round_T(ref + err) elementwise (NaN in got fails)."""
    import torch

    ref = np.asarray(ref, float)
    err = np.broadcast_to(np.asarray(err, float), ref.shape)
    to_t = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float64)).float().to(_tdt(dtype)).double().numpy()
    lo, hi = to_t(ref - err), to_t(ref + err)
    g = np.asarray(got, float)
    ok = (g >= lo) & (g <= hi)
    if not ok.all():
        i = np.unravel_index(np.argmin(ok), ok.shape)
        raise AssertionError(f"{int((~ok).sum())} of {ok.size} outside the bound; first at {i}: got {g[i]!r}, "
                             f"ref {ref[i]!r}, err {err[i]!r}")


def _half_ulp(x, dtype):
    mant, emin = {"float32": (23, -126), "bfloat16": (7, -126), "float16": (10, -14)}[dtype]
    e = np.maximum(np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** -200))), emin)
    return 2.0 ** (e - mant - 1)


# ---- C51 loss: hb_c51_loss_sparse and hb_c51_loss_grad ---------------------------------------------------------------------
SHAPES = [(1, 51), (5, 21), (11, 51), (20, 51), (21, 51), (32, 51), (48, 51), (64, 64), (20, 2)]
# (beta, bias given, mask_terminal, padded row stride): every combination of each column appears across the batch sizes
CONFIGS = [(-0.5, True, 1, True), (0.0, False, 0, False), (0.4, True, 0, True), (1.0, False, 1, True)]
VMAX = 25.0
GAP = 1e-3   # smallest f64 gap between the best and the second-best selector q outside deliberate ties: far above the kernel's
             # q error (relative ~ (4 u M + K u) of q <= 25 / K), so fp32 cannot reorder the two


def _q_sel(sel, bias, support):
    x = sel + (0.0 if bias is None else bias)
    return (LO.softmax(x) * support).mean(-1)


def _c51_batch(B, A, K, dtype, seed, bias_on, pad):
    """Random rows with case rows mixed in (row b % 9): 1 exact selector tie between actions lo < hi (duplicated rows, equal
    bias slices), 2 targets on atoms (gamma = 1, r = m * delta), 3 r = +-30 (clipped at vmax / vmin), 4 gamma = 0, 5 term = 1,
    6 logits near +-90 (exp overflows fp32 without the max subtraction), 7 per-sample gamma^n, 8 all actions tie (no bias)."""
    rng = np.random.default_rng(seed)
    AK = A * K
    rs = AK + (13 if pad else 0)
    support = np.linspace(-VMAX, VMAX, K).astype(np.float32).astype(float)
    delta = 2 * VMAX / (K - 1)
    lo, hi = (0, 1) if A == 2 else (1, A - 1)
    l1 = rng.standard_normal((B, A, K)) * 1.5
    ls = rng.standard_normal((B, A, K)) * 1.5
    lt = rng.standard_normal((B, A, K)) * 1.5
    rew = rng.integers(-2, 3, B) + rng.uniform(-0.5, 0.5, B) * (rng.random(B) < 0.5)
    disc = np.full(B, 0.99)
    term = np.zeros(B)
    ties = np.zeros(B, bool)
    up = np.linspace(0.0, 4.0, K)
    for b in range(B):
        case = b % 9
        if case == 1 and A >= 2:
            ls[b] = rng.standard_normal((A, K)) * 0.3 - up                # every other action leans to -vmax
            ls[b, lo] = ls[b, hi] = rng.standard_normal(K) * 0.3 + up
            lt[b, hi] = lt[b, lo][::-1] + up                      # another target: the wrong choice changes td
            ties[b] = True
        elif case == 2:
            disc[b], rew[b] = 1.0, delta * rng.integers(-3, 4)
        elif case == 3:
            rew[b] = 30.0 if (b // 9) % 2 == 0 else -30.0
        elif case == 4:
            disc[b] = 0.0
        elif case == 5:
            term[b] = 1.0
        elif case == 6:
            for x in (l1, ls, lt):
                x[b] = rng.choice([-1.0, 1.0], (A, K)) * 90.0 + rng.standard_normal((A, K))
        elif case == 7:
            disc[b] = 0.99 ** rng.integers(1, 6)
            rew[b] = rng.uniform(-3, 3)
        elif case == 8 and bias_on is None:
            ls[b, :] = rng.standard_normal(K)
            ties[b] = A >= 2
    on = np.full((2 * B, rs), np.nan)
    tg = np.full((B, rs), np.nan)
    on[:B, :AK], on[B:, :AK], tg[:, :AK] = l1.reshape(B, AK), ls.reshape(B, AK), lt.reshape(B, AK)
    on_d, on_v = _dev(on, dtype)
    tg_d, tg_v = _dev(tg, dtype)
    # selector near-ties outside the deliberate ones: tilt the best action towards +vmax and its close competitors towards -vmax
    # (one side moves even where a saturated softmax pins the other) until the gap is clear
    bias_v = None if bias_on is None else bias_on.reshape(A, K)
    for _ in range(20):
        ls_v = on_v[B:, :AK].reshape(B, A, K)
        q = np.stack([_q_sel(ls_v[b], bias_v, support) for b in range(B)])
        srt = np.sort(q, axis=1)
        bad = [b for b in range(B) if A > 1 and not ties[b] and srt[b, -1] - srt[b, -2] < GAP]
        if not bad:
            break
        for b in bad:
            best = int(np.argmax(q[b]))
            for a in range(A):
                if a == best or q[b, a] > q[b, best] - GAP:
                    on[B + b, a * K:(a + 1) * K] += (30.0 if a == best else -30.0) * np.linspace(0.0, 1.0, K)
        on_d, on_v = _dev(on, dtype)
    else:
        raise AssertionError("could not separate the selector's q values")
    for b in np.nonzero(ties)[0]:                                # the deliberate ties are exact, and they are the maximum
        qb = q[b]
        assert qb[lo] == qb[hi] and qb.max() == qb[lo], (b, qb)
    act = rng.integers(0, A, B)
    prios = 10.0 ** rng.uniform(-8, 0, B)
    return dict(rs=rs, support=support, on_d=on_d, tg_d=tg_d, l1=on_v[:B, :AK].reshape(B, A, K),
                ls=on_v[B:, :AK].reshape(B, A, K), lt=tg_v[:, :AK].reshape(B, A, K), act=act,
                rew=rew.astype(np.float32).astype(float), disc=disc.astype(np.float32).astype(float), term=term, prios=prios,
                ties=ties, delta=delta)


def _c51_tolerances(d, bias_on, bias_t, td, w, dl):
    """Per-sample bounds on td, w and dl from the oracle's values (first order in u, doubled):
      M      largest |logit| (bias included) the sample touches; dx = u M: the fp32 rounding of logit + bias
      rho_e  relative error of __expf(x), x = l - max in [-2M, 0]: 2 dx + (x * log2 e rounded: u |x|) + 2 ulp of v_exp
             <= 2 dx + 6 u M + 4 u;  rho_s = rho_e + K u (sum of K terms); rho_p = rho_e + rho_s + u (the division)
      e_lp   |error| of log_softmax = x - log(s): 2 dx + 2 u M + rho_s + 4 u (1 + log K) + u |logp|
      eta    |error| of a triangular weight 1 - |tz_j - z_i| / delta: tz = r + g z rounded twice (2 u (|r| + vmax)), the fp32
             support off its uniform grid (2 u vmax), the rounded 1/delta (4 u) -> (2 u (|r| + 2 vmax)) / delta + 5 u
      tau    L1 error of the projected target: every source atom feeds <= 3 target atoms: rho_p + 3 eta + K u
      td     tau max|logp| + e_lp (1 + tau) + 6 u |td| (64-lane tree sums)
      w      two powf (2 ulp each) and a division: 8 u w
      dl_k   (w / B) (p_k (rho_p + tau + 6 u) + tau + 6 u) + 10 u |dl_k|"""
    B, A, K = d["l1"].shape
    bo = 0.0 if bias_on is None else bias_on.reshape(A, K)
    bt = 0.0 if bias_t is None else bias_t.reshape(A, K)
    M = np.array([max(np.abs(d["l1"][b] + bo).max(), np.abs(d["ls"][b] + bo).max(), np.abs(d["lt"][b] + bt).max())
                  for b in range(B)])
    dx = U * M
    rho_e = 2 * dx + 6 * U * M + 4 * U
    rho_s = rho_e + K * U
    rho_p = rho_e + rho_s + U
    l1b = np.stack([(d["l1"][b] + bo)[d["act"][b]] for b in range(B)])
    logp = np.stack([LO.log_softmax(r) for r in l1b])
    e_lp = 2 * dx + 2 * U * M + rho_s + 4 * U * (1 + np.log(K)) + U * np.abs(logp).max(1)
    eta = 2 * U * (np.abs(d["rew"]) + 2 * VMAX) / d["delta"] + 5 * U
    tau = rho_p + 3 * eta + K * U
    tol_td = 2 * (tau * np.abs(logp).max(1) + e_lp * (1 + tau) + 6 * U * np.abs(td))
    tol_w = 2 * 8 * U * w
    p = np.exp(logp)
    tol_dl = 2 * ((w / B)[:, None] * (p * (rho_p + tau + 6 * U)[:, None] + (tau + 6 * U)[:, None]) + 10 * U * np.abs(dl))
    return tol_td, tol_w, tol_dl


@pytest.mark.parametrize("A,K", SHAPES)
@pytest.mark.parametrize("B", [1, 63, 65, 256, 300])
@pytest.mark.parametrize("dtype", DTYPES)
def test_c51_loss_kernels_equal_f64_oracle(dtype, B, A, K):
    """hb_c51_loss_sparse (B <= 256 here) and hb_c51_loss_grad (every B) on the same crafted batch: td, IS weights, dLoss/dlogits
    of the taken action (compact: columns >= K exactly zero; dense: every other column, padding included, exactly zero) and the
    update counter advanced by exactly one per launch. A selector tie resolved to the higher action changes the sample's
    target (its target row differs), so the td comparison also pins the lowest-index rule."""
    import torch

    K_ = _K()
    L, s = K_.lib(), K_.current_stream()
    iB = [1, 63, 65, 256, 300].index(B)
    for ci in (iB % 4, (iB + 2) % 4):
        beta, has_bias, mask, pad = CONFIGS[ci]
        seed = 1000 * A + 10 * K + B + ci
        rng = np.random.default_rng(seed + 7)
        bias_on = bias_t = None
        bo_d = bt_d = None
        if has_bias:
            bo = rng.standard_normal(A * K) * 0.5
            lo, hi = (0, 1) if A == 2 else (1, A - 1)
            if A >= 2:
                bo[hi * K:(hi + 1) * K] = bo[lo * K:(lo + 1) * K]   # a tie stays a tie with the bias added
            bo_d, bias_on = _dev(bo, dtype)
            bt_d, bias_t = _dev(rng.standard_normal(A * K) * 0.5, dtype)
        d = _c51_batch(B, A, K, dtype, seed, bias_on, pad)
        td, w, dl, sel = LO.c51_td_and_grad(d["l1"], d["ls"], d["lt"], d["act"], d["rew"], d["term"], d["disc"], mask,
                                            d["support"], d["prios"], beta, bias_on, bias_t)
        if A >= 2:
            lo = 0 if A == 2 else 1
            assert (sel[d["ties"]] == np.where(np.arange(B)[d["ties"]] % 9 == 8, 0, lo)).all()
        tol_td, tol_w, tol_dl = _c51_tolerances(d, bias_on, bias_t, td, w, dl)
        f32 = lambda x: torch.as_tensor(np.asarray(x, np.float32)).cuda()
        act_d = torch.as_tensor(d["act"].astype(np.int32)).cuda()
        rew_d, term_d, disc_d, sup_d = f32(d["rew"]), f32(d["term"]), f32(d["disc"]), f32(d["support"])
        pr_d = torch.as_tensor(d["prios"]).cuda()
        beta_d = f32([beta])
        args = (K_.dptr(d["on_d"]), K_.dptr(d["tg_d"]), CODE[dtype], K_.dptr(act_d), K_.dptr(rew_d), K_.dptr(term_d),
                K_.dptr(pr_d), K_.dptr(beta_d), K_.dptr(disc_d), mask, K_.dptr(sup_d), B, A, K, d["rs"])
        rows = np.arange(B)
        # ---- sparse (batch <= 256: the learner's batches; the kernel itself has no limit, the test keeps to the tested sizes)
        if B <= 256:
            td_d, w_d = torch.full((B,), float("nan"), device="cuda"), torch.full((B,), float("nan"), device="cuda")
            dl_d = torch.full((B, 64), float("nan"), device="cuda")
            cnt = f32([5.0])
            K_.check(L.hb_c51_loss_sparse(*args, K_.dptr(td_d), K_.dptr(w_d), K_.dptr(dl_d), K_.dptr(cnt), K_.dptr(bo_d),
                                          K_.dptr(bt_d), s))
            torch.cuda.synchronize()
            _within(_host(td_d), td, tol_td)
            _within(_host(w_d), w, tol_w)
            got = _host(dl_d)
            _within(got[:, :K], dl, tol_dl)
            assert (got[:, K:] == 0).all()
            assert float(cnt) == 6.0
        # ---- dense cross-check kernel: dlogits in the input dtype over the whole padded row
        td_d, w_d = torch.full((B,), float("nan"), device="cuda"), torch.full((B,), float("nan"), device="cuda")
        dlog = torch.full((B, d["rs"]), float("nan"), device="cuda", dtype=_tdt(dtype))
        cnt = f32([5.0])
        K_.check(L.hb_c51_loss_grad(*args, K_.dptr(td_d), K_.dptr(w_d), K_.dptr(dlog), K_.dptr(cnt), K_.dptr(bo_d),
                                    K_.dptr(bt_d), s))
        torch.cuda.synchronize()
        _within(_host(td_d), td, tol_td)
        _within(_host(w_d), w, tol_w)
        got = _host(dlog)
        cols = d["act"][:, None] * K + np.arange(K)[None]
        _within(got[rows[:, None], cols], dl, tol_dl, dtype)
        rest = np.ones_like(got, bool)
        rest[rows[:, None], cols] = False
        assert (got[rest] == 0).all()
        assert float(cnt) == 6.0


# ---- scalar double-Q loss: hb_dqn_loss_sparse ------------------------------------------------------------------------------
@pytest.mark.parametrize("cs", [1, 2])
@pytest.mark.parametrize("B", [1, 64, 65, 256])
@pytest.mark.parametrize("dtype", DTYPES)
def test_dqn_loss_kernel_equals_f64_oracle(dtype, B, cs):
    """td, IS weights and dl[b, 0] = -w td / B against dqn_td_and_grad; columns 1..63 of dl exactly zero; unused q columns
    (the second atom of cs = 2, the row padding) hold NaN, so reading one fails. Case rows: exact selector ties between
    actions 2 and A - 1 (equal bias there; the lowest must win: their target values differ by >= 1), terminal rows.
    Bounds (first order, doubled): q + bias, disc * q_t, r + that and the difference each round once:
    |td err| <= 4 u (|r| + |disc q_t| + |q_tm1| + |td|); w: two powf and a division, 8 u w; dl: |w / B| |td err| + 8 u |dl|."""
    import torch

    K_ = _K()
    L, s = K_.lib(), K_.current_stream()
    A = 11 if cs == 1 else 20
    rs = (A - 1) * cs + 1 + 5
    for ci, (beta, has_bias) in enumerate([(-0.5, True), (0.4, False)] if B % 2 == 0 else [(1.0, False), (0.0, True)]):
        rng = np.random.default_rng(B * 10 + cs + ci)
        q1, qs, qt = (rng.standard_normal((B, A)) * 2 for _ in range(3))
        term = (rng.random(B) < 0.25).astype(float)
        ties = np.arange(B) % 5 == 1
        bo = bt = None
        if has_bias:
            bo, bt = rng.standard_normal(A), rng.standard_normal(A)
            bo[A - 1] = bo[2]
        qs[ties, 2] = qs[ties, A - 1] = 20.0
        qt[ties, 2], qt[ties, A - 1] = 1.0, -1.0
        # outside the ties, the best selector value stands GAP clear of the second (fp32 rounding cannot reorder them)
        for b in np.nonzero(~ties)[0]:
            v = qs[b] + (0 if bo is None else bo)
            o = np.argsort(v)
            if v[o[-1]] - v[o[-2]] < 0.05:
                qs[b, o[-1]] += 0.1
        on = np.full((2 * B, rs), np.nan)
        tg = np.full((B, rs), np.nan)
        on[:B, 0:A * cs:cs], on[B:, 0:A * cs:cs], tg[:, 0:A * cs:cs] = q1, qs, qt
        on_d, on_v = _dev(on, dtype)
        tg_d, tg_v = _dev(tg, dtype)
        bo_d = bt_d = None
        bo_v = bt_v = None
        if has_bias:
            bb = np.full(rs, np.nan)
            bb[0:A * cs:cs] = bo
            bo_d, bo_full = _dev(bb, dtype)
            bb[0:A * cs:cs] = bt
            bt_d, bt_full = _dev(bb, dtype)
            bo_v, bt_v = bo_full[0:A * cs:cs], bt_full[0:A * cs:cs]
        q1v, qsv, qtv = on_v[:B, 0:A * cs:cs], on_v[B:, 0:A * cs:cs], tg_v[:, 0:A * cs:cs]
        act = rng.integers(0, A, B)
        rew = rng.integers(-2, 3, B).astype(float)
        disc = (0.99 ** rng.integers(1, 4, B)).astype(np.float32).astype(float)
        prios = 10.0 ** rng.uniform(-8, 0, B)
        td, w, dq, sel = LO.dqn_td_and_grad(q1v, qsv, qtv, act, rew, term, disc, prios, beta, bo_v, bt_v)
        assert (sel[ties] == 2).all()
        f32 = lambda x: torch.as_tensor(np.asarray(x, np.float32)).cuda()
        td_d, w_d = torch.full((B,), float("nan"), device="cuda"), torch.full((B,), float("nan"), device="cuda")
        dl_d = torch.full((B, 64), float("nan"), device="cuda")
        act_d = torch.as_tensor(act.astype(np.int32)).cuda()
        rew_d, term_d, disc_d, beta_d = f32(rew), f32(term), f32(disc), f32([beta])
        pr_d = torch.as_tensor(prios).cuda()
        K_.check(L.hb_dqn_loss_sparse(K_.dptr(on_d), K_.dptr(tg_d), CODE[dtype], K_.dptr(act_d), K_.dptr(rew_d), K_.dptr(term_d),
                                      K_.dptr(pr_d), K_.dptr(beta_d), K_.dptr(disc_d), B, A, cs, rs, K_.dptr(td_d), K_.dptr(w_d),
                                      K_.dptr(dl_d), K_.dptr(bo_d), K_.dptr(bt_d), s))
        torch.cuda.synchronize()
        r = np.arange(B)
        qbo = q1v + (0 if bo_v is None else bo_v)
        qtb = np.where(term[:, None] != 0, 0.0, qtv + (0 if bt_v is None else bt_v))
        tol_td = 2 * 4 * U * (np.abs(rew) + np.abs(disc * qtb[r, sel]) + np.abs(qbo[r, act]) + np.abs(td))
        _within(_host(td_d), td, tol_td)
        _within(_host(w_d), w, 2 * 8 * U * w)
        got = _host(dl_d)
        _within(got[:, 0], dq, 2 * (np.abs(w / B) * tol_td + 8 * U * np.abs(dq)))
        assert (got[:, 1:] == 0).all()


# ---- backward through the output layer: hb_c51_backward -------------------------------------------------------------------
def _bwd_lds(B, H, A, dtype):
    """launch_backward's LDS request (csrc/learner2.hip), to know which shapes the wrapper refuses (> 150 KB)."""
    row = A * (72 if dtype != "float32" else 68) * (2 if dtype != "float32" else 4)
    jt = 8
    while jt > 1 and jt * row + 16 * jt * 4 > 64 * 1024:
        jt >>= 1
    list_bytes = ((B + 3) & ~3) * 4
    return max(jt * row + 16 * jt * 4, list_bytes, list_bytes + B * 64 * 4 + (8 * 64 * 20 + 8 * 64) * 4)


@pytest.mark.parametrize("A,K", SHAPES)
@pytest.mark.parametrize("hidden", [32, 40, 100, 512])
@pytest.mark.parametrize("dtype", DTYPES)
def test_c51_backward_equals_f64_oracle(dtype, hidden, A, K):
    """dH, db1, dW2, db2 against c51_backward for B in {1, 30, 256}: H with exact zeros (relu'(0) = 0), an action nobody took
    (its dW2 / db2 slices exactly zero), at B = 256 with hidden >= 100 every sample on one action; padded strides (h_ld odd
    for B = 30: the scalar load path) with NaN in every padding column the kernel must not read; columns >= A K of dW2 left
    untouched; two runs bit-identical.
    Bounds (first order, doubled), S = sum of |terms| of the exact sum:
      dH   K fp32 fmas in 4 parts + 2 adds: (K + 2) u S, then rounded to the dtype (interval)
      dW2  <= B fmas in 8 ranges + 8 adds: (B + 8) u S, rounded to the dtype; db2 the same on sum |dl|
      db1  the column sum of dH AS STORED: each term off the exact dH by e_b + half an ulp of the dtype, plus (B + 20) u of
           the fp32 sum (per-lane, 64-lane tree, 16 wavefronts)"""
    import torch

    K_ = _K()
    L, s = K_.lib(), K_.current_stream()
    AK = A * K
    runs = 0
    for B in (1, 30, 256):
        assert _bwd_lds(B, hidden, A, dtype) <= 150 * 1024      # no shape of the learner's range (B <= 256) is refused
        rng = np.random.default_rng(hidden * 1000 + AK + B)
        h_ld = hidden + (3 if B == 30 else 0)
        w2_ld, dw2_ld = AK + 5, AK + 7
        idle = A // 2 if A >= 2 else -1
        act = rng.integers(0, A, B)
        if A >= 2:
            act[act == idle] = (idle + 1) % A
        if B == 256 and hidden >= 100:
            act[:] = (idle + 1) % A if A >= 2 else 0
        dl = np.zeros((B, 64))
        dl[:, :K] = rng.standard_normal((B, K)) * 1e-3
        hm = np.full((B, h_ld), np.nan)
        hm[:, :hidden] = np.maximum(rng.standard_normal((B, hidden)), 0.0)   # about half the units exactly zero
        w2 = np.full((hidden, w2_ld), np.nan)
        w2[:, :AK] = rng.standard_normal((hidden, AK)) * 0.05
        dl_d = torch.as_tensor(dl.astype(np.float32)).cuda()
        dl_v = _host(dl_d)[:, :K]
        h_d, h_v = _dev(hm, dtype)
        w2_d, w2_v = _dev(w2, dtype)
        h_v, w2_v = h_v[:, :hidden], w2_v[:, :AK]
        act_d = torch.as_tensor(act.astype(np.int32)).cuda()
        dh, db1, dw2, db2 = LO.c51_backward(dl_v, act, h_v, w2_v, K)
        outs = []
        for _ in range(2):
            dh_d = torch.full((B, hidden), float("nan"), device="cuda", dtype=_tdt(dtype))
            db1_d = torch.full((hidden,), float("nan"), device="cuda")
            dw2_d = torch.full((hidden, dw2_ld), float("nan"), device="cuda", dtype=_tdt(dtype))
            db2_d = torch.full((AK,), float("nan"), device="cuda")
            K_.check(L.hb_c51_backward(K_.dptr(dl_d), K_.dptr(act_d), K_.dptr(h_d), h_ld, K_.dptr(w2_d), w2_ld, CODE[dtype], B, hidden,
                                       A, K, K_.dptr(dh_d), K_.dptr(db1_d), K_.dptr(dw2_d), dw2_ld, K_.dptr(db2_d), s))
            outs.append((dh_d, db1_d, dw2_d, db2_d))
        torch.cuda.synchronize()
        runs += 1
        for x, y in zip(*outs):
            assert torch.equal(x.view(torch.uint8) if x.dtype != torch.float32 else x.view(torch.int32),
                               y.view(torch.uint8) if y.dtype != torch.float32 else y.view(torch.int32))
        dh_g, db1_g, dw2_g, db2_g = (_host(t) for t in outs[0])
        dense = np.zeros((B, AK))
        for i in range(B):
            dense[i, act[i] * K:(act[i] + 1) * K] = dl_v[i]
        s_dh = np.abs(dense) @ np.abs(w2_v).T
        e_dh = 2 * (K + 2) * U * s_dh
        _within(dh_g, dh, e_dh, dtype)
        assert (dh_g[h_v == 0] == 0).all()
        term_err = e_dh + (_half_ulp(np.abs(dh) + e_dh, dtype) if dtype != "float32" else 0.0)
        e_db1 = (term_err * (h_v > 0)).sum(0) + 2 * (B + 20) * U * (np.abs(dh) + term_err).sum(0)
        _within(db1_g, db1, e_db1)
        _within(dw2_g[:, :AK], dw2, 2 * (B + 8) * U * (np.abs(h_v).T @ np.abs(dense)), dtype)
        assert np.isnan(dw2_g[:, AK:]).all()
        _within(db2_g, db2, 2 * (B + 8) * U * np.abs(dense).sum(0))
        if idle >= 0:
            assert (dw2_g[:, idle * K:(idle + 1) * K] == 0).all() and (db2_g[idle * K:(idle + 1) * K] == 0).all()
    assert runs == 3


def test_c51_backward_refuses_what_it_cannot_hold():
    """The wrapper's limits, checked before any launch: batch > 256 (a thread keeps its share of one action's samples in 32
    registers), more than 64 actions or atoms. Inside them its LDS request never exceeds 150 KB (largest: B = 256)."""
    import torch

    K_ = _K()
    L, s = K_.lib(), K_.current_stream()
    assert max(_bwd_lds(256, 512, a, dt) for a in (1, 20, 64) for dt in DTYPES) <= 150 * 1024
    buf = torch.zeros(1 << 16, device="cuda")
    p = K_.dptr(buf)
    for B, A, Kk in ((257, 20, 51), (16, 65, 51), (16, 20, 65), (16, 20, 1)):
        assert L.hb_c51_backward(p, p, p, 64, p, A * Kk, 0, B, 64, A, Kk, p, p, p, A * Kk, p, s) == HB_ERR_INVALID
        assert L.hb_last_error()


# ---- Adam on the NoisyLinear triple: hb_noisy_adam, hb_noisy_adam_multi, hb_noisy_adam_multi_pack ---------------------------
B1, B2, LR, EPS = (float(np.float32(x)) for x in (0.9, 0.999, 1e-3, 3.125e-5))


def _adam_bounds(g, nz, mom, out, tt, shared):
    """Per-element bounds of one fp32 Adam step (adam1 in csrc/learner.hip: every operation rounded once), first order, doubled.
      m' = fma(b1, m, (1-b1) g)          (1 - b1 exact, Sterbenz): u |(1-b1) g| + u |m'|      (sigma: g * noise rounded: + (1-b1) u |g nz|)
      v' = fma(b2, v, ((1-b2) g) g)      2 u (1-b2) g^2 + u |v'|                             (sigma: + 2 u (1-b2) (g nz)^2)
      bc1 = 1 - powf(b1, t)              relative 2 u b1^t / bc1 + u   (powf within 2 ulp)
      bc2s = sqrtf(1 - powf(b2, t))      relative (2 u b2^t / bc2 + u) / 2 + u
      step = (lr / bc1) m' / (sqrt(v') / bc2s + eps)  with the errors of m' and sqrt(v') carried through, 5 roundings
      p' = p - step                      err(step) + u |p'|
    Returns (err of the three parameters, err of the six moments, err of the merged weight before its dtype rounding)."""
    m_w, v_w, m_mu, v_mu, m_sg, v_sg = mom
    nm = out[3]
    bc1, bc2 = 1 - B1 ** tt, 1 - B2 ** tt
    r1 = 2 * U * B1 ** tt / bc1 + U
    r2 = (2 * U * B2 ** tt / bc2 + U) / 2 + U

    def one(gg, extra_g, m1, v1, pnew):
        em = U * np.abs((1 - B1) * gg) + U * np.abs(m1) + (1 - B1) * extra_g
        ev = 2 * U * (1 - B2) * gg * gg + U * np.abs(v1) + 2 * (1 - B2) * np.abs(gg) * extra_g
        sq = np.sqrt(v1)
        esq = sq - np.sqrt(np.maximum(v1 - ev, 0.0)) + U * sq
        den = sq / np.sqrt(bc2) + EPS
        eden = (esq + sq * r2) / np.sqrt(bc2) + 2 * U * den
        num = LR / bc1 * np.abs(m1)
        enum = num * (r1 + 2 * U) + LR / bc1 * em
        step = num / den
        est = step * (eden / den + U) + enum / den
        return 2 * (est + U * np.abs(pnew)), 2 * em, 2 * ev, 2 * est

    ew, emw, evw, stw = one(g, 0.0, nm[0], nm[1], out[0])
    if shared:
        emu, emm, evm = 2 * (stw / 2 + U * np.abs(out[1])), 0 * emw, 0 * evw
    else:
        emu, emm, evm, _ = one(g, 0.0, nm[2], nm[3], out[1])
    gs = g * nz
    esg, ems, evs, _ = one(gs, U * np.abs(gs), nm[4], nm[5], out[2])
    eff = ew + emu + np.abs(nz) * esg + 2 * U * (np.abs(out[0] + out[1]) + np.abs(out[4]) + np.abs(out[2] * nz))
    return (ew, emu, esg), (emw, evw, emm, evm, ems, evs), eff


class _AdamTensor:
    """One NoisyLinear tensor's device arrays (fp32 master copies, moments, noise, gradient in its dtype with padded rows, the
    merged weight in the GEMM dtype with padded rows whose padding holds a sentinel) and its float64 host values."""

    def __init__(self, rng, rows, cols, grad_dtype, eff_dtype, shared, grad_pad=4, eff_pad=4):
        import torch

        self.rows, self.cols, self.shared = rows, cols, shared
        self.grad_dtype, self.eff_dtype = grad_dtype, eff_dtype
        mk = lambda sc: torch.as_tensor((rng.standard_normal((rows, cols)) * sc).astype(np.float32)).cuda()
        self.p = [mk(0.1) for _ in range(3)]
        self.noise = mk(1.0)
        mom = [mk(1e-3), mk(1e-3).abs() * 1e-3, mk(1e-3), mk(1e-3).abs() * 1e-3, mk(1e-3), mk(1e-3).abs() * 1e-3]
        if shared:
            mom[2], mom[3] = mom[0], mom[1]
        self.mom = mom
        self.gl = cols + grad_pad
        gh = np.full((rows, self.gl), np.nan)
        gh[:, :cols] = rng.standard_normal((rows, cols)) * 1e-2
        gh[0, 0] = 0.0                                           # a zero gradient (v may stay tiny)
        self.grad, gv = _dev(gh, grad_dtype)
        self.g = gv[:, :cols]
        self.eff_ld = cols + eff_pad
        self.eff = torch.full((rows, self.eff_ld), 7.0, device="cuda", dtype=_tdt(eff_dtype))
        self.before = [_host(t) for t in self.p], _host(self.noise), [_host(t) for t in mom]

    def table_entry(self, d):
        d.w, d.w_mu, d.w_sigma = (t.data_ptr() for t in self.p)
        d.noise, d.grad, d.grad_dtype, d.grad_ld = self.noise.data_ptr(), self.grad.data_ptr(), CODE[self.grad_dtype], self.gl
        d.m_w, d.v_w, d.m_mu, d.v_mu, d.m_sigma, d.v_sigma = (t.data_ptr() for t in self.mom)
        d.eff, d.n, d.cols, d.eff_ld = self.eff.data_ptr(), self.rows * self.cols, self.cols, self.eff_ld

    def check(self, t_done, offset):
        (w, mu, sg), nz, mom = self.before
        tt = t_done + offset
        out = LO.noisy_adam(w, mu, sg, nz, self.g, mom, t_done, LR, B1, B2, EPS, offset, self.shared)
        ep, em, eeff = _adam_bounds(self.g, nz, mom, out, tt, self.shared)
        for t, ref, e in zip(self.p, out[:3], ep):
            _within(_host(t), ref, e)
        for i, (t, ref, e) in enumerate(zip(self.mom, out[3], em)):
            if self.shared and i in (2, 3):
                continue                                         # the same arrays as m_w / v_w
            _within(_host(t), ref, e)
        eff = _host(self.eff)
        _within(eff[:, :self.cols], out[4], eeff, self.eff_dtype)
        assert (eff[:, self.cols:] == 7.0).all()                 # padding columns untouched
        return eff


TS = [(1, 1.0), (2, 1.0), (1_000_000, 1.0), (1, 0.0), (2, 0.0), (1_000_000, 0.0)]   # (this step's number t, step_offset)


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("eff_dtype", DTYPES)
def test_noisy_adam_equals_f64_oracle(eff_dtype, shared):
    """hb_noisy_adam (fp32 gradient, this step = *step + 1) at t = 1, 2, 10^6; both shapes of the scalar kernel (cols % 4 != 0
    and a 16-byte-friendly one), padded eff rows."""
    import torch

    K_ = _K()
    L, s = K_.lib(), K_.current_stream()
    for ti, t in enumerate((1, 2, 1_000_000)):
        for rows, cols in ((7, 5), (40, 68)):
            rng = np.random.default_rng(100 * ti + rows + int(shared))
            T = _AdamTensor(rng, rows, cols, "float32", eff_dtype, shared, grad_pad=0)
            step = torch.tensor([float(t - 1)], device="cuda")
            p, m = T.p, T.mom
            K_.check(L.hb_noisy_adam(K_.dptr(p[0]), K_.dptr(p[1]), K_.dptr(p[2]), K_.dptr(T.noise), K_.dptr(T.grad), K_.dptr(m[0]),
                                     K_.dptr(m[1]), K_.dptr(m[2]), K_.dptr(m[3]), K_.dptr(m[4]), K_.dptr(m[5]), K_.dptr(step),
                                     K_.dptr(T.eff), CODE[eff_dtype], rows * cols, cols, T.eff_ld, LR, B1, B2, EPS, s))
            torch.cuda.synchronize()
            T.check(t - 1, 1.0)


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("eff_dtype", DTYPES)
@pytest.mark.parametrize("grad_dtype", DTYPES)
def test_noisy_adam_multi_equals_f64_oracle(grad_dtype, eff_dtype, shared):
    """hb_noisy_adam_multi: count 1 (the 4-wide vector kernel), 8 tensors of different shapes all 16-byte friendly (vector
    kernel, 8 tensor slots), 8 tensors one of which has cols % 4 != 0 (the whole launch takes the scalar kernel); every
    (t, step_offset) of TS."""
    import torch

    K_ = _K()
    L, s = K_.lib(), K_.current_stream()
    sets = [[(24, 36)], [(8, 4), (3, 64), (17, 12), (1, 128), (40, 68), (2, 8), (5, 4), (9, 100)],
            [(8, 4), (3, 64), (17, 12), (1, 126), (40, 68), (2, 8), (5, 4), (9, 7)]]
    for si, shapes in enumerate(sets):
        for ti, (t, off) in enumerate(TS):
            if si > 0 and ti % 2:
                continue                                         # (the single-tensor set takes every t; the others half)
            rng = np.random.default_rng(1000 * si + 10 * ti + int(shared))
            ts = [_AdamTensor(rng, r, c, grad_dtype, eff_dtype, shared) for r, c in shapes]
            tab = (K_.HbAdamTensor * len(ts))()
            for i, T in enumerate(ts):
                T.table_entry(tab[i])
            step = torch.tensor([float(t) - off], device="cuda")
            K_.check(L.hb_noisy_adam_multi(tab, len(ts), K_.dptr(step), off, CODE[eff_dtype], LR, B1, B2, EPS, s))
            torch.cuda.synchronize()
            for T in ts:
                T.check(t - off, off)


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("eff_dtype", ["bfloat16", "float16"])
@pytest.mark.parametrize("grad_dtype", DTYPES)
def test_noisy_adam_multi_pack_equals_f64_oracle(grad_dtype, eff_dtype, shared):
    """hb_noisy_adam_multi_pack without fragment copies: a weight tensor of 37 x 136 (a partial 8-row group and a partial
    128-column tile) with its transposed copy (wt[n, k] = eff[k, n]; rows 37..39 of the 8-row group zero, columns from 40 on
    untouched) and a bias tensor (one row) with its fp32 copy (= the rounded merged bias); weights, moments and the merged
    tensors against the oracle at every (t, step_offset) of TS."""
    import torch

    K_ = _K()
    L, s = K_.lib(), K_.current_stream()
    for ti, (t, off) in enumerate(TS):
        rng = np.random.default_rng(50 * ti + int(shared))
        wt_t, bias_t = _AdamTensor(rng, 37, 136, grad_dtype, eff_dtype, shared), _AdamTensor(rng, 1, 68, grad_dtype, eff_dtype, shared)
        tab, packs = (K_.HbAdamTensor * 2)(), (K_.HbAdamPack * 2)()
        wt_t.table_entry(tab[0])
        bias_t.table_entry(tab[1])
        wt_ld = 48
        wt = torch.full((136, wt_ld), 3.0, device="cuda", dtype=_tdt(eff_dtype))
        bf32 = torch.full((68,), float("nan"), device="cuda")
        packs[0].wt, packs[0].wt_ld = wt.data_ptr(), wt_ld
        packs[1].bias_f32 = bf32.data_ptr()
        step = torch.tensor([float(t) - off], device="cuda")
        K_.check(L.hb_noisy_adam_multi_pack(C.cast(tab, C.c_void_p), C.cast(packs, C.c_void_p), 2, K_.dptr(step), off,
                                            CODE[eff_dtype], LR, B1, B2, EPS, s))
        torch.cuda.synchronize()
        eff_w = wt_t.check(t - off, off)
        eff_b = bias_t.check(t - off, off)
        wth = _host(wt)
        assert np.array_equal(wth[:, :37], eff_w[:, :136].T)
        assert (wth[:, 37:40] == 0).all() and (wth[:, 40:] == 3.0).all()
        assert np.array_equal(_host(bf32), eff_b[0, :68])


# ---- priorities: hb_per_update ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["", "two"])
def test_per_update_is_bit_exact(path, monkeypatch):
    """hb_per_update writes per_priority(td, alpha) into the tree, bit for bit (the power in double rounded once to float, as
    the oracle takes it), on every update path: fewer than 96 entries (one workgroup), 96..1024 (per 1024-leaf subtree, the
    power fused or — HB_TREE_UPDATE_PATH=two at creation — in a launch of its own) and more than 1024 (stamp + scatter); the
    tracked max / min priority are those of the batch. td in {0, +-1e-12, +-1, +-1e6} and random magnitudes."""
    import torch

    if path:
        monkeypatch.setenv("HB_TREE_UPDATE_PATH", path)
    K_ = _K()
    L, s = K_.lib(), K_.current_stream()
    special = np.array([0.0, 1e-12, -1e-12, 1.0, -1.0, 1e6, -1e6], np.float32)
    for cap, n in ((64, 24), (4096, 120), (4096, 1100)):
        for alpha in (0.0, 0.6, 1.0):
            rng = np.random.default_rng(cap + n + int(alpha * 10))
            td = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 3, n)).astype(np.float32)
            td[:len(special)] = special
            idx = rng.permutation(cap)[:n].astype(np.int64)
            tree = C.c_void_p()
            K_.check(L.hb_tree_create(cap, C.byref(tree)))
            try:
                td_d, idx_d = torch.as_tensor(td).cuda(), torch.as_tensor(idx).cuda()
                mx = torch.zeros(1, device="cuda")
                mn = torch.full((1,), float("inf"), device="cuda")
                K_.check(L.hb_per_update(tree, K_.dptr(idx_d), K_.dptr(td_d), n, alpha, K_.dptr(mx), K_.dptr(mn), s))
                out = torch.full((n,), float("nan"), device="cuda")
                K_.check(L.hb_tree_get(tree, K_.dptr(idx_d), K_.dptr(out), n, s))
                torch.cuda.synchronize()
                want = LO.per_priority(td, alpha)
                got = out.cpu().numpy()
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (cap, n, alpha,
                                                                                   np.nonzero(got != want)[0][:5])
                assert float(mx) == float(want.max()) and float(mn) == float(want.min())
            finally:
                L.hb_tree_destroy(tree)
