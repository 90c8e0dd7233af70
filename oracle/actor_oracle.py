"""numpy float64 restatement of the actor's forward pass, its action selection and the learner's forward GEMM. TEST
INFRASTRUCTURE ONLY.

Written independently of hanabi_agents/rlax_dqn and hanabi_hip/ops.py, as oracle/learner_oracle.py is.
Sources: hanabi_agents/rlax_dqn/rlax_rainbow.py:113-122 (q = jnp.mean(probs * atoms), the legal-masked arg-max and the
epsilon-greedy draw), noisy_mlp.py:176-185 (the one-hidden-layer network), include/hanabi_hip.h (the selection rule of
hb_policy_select: Philox4x32-10 on counter (draw, game id) and key seed; word 0 decides explore, word 1 picks the candidate).

Error bounds. Every helper below returns a first-order bound on the error of the kernels' fp32 arithmetic (unit roundoff
U = 2^-24) computed per element from the oracle's own values, DOUBLED to cover products of first-order terms. A value the
kernel rounds to a 16-bit type T is pinned as an interval [round_T(ref - e), round_T(ref + e)]: rounding is monotone, so the
kernel's value lies inside, and where both ends round alike the interval is one value (exact)."""
import numpy as np

U = 2.0 ** -24
F16_CLAMP = 65000.0          # the two-kernel actor clamps its fp32 logits into the fp16 range before staging them
_MANT = {"float32": 23, "bfloat16": 7, "float16": 10}
_EMIN = {"float32": -126, "bfloat16": -126, "float16": -14}


# ---- rounding ----------------------------------------------------------------------------------------------------------------
def round_to(x, dtype):
    """x (float64) -> the nearest value of `dtype` (ties to even) as float64. bf16 / fp16 round the float32 value: a kernel's
    16-bit value is always the rounding of an fp32 one, and round_T(f32(.)) is monotone, which is all the intervals need."""
    x32 = np.asarray(x, np.float64).astype(np.float32)
    if dtype == "float32":
        return x32.astype(np.float64)
    if dtype == "float16":
        return x32.astype(np.float16).astype(np.float64)
    if dtype == "bfloat16":
        b = x32.view(np.uint32).astype(np.uint64)
        r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
        out = r.astype(np.uint32).view(np.float32)
        return np.where(np.isnan(x32), x32, out).astype(np.float64)
    raise ValueError(dtype)


def half_ulp(x, dtype):
    """Half a unit in the last place of |x| in `dtype` (subnormals: the fixed spacing of the smallest exponent)."""
    e = np.maximum(np.floor(np.log2(np.maximum(np.abs(np.asarray(x, float)), 2.0 ** -200))), _EMIN[dtype])
    return 2.0 ** (e - _MANT[dtype] - 1)


def relu(x):
    return np.maximum(x, 0.0)


# ---- forward -------------------------------------------------------------------------------------------------------------------
def softmax(x):
    x = np.asarray(x, float)
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def expectation(logits, support):
    """q[..., a] = mean_k softmax_k(logits[..., a, :]) * support[k] (rlax_rainbow.py:117-118: jnp.mean, hence the 1 / K)."""
    support = np.asarray(support, float)
    return (softmax(logits) * support).mean(-1)


def forward(obs, w1, b1, w2, b2, support, n_actions, h_dtype=None):
    """z = b1 + obs @ W1, H = relu(z) (rounded to h_dtype when given: what the kernels feed their second layer),
    logits = b2 + H @ W2 viewed [rows, A, K], p = softmax over K, q = mean_k p * support. Every array float64."""
    obs, w1, b1, w2, b2 = (np.asarray(v, float) for v in (obs, w1, b1, w2, b2))
    k = len(support)
    z = obs @ w1 + b1
    h = relu(z)
    if h_dtype is not None:
        h = round_to(h, h_dtype)
    logits = (h @ w2[:, :n_actions * k] + b2[:n_actions * k]).reshape(obs.shape[0], n_actions, k)
    p = softmax(logits)
    q = (p * np.asarray(support, float)).mean(-1)
    return dict(z=z, h=h, logits=logits, p=p, q=q)


# ---- bounds --------------------------------------------------------------------------------------------------------------------
def dot_err(a_abs, b_abs, c_abs, n_terms):
    """Error of an fp32 accumulation sum_j a_j b_j + c whose products are exact (16-bit x 16-bit operands fit in fp32's 24 bits;
    0 / 1 observations times a 16-bit weight are the weight): any summation order of n terms plus the bias rounds at most
    n_terms times, each time by U of a partial sum no larger than sum |a_j b_j| + |c|. Doubled."""
    return 2.0 * n_terms * U * (np.asarray(a_abs, float) @ np.asarray(b_abs, float) + np.asarray(c_abs, float))


def layer1_err(obs, w1, b1):
    """e_z of z = b1 + obs @ W1: obs entries are small integers (bits, or the int8 rows' 0..127), so each product is exact, and a
    zero entry adds an exact 0: a row's nonzero entries plus the bias are its terms."""
    obs = np.asarray(obs, float)
    return dot_err(np.abs(obs), np.abs(w1), np.abs(b1), (obs != 0).sum(-1, keepdims=True) + 1)


def h_interval(z, e_z, dtype):
    """H = round_T(relu(v)) for an fp32 accumulator |v - z| <= e_z: relu and rounding are monotone, so
    H in [round_T(relu(z - e_z)), round_T(relu(z + e_z))]; equal ends pin H exactly, else H is one of the (two, for a bound far
    below an ulp) values between them."""
    return round_to(relu(z - e_z), dtype), round_to(relu(z + e_z), dtype)


def logit_err(h_lo, h_hi, h_mid, w2, b2):
    """Bound on |l_kernel - (b2 + h_mid @ W2)| when the kernel's H is any value in [h_lo, h_hi] and its logits are fp32
    accumulations of exact products: sum_j |W2_jk| max(h_hi - h_mid, h_mid - h_lo) (exact: which H the kernel holds) plus the
    accumulation error of hidden + 1 terms over the largest H it may hold."""
    dev = np.maximum(h_hi - h_mid, h_mid - h_lo)
    w2a = np.abs(np.asarray(w2, float))
    return dev @ w2a + dot_err(np.maximum(np.abs(h_lo), np.abs(h_hi)), w2a, np.abs(b2), h_mid.shape[-1] + 1)


def stage_f16(logits, e_l):
    """The two-kernel actor's logits staging: its fp32 accumulator v (|v - l| <= e_l) is clamped to +-65 000 and rounded to fp16.
    Clamping and rounding are monotone, so the staged value lies in [round_f16(clamp(l - e_l)), round_f16(clamp(l + e_l))];
    where both ends agree (a logit far beyond the clamp, or one whose interval holds no fp16 rounding edge) it is exact.
    Returns the interval's centre and half width: the logits the kernel's softmax sees, known to within that half width."""
    lo = round_to(np.clip(logits - e_l, -F16_CLAMP, F16_CLAMP), "float16")
    hi = round_to(np.clip(logits + e_l, -F16_CLAMP, F16_CLAMP), "float16")
    return (lo + hi) / 2, (hi - lo) / 2


def q_bound(logits, e_l, support):
    """Bound on |q_kernel - expectation(logits)| for the kernels' fp32 softmax expectation over logits [..., K] known to within
    e_l [..., K] (first order, doubled):
      input   dq/dl_k = p_k (s_k - E) / K with E = sum p_k s_k: sum_k p_k |s_k - E| e_l_k / K
      exp     e_k = exp2(l_k log2e - M log2e) is computed with the product l * log2e and M * log2e rounded (u |l|, u |M|, LOG2E
              itself off by u: u (|l| + |M|)), the argument's sum rounded (u |l - M|) and, in the one-kernel actor's quarter merge,
              exp2(m_i - M) and its product (u |m_i - M| <= u |l - M|, u); in natural-log units that is a relative error of
              u (2 |l| + 2 |M| + 2 |l - M|), plus v_exp_f32 (1 ulp = 2 u) twice and the merge's product and 4-term sums: 16 u.
              A relative error rho_k of e_k moves q by p_k rho_k |s_k - E| / K (the common part cancels in t / s)
      sums    t = sum e_k s_k: the product (u) and K - 1 additions: (K + 1) u sum p_k |s_k| / K;
              s = sum e_k (K - 1) u, v_rcp_f32 (2 u), the products by 1 / s and by 1 / K (2 u) and 1 / K rounded (u):
              (K + 4) u |q|, and 4 u more for the merge's 4-term sums
      flush   atoms 87 below the maximum underflow in exp2: p_k < 2^-125 each, at most K 2^-125 max|s|
    """
    logits = np.asarray(logits, float)
    s = np.asarray(support, float)
    K = s.shape[-1]
    p = softmax(logits)
    E = (p * s).sum(-1, keepdims=True)
    M = logits.max(-1, keepdims=True)
    rho = U * (2 * np.abs(logits) + 2 * np.abs(M) + 2 * np.abs(logits - M) + 16)
    q = E[..., 0] / K
    e = ((p * np.abs(s - E) * (np.asarray(e_l, float) + rho)).sum(-1) + (K + 1) * U * (p * np.abs(s)).sum(-1)) / K
    e = e + (K + 8) * U * np.abs(q) + K * 2.0 ** -125 * np.abs(s).max()
    return 2.0 * e


# ---- Philox4x32-10 and the selection rule ---------------------------------------------------------------------------------------
_M0, _M1, _W0, _W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_LO = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """Random123 Philox4x32-10, vectorised: ctr [..., 4], key [..., 2] (uint32 values) -> [..., 4] uint32."""
    c = [np.asarray(ctr, np.uint64)[..., i] & _LO for i in range(4)]
    k0, k1 = (np.asarray(key, np.uint64)[..., i] & _LO for i in range(2))
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & _LO, p1 & _LO, ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & _LO, p0 & _LO]
        k0, k1 = (k0 + _W0) & _LO, (k1 + _W1) & _LO
    return np.stack(c, -1).astype(np.uint32)


def selection_draws(seed, draw, gids):
    """The two Philox words a game's selection uses: counter (draw lo, draw hi, gid lo, gid hi), key (seed lo, seed hi)."""
    gids = np.asarray(gids, np.uint64)
    n = gids.shape[0]
    lo = lambda v: np.uint64(int(v) & 0xFFFFFFFF)
    hi = lambda v: np.uint64((int(v) >> 32) & 0xFFFFFFFF)
    ctr = np.stack([np.full(n, lo(draw)), np.full(n, hi(draw)), gids & _LO, gids >> np.uint64(32)], -1)
    key = np.stack([np.full(n, lo(seed)), np.full(n, hi(seed))], -1)
    r = philox4x32_10(ctr, key)
    return r[:, 0], r[:, 1]


def select(q, legal, epsilon, seed, draw, first_gid):
    """The action hb_policy_select and every fused form define, per row g with game id first_gid + g (mod 2^64):
    legal-masked maximum of the float32 q row and its tie set; u = (r0 >> 8) / 2^24 (exact in float32); the pool is every legal
    action when u < epsilon (float32), else the tie set; an empty pool falls back to the legal set; the pick is the
    umulhi(r1, |pool|)-th set bit (ascending) of the pool, and 0 when no action is legal."""
    q = np.asarray(q, np.float32)
    legal = np.asarray(legal) != 0
    n, A = q.shape
    gids = (np.arange(n, dtype=np.uint64) + np.uint64(int(first_gid) & 0xFFFFFFFFFFFFFFFF))
    r0, r1 = selection_draws(seed, draw, gids)
    u = (r0 >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    explore = u < np.float32(epsilon)
    out = np.zeros(n, np.int32)
    for g in range(n):
        lg = np.nonzero(legal[g])[0]
        if lg.size == 0:
            continue
        best = q[g, lg].max()
        ties = lg[q[g, lg] == best]
        pool = lg if explore[g] or ties.size == 0 else ties
        out[g] = pool[(int(r1[g]) * pool.size) >> 32]
    return out


# ---- the learner's forward GEMM and its column sums ------------------------------------------------------------------------------
def thin_gemm(x, wt, bias, relu_on):
    """hb_thin_gemm's product for one batch entry: act(x [m, k] @ wt [n, k]^T + bias [n]) in float64, with its fp32
    accumulation bound (k products, exact for 16-bit operands, and the bias: k + 1 roundings). Returns (out, err); ReLU is
    monotone and 1-Lipschitz, so the bound holds after it."""
    x, wt = np.asarray(x, float), np.asarray(wt, float)
    b = np.zeros(wt.shape[0]) if bias is None else np.asarray(bias, float)
    pre = x @ wt.T + b
    err = dot_err(np.abs(x), np.abs(wt).T, np.abs(b), x.shape[1] + 1)
    return (relu(pre) if relu_on else pre), err


def colsum(x):
    """Column sums in float64 and the bound of hb_colsum's fp32 order: 16 partial sums of ceil(rows / 16) rows each, then the
    16 partials: at most ceil(rows / 16) + 16 roundings, each of a partial sum no larger than sum_i |x_ij|. Doubled."""
    x = np.asarray(x, float)
    rows = x.shape[0]
    return x.sum(0), 2.0 * ((rows + 15) // 16 + 16) * U * np.abs(x).sum(0)


def relu_bwd_colsum(dy, act):
    """hb_relu_bwd_colsum: dy masked where act > 0 (threshold_backward: act == +0 and -0 are NOT > 0), and its column sums."""
    masked = np.where(np.asarray(act, float) > 0, np.asarray(dy, float), 0.0)
    s, e = colsum(masked)
    return masked, s, e
