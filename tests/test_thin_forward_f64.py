"""GPU: hb_thin_forward (csrc/learner2.hip, thin_forward_kernel) through the C-ABI against the float64 product of the same 16-bit
operand values (oracle.actor_oracle.thin_gemm: the product and its fp32 accumulation bound, the bound of
test_thin_gemm_equals_f64_product) and against the write contract of oracle/thin_forward_oracle.py.

Every launch writes into an output full of NaN and must satisfy all of:
  * every element the loss and the backward read (`need`) is written and within the bound: fp32 outputs |out - ref| <= e, 16-bit
    outputs inside [round(ref - e), round(ref + e)];
  * every element written lies in `may` (need widened to its 16-column tiles) and is within the bound as well;
  * everything else is still NaN: columns [n, ldo), layer 1's target half on obs_tm1, layer 2's target entry on obs_tm1 and the
    online entry's other actions;
  * the written elements are bit-equal to hb_thin_gemm's on the same operands (the header's promise).
The operands carry NaN beyond k (ldx = k + 8, ldw = k + 16) and, in layer 2, in the target entry's obs_tm1 rows, which nobody may
read: a read of either that feeds a `need` element reaches it as NaN, i.e. as "not written" (in a tile's other columns, which
nobody reads, a NaN is indistinguishable from the fill). Row 0 of x is zero and every fifth bias is -0, so exact
+-0 pre-activations meet the ReLU; that row's outputs are exactly the (rectified) biases.

What each case reaches in thin_forward_kernel (k counts 32-wide steps; the loop takes two per trip, `if (kb < kend)` the odd one):
  tail only k = 32; loop + tail k = 96, 160; loop only k = 64, 512, 704; B < 64 (av[] registers all -1) B = 32;
  group border / partial row tiles: the "border" actions (31, 32, 33 samples) and every "each" vector (groups of one sample);
  the maximum tile count for K: (20, 51) and (48, 51) with action 5 (columns 255 .. 305: five tiles), (5, 33), (3, 17), (30, 7);
  fewer tiles than npair (`t0 > tl`): (64, 64), (2, 16); fewer groups than the launch provides (`act_id < 0`): every case;
  the walking launch (more than 1 024 units): WALKING, asserted from the oracle's formulas.
The case tables (LAYER1_CASES, LAYER2_CASES, WALKING) are in tests/thin_forward_cases.py."""
import ctypes as C

import numpy as np
import pytest

from oracle import actor_oracle as AO
from oracle import thin_forward_oracle as TF
from test_actor_kernels_f64 import _close, _dev, _host, _inside
from thin_forward_cases import BF, HF, LAYER1_CASES, LAYER2_CASES, WALKING  # noqa: F401

pytestmark = pytest.mark.gpu


def _K():
    from hanabi_hip import _capi as K

    return K


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _pad(v, m):
    return (v + m - 1) // m * m


def _flags(dtype, out32, relu):
    return (1 if relu else 0) | (2 if out32 else 0) | (4 if dtype == HF else 0)


def _operands(rng, batch, m, n, k, dtype, bias):
    """x [batch, m, k + 8], wt [batch, n, k + 16] with NaN beyond k, row 0 of x zero; bias [batch, n] with every fifth -0"""
    x = np.full((batch, m, k + 8), np.nan)
    x[:, :, :k] = rng.standard_normal((batch, m, k)) * 0.5
    x[:, 0, :k] = 0.0
    wt = np.full((batch, n, k + 16), np.nan)
    wt[:, :, :k] = rng.standard_normal((batch, n, k)) * (1.0 / np.sqrt(k))
    bb = None
    if bias:
        bb = rng.standard_normal((batch, n)) * 0.3
        bb[:, ::5] = -0.0
    return x, wt, bb


def _check_values(o, ref, err, sel, dtype, out32, what):
    """o, ref, err [.., n] float64; sel: the elements to hold to the bound"""
    if out32:
        _close(o[sel], ref[sel], err[sel], what)
    else:
        _inside(o[sel], AO.round_to(ref - err, dtype)[sel], AO.round_to(ref + err, dtype)[sel], what)


def _check_contract(out, n, need, may, ref, err, dtype, out32, what):
    """out: the device output [.., rows, ldo] that was NaN before the launch; need / may / ref / err [.., rows, n]. Returns the
    written mask [.., rows, ldo] (device) for the bit comparison and the output's first n columns in float64."""
    import torch

    wrote_d = ~torch.isnan(out)
    wrote = wrote_d.cpu().numpy()
    assert not wrote[..., n:].any(), f"{what}: columns beyond n written"
    wrote = wrote[..., :n]
    miss = need & ~wrote
    assert not miss.any(), f"{what}: {int(miss.sum())} needed elements not written (or NaN); first at {tuple(np.argwhere(miss)[0])}"
    extra = wrote & ~may
    assert not extra.any(), f"{what}: {int(extra.sum())} elements written outside the tiles; first at {tuple(np.argwhere(extra)[0])}"
    o = _host(out)[..., :n]
    _check_values(o, ref, err, need, dtype, out32, what + " (need)")
    _check_values(o, ref, err, wrote, dtype, out32, what + " (written)")
    return wrote_d, o


@pytest.mark.parametrize("B,n,k,dtype,out32,bias", LAYER1_CASES)
def test_layer1_equals_f64_product_and_writes_only_what_is_read(B, n, k, dtype, out32, bias):
    """bias + ReLU over [online | target] columns: rows [B, 2B) in full, rows [0, B) the online half [0, n / 2) only."""
    import torch

    K = _K()
    L, s = K.lib(), K.current_stream()
    rng = np.random.default_rng(B + n + k)
    m, ldx, ldw, ldo = 2 * B, k + 8, k + 16, n + 4
    x, wt, bb = _operands(rng, 1, m, n, k, dtype, bias)
    x_d, x_v = _dev(x[0], dtype)
    w_d, w_v = _dev(wt[0], dtype)
    b_d, b_v = _dev(bb[0], dtype) if bias else (None, None)
    odt = torch.float32 if out32 else getattr(torch, dtype)
    flags = _flags(dtype, out32, relu=True)
    out = torch.full((m, ldo), float("nan"), dtype=odt, device="cuda")
    K.check(L.hb_thin_forward(1, _ptr(x_d), _ptr(w_d), _ptr(b_d), _ptr(out), None, B, n, k, ldx, ldw, ldo, 0, 0, 0, 0, 0, flags, s))
    gemm = torch.full((m, ldo), float("nan"), dtype=odt, device="cuda")
    K.check(L.hb_thin_gemm(_ptr(x_d), _ptr(w_d), _ptr(b_d), _ptr(gemm), m, n, k, ldx, ldw, ldo, 1, 0, 0, 0, flags, s))
    torch.cuda.synchronize()
    need, may = TF.masks(1, B, n)
    ref, err = AO.thin_gemm(x_v[:, :k], w_v[:, :k], b_v, True)
    what = f"layer 1 {dtype} B={B} n={n} k={k}"
    assert np.array_equal(need, may)                       # layer 1's regions are whole tiles
    wrote, o = _check_contract(out, n, need, may, ref, err, dtype, out32, what)
    assert torch.equal(out[wrote], gemm[wrote]), f"{what}: not bit-equal to hb_thin_gemm"
    np.testing.assert_array_equal(o[0, :n // 2], np.maximum(b_v[:n // 2], 0) if bias else np.zeros(n // 2))


def _action_vectors(B, A, rng):
    """name -> int64 [B] inside [0, A)"""
    acts = {"first": np.zeros(B, np.int64), "last": np.full(B, A - 1, np.int64)}
    each = np.zeros(B, np.int64)
    n = min(A, B)
    each[rng.permutation(B)[:n]] = np.arange(n)          # one sample per action, the remainder on action 0
    acts["each"] = each
    acts["uniform"] = rng.integers(0, A, B)
    if A >= 4 and B >= 31 + 32 + 33 + 1:
        # exactly 31, 32 and 33 samples on three actions, the rest on a fourth, spread over the batch: a group with one row
        # short of full, a full one, and a full one followed by a group of a single sample
        pool = rng.permutation(A)
        big = 5 if A > 5 else pool[0]                     # (K = 51: action 5 starts at column 255 and needs all five tiles)
        rest = [a for a in pool if a != big][:3]
        ids = [rest[0], rest[1], big, rest[2]]
        v = np.full(B, ids[3], np.int64)
        v[:31], v[31:63], v[63:96] = ids[0], ids[1], ids[2]
        v = rng.permutation(v)
        for a, c in zip(ids[:3], (31, 32, 33)):
            assert (v == a).sum() == c
        where33 = np.nonzero(v == ids[2])[0] // 64        # which of the four 64-sample registers of a lane holds each
        assert len(set(where33)) == (B + 63) // 64, "the 33-sample action must sit in every 64-sample part of the batch"
        acts["border"] = v
    return acts


@pytest.mark.parametrize("A,K,k,B,dtype,n_round,out32,bias", LAYER2_CASES)
def test_layer2_equals_f64_product_and_writes_only_what_is_read(A, K, k, B, dtype, n_round, out32, bias):
    """{online, target} entries: rows [B, 2B) of both in full; of the online entry on rows [0, B) the tiles of the action taken;
    the target entry on rows [0, B) never. Five action vectors per case on the same operands and the same reference."""
    import torch

    Kc = _K()
    L, s = Kc.lib(), Kc.current_stream()
    rng = np.random.default_rng(1000 * A + 10 * K + k + B)
    n = _pad(A * K, n_round)
    m, ldx, ldw, ldo = 2 * B, k + 8, k + 16, n + 4
    x, wt, bb = _operands(rng, 2, m, n, k, dtype, bias)
    x[1, :B] = np.nan                                     # the target network's obs_tm1 activations: nobody may read them
    x_d, x_v = _dev(x, dtype)
    w_d, w_v = _dev(wt, dtype)
    b_d, b_v = _dev(bb, dtype) if bias else (None, None)
    odt = torch.float32 if out32 else getattr(torch, dtype)
    flags = _flags(dtype, out32, relu=False)
    strides = (m * ldx, n * ldw, m * ldo)
    gemm = torch.full((2, m, ldo), float("nan"), dtype=odt, device="cuda")
    Kc.check(L.hb_thin_gemm(_ptr(x_d), _ptr(w_d), _ptr(b_d), _ptr(gemm), m, n, k, ldx, ldw, ldo, 2, *strides, flags, s))
    ref, err = np.zeros((2, m, n)), np.zeros((2, m, n))
    for z, rows in ((0, slice(0, m)), (1, slice(B, m))):
        ref[z, rows], err[z, rows] = AO.thin_gemm(x_v[z, rows, :k], w_v[z][:, :k], None if b_v is None else b_v[z], False)
    if (A, K, B, n) == WALKING:
        units = TF.group_bound(B, A) * TF.npair(K) + 2 * (B // 32) * (n // 16)
        assert units == TF.n_units(2, B, n, A, K) and units > TF.MAX_WORKGROUPS, units
    vectors = _action_vectors(B, A, rng)
    assert ("border" in vectors) == (A >= 4 and B >= 224)
    # "each" holds actions 0 .. min(A, B) - 1, among them the alignment that needs the most tiles: all npair(K) of them, one
    # fewer for K = 16 and 64, whose starts are aligned (the group's last unit then finds no tile)
    assert max(TF.tiles_touched(a * K, K) for a in np.unique(vectors["each"])) == TF.npair(K) - (1 if K % 16 == 0 else 0)
    for name, act in vectors.items():
        assert act.min() >= 0 and act.max() < A and TF.row_groups(act, A) <= TF.group_bound(B, A)
        act_d = torch.as_tensor(act.astype(np.int32)).cuda()
        out = torch.full((2, m, ldo), float("nan"), dtype=odt, device="cuda")
        Kc.check(L.hb_thin_forward(2, _ptr(x_d), _ptr(w_d), _ptr(b_d), _ptr(out), _ptr(act_d), B, n, k, ldx, ldw, ldo, *strides, A, K,
                                   flags, s))
        torch.cuda.synchronize()
        need, may = TF.masks(2, B, n, act, A, K)
        what = f"layer 2 {dtype} A={A} K={K} B={B} n={n} k={k} {name}"
        wrote, o = _check_contract(out, n, need, may, ref, err, dtype, out32, what)
        assert torch.equal(out[wrote], gemm[wrote]), f"{what}: not bit-equal to hb_thin_gemm"
        c = slice(act[0] * K, act[0] * K + K)             # row 0 of x is zero: its logits are exactly the biases
        np.testing.assert_array_equal(o[0, 0, c], b_v[0, c] if bias else np.zeros(K))

