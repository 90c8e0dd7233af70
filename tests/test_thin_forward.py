"""GPU: hb_thin_forward (csrc/learner2.hip), the learner's forward pass restricted to what the C51 loss and the backward read.

1. Bit equality with hb_thin_gemm through the C-ABI on every element the new entry writes, bf16 and fp16, the 2-player and the
   5-player shape, B = 256 and a smaller batch, with the batch's actions all equal, all different, and drawn uniformly; the
   elements it must NOT write keep the NaN they were filled with.
2. Nothing else is read: with the logits and the target x obs_tm1 block of the hidden activations filled with NaN before the
   forward, FusedLearner's loss + backward give td, IS weights, loss and all four gradients equal to the dense forward's.
3. Training: N updates with prioritized replay on the trimmed forward leave weights, Adam moments and the sum tree equal to the
   same updates on the two hb_thin_gemm calls.
Everything is torch.equal: each output element is one chain of MFMA accumulations over its own row and column in ascending k, in
both kernels."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

K51, HID = 51, 512
SHAPES = {2: (658, 20), 5: (1280, 48)}          # players -> (observation bits, actions)


def _K():
    from hanabi_hip import _capi as K

    return K


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _pad(v, m):
    return (v + m - 1) // m * m


def _actions(kind, B, A, g):
    import torch

    if kind == "one":
        return torch.full((B,), A - 1, dtype=torch.int32, device="cuda")
    if kind == "each":            # every action once (as far as the batch goes), the rest of the batch on action 0
        a = torch.zeros(B, dtype=torch.int32, device="cuda")
        n = min(A, B)
        a[torch.randperm(B, device="cuda", generator=g)[:n]] = torch.arange(n, dtype=torch.int32, device="cuda")
        return a
    return torch.randint(0, A, (B,), device="cuda", generator=g, dtype=torch.int32)


@pytest.mark.parametrize("kind", ["one", "each", "uniform"])
@pytest.mark.parametrize("B", [256, 96])
@pytest.mark.parametrize("players", [2, 5])
@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_bit_equal_to_thin_gemm_where_it_writes(dtype, players, B, kind):
    import torch

    K = _K()
    L = K.lib()
    s = K.current_stream()
    dt = getattr(torch, dtype)
    f16 = 4 if dtype == "float16" else 0
    obs_len, A = SHAPES[players]
    Kp, Np, H = _pad(obs_len, 64), _pad(A * K51, 64), HID
    g = torch.Generator(device="cuda").manual_seed(1000 * players + B)
    x = (torch.rand(2 * B, Kp, device="cuda", generator=g) < 0.3).to(dt)
    w1t = (torch.randn(2 * H, Kp, device="cuda", generator=g) * 0.05).to(dt)
    b1 = (torch.randn(2 * H, device="cuda", generator=g) * 0.1).to(dt)
    w2t = (torch.randn(2, Np, H, device="cuda", generator=g) * 0.05).to(dt)
    b2 = (torch.randn(2, Np, device="cuda", generator=g) * 0.1).to(dt)
    act = _actions(kind, B, A, g)

    # ---- layer 1: bias + ReLU, 16-bit output
    h_ref = torch.zeros(2 * B, 2 * H, dtype=dt, device="cuda")
    K.check(L.hb_thin_gemm(_ptr(x), _ptr(w1t), _ptr(b1), _ptr(h_ref), 2 * B, 2 * H, Kp, Kp, Kp, 2 * H, 1, 0, 0, 0, 1 | f16, s))
    h = torch.full((2 * B, 2 * H), float("nan"), dtype=dt, device="cuda")
    K.check(L.hb_thin_forward(1, _ptr(x), _ptr(w1t), _ptr(b1), _ptr(h), None, B, 2 * H, Kp, Kp, Kp, 2 * H, 0, 0, 0, 0, 0, 1 | f16, s))
    wrote1 = torch.ones(2 * B, 2 * H, dtype=torch.bool, device="cuda")
    wrote1[:B, H:] = False
    assert not torch.isnan(h_ref).any()
    assert torch.equal(h[wrote1], h_ref[wrote1])
    assert torch.isnan(h[~wrote1]).all()

    # ---- layer 2: {online, target}, fp32 output with the biases added
    lg_ref = torch.zeros(2, 2 * B, Np, dtype=torch.float32, device="cuda")
    K.check(L.hb_thin_gemm(_ptr(h_ref), _ptr(w2t), _ptr(b2), _ptr(lg_ref), 2 * B, Np, H, 2 * H, H, Np, 2, H, Np * H, 2 * B * Np,
                           2 | f16, s))
    lg = torch.full((2, 2 * B, Np), float("nan"), dtype=torch.float32, device="cuda")
    K.check(L.hb_thin_forward(2, _ptr(h_ref), _ptr(w2t), _ptr(b2), _ptr(lg), _ptr(act), B, Np, H, 2 * H, H, Np, H, Np * H,
                              2 * B * Np, A, K51, 2 | f16, s))
    # (need / may: tests/test_thin_forward_cpu.py holds oracle/thin_forward_oracle.py's masks to these expressions; change both)
    cols = torch.arange(Np, device="cuda")
    a64 = act.long()
    need = (cols[None, :] >= (a64 * K51)[:, None]) & (cols[None, :] < ((a64 + 1) * K51)[:, None])          # what the loss reads
    tile_lo, tile_hi = (a64 * K51) // 16 * 16, ((a64 + 1) * K51 - 1) // 16 * 16 + 16
    may = (cols[None, :] >= tile_lo[:, None]) & (cols[None, :] < tile_hi[:, None])                          # its 16-column tiles
    assert torch.equal(lg[:, B:], lg_ref[:, B:])                        # obs_t: both networks, dense
    assert torch.isnan(lg[1, :B]).all()                                 # target on obs_tm1: never
    on = lg[0, :B]
    assert torch.equal(on[need], lg_ref[0, :B][need])
    wrote2 = ~torch.isnan(on)
    assert bool((wrote2 <= may).all()) and bool((need <= wrote2).all())
    assert torch.equal(on[wrote2], lg_ref[0, :B][wrote2])

    # ---- 16-bit output of the same launch shape (the entry's other output form)
    o16_ref = torch.zeros(2, 2 * B, Np, dtype=dt, device="cuda")
    K.check(L.hb_thin_gemm(_ptr(h_ref), _ptr(w2t), _ptr(b2), _ptr(o16_ref), 2 * B, Np, H, 2 * H, H, Np, 2, H, Np * H, 2 * B * Np,
                           f16, s))
    o16 = torch.full((2, 2 * B, Np), float("nan"), dtype=dt, device="cuda")
    K.check(L.hb_thin_forward(2, _ptr(h_ref), _ptr(w2t), _ptr(b2), _ptr(o16), _ptr(act), B, Np, H, 2 * H, H, Np, H, Np * H,
                              2 * B * Np, A, K51, f16, s))
    w16 = ~torch.isnan(o16)
    assert torch.equal(w16[0, :B], wrote2) and bool(w16[:, B:].all()) and not bool(w16[1, :B].any())
    assert torch.equal(o16[w16], o16_ref[w16])


def test_argument_validation():
    K = _K()
    L = K.lib()
    one = C.c_void_p(16)
    assert L.hb_thin_forward(3, one, one, None, one, one, 32, 64, 32, 32, 32, 64, 0, 0, 0, 4, 8, 0, None) < 0 and b"layer" in L.hb_last_error()
    assert L.hb_thin_forward(1, one, one, None, one, None, 48, 64, 32, 32, 32, 64, 0, 0, 0, 0, 0, 0, None) < 0 and b"batch % 32" in L.hb_last_error()
    assert L.hb_thin_forward(2, one, one, None, one, None, 32, 64, 32, 32, 32, 64, 0, 0, 0, 4, 8, 0, None) < 0 and b"null" in L.hb_last_error()
    assert L.hb_thin_forward(2, one, one, None, one, one, 512, 64, 32, 32, 32, 64, 0, 0, 0, 4, 8, 0, None) < 0 and b"256" in L.hb_last_error()
    assert L.hb_thin_forward(2, one, one, None, one, one, 32, 64, 32, 32, 32, 64, 0, 0, 0, 4, 17, 0, None) < 0 and b"n_actions" in L.hb_last_error()
    assert L.hb_thin_forward(1, one, one, None, one, None, 32, 64, 32, 32, 32, 64, 0, 0, 0, 0, 0, 8, None) < 0 and b"relu" in L.hb_last_error()
    assert L.hb_thin_forward(1, one, one, None, one, None, 0, 64, 32, 32, 32, 64, 0, 0, 0, 0, 0, 0, None) == 0


def _agent(dtype, players, n, use_priority, seed=3):
    import torch

    from hanabi_agents.rlax_dqn import ActionSpec, DQNAgent, ObservationSpec, RlaxRainbowParams

    obs_len, n_act = SHAPES[players]
    params = RlaxRainbowParams(use_priority=use_priority, train_batch_size=256, experience_buffer_size=n, target_update_period=3,
                               mask_terminal=True, compute_dtype=dtype, seed=seed, learning_rate=0.01)
    a = DQNAgent(ObservationSpec((n, obs_len)), ActionSpec(n_act), params, device="cuda", use_graphs=use_priority,
                 use_fused_learner=True)
    g = torch.Generator(device="cuda").manual_seed(7 + players)
    with torch.no_grad():          # non-zero biases and bias noise, target != online
        for layer in a.online.layers:
            layer.b_sigma.fill_(0.05)
            layer.b.fill_(0.02)
        a.target.load_state_dict(a.online.state_dict())
        for p in a.target.parameters():
            p.add_(torch.randn(p.shape, device="cuda", generator=g) * 0.01)
    o1 = (torch.rand(n, obs_len, device="cuda", generator=g) < 0.3).to(torch.int8)
    o2 = (torch.rand(n, obs_len, device="cuda", generator=g) < 0.3).to(torch.int8)
    legal = torch.ones(n, n_act, dtype=torch.int8, device="cuda")
    act = torch.randint(0, n_act, (n,), device="cuda", generator=g, dtype=torch.int32)
    rew = torch.randint(-1, 2, (n,), device="cuda", generator=g).float()
    st = torch.randint(1, 3, (n,), device="cuda", generator=g).to(torch.int8)
    a.add_experience_first((None, (o1, legal)), torch.zeros(n, dtype=torch.int8, device="cuda"))
    a.add_experience((None, (o2, legal)), act, rew, st)
    return a, g


@pytest.mark.parametrize("players", [2, 5])
@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_loss_and_backward_read_nothing_else(dtype, players):
    import torch

    n = 256
    a, g = _agent(dtype, players, n, use_priority=False)
    fl = a._fused_learner()
    assert fl is not None and fl.thin and fl.trimmed and fl.sparse_backward
    idx = torch.randperm(n, device="cuda", generator=g)
    pri = (torch.rand(n, device="cuda", generator=g, dtype=torch.float64) + 0.05) / n
    B, H = fl.B, fl.H

    def run(dense):
        fl._dense_forward = dense
        fl._logits.fill_(float("nan"))
        fl._hcat[:B, H:].fill_(float("nan"))
        for t in (fl._gw1_out, fl.g_b1, fl._gw2_out, fl._gb2_pad, fl.td, fl.w_is, fl.dl, fl.dh):
            t.zero_()
        fl.part1(idx, pri)
        torch.cuda.synchronize()
        return [t.clone() for t in (fl.td, fl.w_is, fl.loss(), fl._gw1_out, fl.g_b1, fl._gw2_out, fl._gb2_pad)]

    dense, trimmed = run(True), run(False)
    assert torch.isnan(fl._logits[1, :B]).all() and torch.isnan(fl._hcat[:B, H:]).all()    # the trimmed forward left them alone
    for name, x, y in zip(("td", "is_weights", "loss", "dW1", "db1", "dW2", "db2"), dense, trimmed):
        assert not torch.isnan(x).any() and not torch.isnan(y).any(), name
        assert torch.equal(x, y), name


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_training_equals_the_dense_forward(dtype):
    import torch

    def run(dense):
        torch.manual_seed(0)
        a, _ = _agent(dtype, 2, 4096, use_priority=True)
        fl = a._fused_learner()
        assert fl.thin and fl.trimmed
        fl._dense_forward = dense
        for _ in range(12):
            a.update()
        torch.cuda.synchronize()
        out = [p.detach().clone() for p in a.online.parameters()] + [p.detach().clone() for p in a.target.parameters()]
        for key in sorted(fl.state):
            out += [fl.state[key][0].clone(), fl.state[key][1].clone()]
        out.append(a.experience.sum_tree.nodes().clone())
        return out

    ref, got = run(True), run(False)
    assert len(ref) == len(got)
    for k, (x, y) in enumerate(zip(ref, got)):
        assert torch.equal(x, y), f"item {k} differs"
