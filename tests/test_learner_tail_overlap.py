"""hb_noisy_adam_multi with a gradient-product entry (hb_adam_tensor.gx; learner_tail_l2_dw1_kernel, csrc/learner2.hip): the
output layer's optimizer step and dW1 = X^T dH in one launch.

Role A (the optimizer step on the caller's table entries) must be bit-identical to hb_noisy_adam_multi; role B (dW1) is held
to a float64 reference computed from the same rounded operands, inside guard bands; and the two roles must not see each other."""
import ctypes as C

import numpy as np
import pytest

from guard_util import FILL, GuardSet, same_bits

pytestmark = pytest.mark.gpu

LR, B1, B2, EPS = 6.25e-5, 0.9, 0.999, 3.125e-5
CODE = {"bfloat16": 1, "float16": 2}
H = 512


def _K():
    from hanabi_hip import _capi as K

    return K


def _tdt(name):
    import torch

    return getattr(torch, name)


def _pad(v, m):
    return (v + m - 1) // m * m


def _game_shape(players):
    """(obs_len, n_actions) of full Hanabi: pure host functions of the library."""
    import hanabi_hip

    cfg = hanabi_hip.make_config("Hanabi-Full", players)
    L = hanabi_hip.lib()
    return L.hb_obs_len(C.byref(cfg)), L.hb_num_actions(C.byref(cfg))


class _Net:
    """The four merged tensors of the one-hidden-layer network as FusedLearner lays them out (direct path): W1 [obs_len, H] with
    its gradient in the GEMM dtype [Kp, H] and its effective copy a column block of [Kp, 2H]; b1 [H]; W2 [H, A*K] with gradient
    and effective copy [H, Np]; b2 [A*K] with an fp32 gradient [Np]; w and w_mu share their moments."""

    def __init__(self, seed, obs_len, n_actions, dtype):
        import torch

        g = torch.Generator(device="cuda").manual_seed(seed)
        dt = _tdt(dtype)
        self.dtype, self.L, self.AK = dtype, obs_len, n_actions * 51
        self.Kp, self.Np = _pad(obs_len, 64), _pad(self.AK, 64)
        shapes = [(obs_len, H), (1, H), (H, self.AK), (1, self.AK)]
        rnd = lambda *s, scale=1.0: torch.randn(*s, device="cuda", generator=g) * scale
        self.params = [[rnd(*s, scale=0.05) for _ in range(3)] for s in shapes]                  # w, w_mu, w_sigma
        self.noise = [rnd(*s) for s in shapes]
        self.mom = [[rnd(*s, scale=1e-3) if k % 2 == 0 else rnd(*s, scale=1e-3).abs() for k in range(4)] for s in shapes]   # m_w, v_w, m_sg, v_sg
        self.gw1 = torch.zeros(self.Kp, H, dtype=dt, device="cuda")
        self.gb1 = torch.zeros(H, device="cuda")
        self.gw2 = torch.zeros(H, self.Np, dtype=dt, device="cuda")
        self.gb2 = torch.zeros(self.Np, device="cuda")
        self.w1cat = torch.zeros(self.Kp, 2 * H, dtype=dt, device="cuda")
        self.b1cat = torch.zeros(2 * H, dtype=dt, device="cuda")
        self.w2 = torch.zeros(H, self.Np, dtype=dt, device="cuda")
        self.b2 = torch.zeros(self.Np, dtype=dt, device="cuda")
        self.step = torch.zeros((), device="cuda")
        K = _K()
        self.tab = (K.HbAdamTensor * 4)()
        grads = [(self.gw1, CODE[dtype], H), (self.gb1, 0, 0), (self.gw2, CODE[dtype], self.Np), (self.gb2, 0, 0)]
        effs = [(self.w1cat, 2 * H), (self.b1cat, H), (self.w2, self.Np), (self.b2, self.AK)]
        for i, d in enumerate(self.tab):
            p, m = self.params[i], self.mom[i]
            d.w, d.w_mu, d.w_sigma, d.noise = (t.data_ptr() for t in (*p, self.noise[i]))
            d.grad, d.grad_dtype, d.grad_ld = grads[i][0].data_ptr(), grads[i][1], grads[i][2]
            d.m_w, d.v_w, d.m_mu, d.v_mu, d.m_sigma, d.v_sigma = (t.data_ptr() for t in (m[0], m[1], m[0], m[1], m[2], m[3]))
            d.eff, d.eff_ld = effs[i][0].data_ptr(), effs[i][1]
            d.n, d.cols = p[0].numel(), p[0].shape[-1]

    def state(self):
        return ([t for p in self.params for t in p] + [t for m in self.mom for t in m] +
                [self.w1cat, self.b1cat, self.w2, self.b2, self.gw1])

    def copy_from(self, other):
        for a, b in zip(self.state() + self.noise + [self.step], other.state() + other.noise + [other.step]):
            a.copy_(b)

    def set_grads(self, seed, x, dh, zero_l2=False):
        import torch

        g = torch.Generator(device="cuda").manual_seed(seed)
        self.gb1.copy_(torch.randn(H, device="cuda", generator=g) * 1e-2)
        self.gw2.zero_()
        self.gb2.zero_()
        if not zero_l2:
            self.gw2[:, :self.AK] = (torch.randn(H, self.AK, device="cuda", generator=g) * 1e-2).to(self.gw2.dtype)
            self.gb2[:self.AK] = torch.randn(self.AK, device="cuda", generator=g) * 1e-2
        self.x, self.dh = x, dh

    def tail(self, n_adam, out=None, out_ld=None):
        """The two-role launch: W1's entry as a gradient product (dW1 into `out`, default its own gradient buffer) and the
        first n_adam of (W2, b2) stepped beside it."""
        K = _K()
        tab = (K.HbAdamTensor * (1 + n_adam))()
        tab[0] = self.tab[0]
        for i in range(n_adam):
            tab[1 + i] = self.tab[2 + i]
        d = tab[0]
        if out is not None:
            d.grad, d.grad_ld = out.data_ptr(), out_ld or H
        d.gx, d.gdh, d.g_batch, d.g_ldx, d.g_ldh = self.x.data_ptr(), self.dh.data_ptr(), self.x.shape[0], self.x.stride(0), self.dh.stride(0)
        K.check(K.lib().hb_noisy_adam_multi(tab, 1 + n_adam, K.dptr(self.step), 0.0, CODE[self.dtype], LR, B1, B2, EPS,
                                            K.current_stream()))

    def adam(self, count):
        K = _K()
        K.check(K.lib().hb_noisy_adam_multi(self.tab, count, K.dptr(self.step), 0.0, CODE[self.dtype], LR, B1, B2, EPS,
                                            K.current_stream()))


def _operands(seed, batch, kp, dtype):
    """X [batch, kp] (every column non-zero, the padding ones included) and dH [batch, H] in `dtype`."""
    import torch

    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(batch, kp, device="cuda", generator=g).to(_tdt(dtype))
    dh = (torch.randn(batch, H, device="cuda", generator=g) * 1e-2).to(_tdt(dtype))
    return x, dh


@pytest.mark.parametrize("players", [2, 5])
@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_role_a_is_bit_identical_to_noisy_adam_multi(dtype, players):
    """The new launch (W2, b2) + hb_noisy_adam_multi on entries 0 and 1, against ONE hb_noisy_adam_multi over all four entries
    from the same inputs: parameters, moments and effective copies equal bit for bit over 3 consecutive steps. 2 players:
    every tensor takes the 4-wide form; 5 players: A * K = 2550 is no multiple of 4, the scalar form."""
    import torch

    obs_len, n_act = _game_shape(players)
    new, old = _Net(7 + players, obs_len, n_act, dtype), _Net(7 + players, obs_len, n_act, dtype)
    old.copy_from(new)
    for t in range(1, 4):
        x, dh = _operands(100 * t + players, 256, new.Kp, dtype)
        for n in (new, old):
            n.step.fill_(float(t))
            n.set_grads(10 * t, x, dh)
        new.tail(2)
        new.adam(2)
        old.gw1.copy_(new.gw1)        # the same dW1 for the reference step
        old.adam(4)
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(new.state(), old.state())):
            assert same_bits(a, b) == -1, (t, i, same_bits(a, b))
    assert float(new.w2[:, :new.AK].float().abs().max()) > 0 and float(new.w1cat[:obs_len, :H].float().abs().max()) > 0


@pytest.mark.parametrize("obs_len", [171, 658, 1280])
@pytest.mark.parametrize("batch", [1, 17, 256])
@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_role_b_equals_f64_reference_inside_guard_bands(dtype, batch, obs_len):
    """dW1 = X^T dH against numpy float64 on the same rounded operands. Tolerance: ONE rounding of the fp32-accumulated sum to the
    output format, |err| <= 2^-8 |ref| (bf16: 8 significand bits) or 2^-11 |ref| (fp16: 11), plus `tiny`: the fp32 accumulation
    itself, batch additions of at most one fp32 ulp (2 * 2^-24: the MFMA adder may truncate) of sum |x| |dh| each, and half the
    smallest fp16 subnormal. The output has 8 padding columns per row and guard bands around it: nothing but rows [0, obs_len)
    x columns [0, H) may be written. obs_len 171: 5 full 32-row tiles and 11 rows; 658: 20 and 18; 1280: 40 whole tiles."""
    import torch

    K = _K()
    kp = _pad(obs_len, 64)
    x, dh = _operands(obs_len + batch, batch, kp, dtype)
    gs = GuardSet("hb_noisy_adam_multi, gradient product")
    gs.inp("x", x)
    gs.inp("dh", dh)
    ld = H + 8
    out = gs.out("dw1", (obs_len, ld), dtype, 64 * ld)
    tab = (K.HbAdamTensor * 1)()
    d = tab[0]
    d.grad, d.grad_dtype, d.grad_ld, d.n, d.cols = out.data_ptr(), CODE[dtype], ld, obs_len * H, H
    d.gx, d.gdh, d.g_batch, d.g_ldx, d.g_ldh = x.data_ptr(), dh.data_ptr(), batch, kp, H
    step = torch.ones((), device="cuda")
    K.check(K.lib().hb_noisy_adam_multi(tab, 1, K.dptr(step), 0.0, CODE[dtype], LR, B1, B2, EPS, K.current_stream()))
    torch.cuda.synchronize()
    gs.check()
    assert bool((out[:, H:].contiguous().view(torch.uint8) == FILL).all()), "padding columns written"
    x64, d64 = x[:, :obs_len].double().cpu().numpy(), dh.double().cpu().numpy()
    ref, mag = x64.T @ d64, np.abs(x64).T @ np.abs(d64)
    got = out[:, :H].double().cpu().numpy()
    rel = 2.0 ** -8 if dtype == "bfloat16" else 2.0 ** -11
    tiny = batch * 2.0 ** -23 * mag * (1 + rel) + (2.0 ** -25 if dtype == "float16" else 0.0)
    err = np.abs(got - ref)
    worst = float((err / (rel * np.abs(ref) + tiny)).max())
    print(f"dw1 {dtype} B={batch} obs_len={obs_len}: worst error / bound = {worst:.3f}")
    assert np.isfinite(got).all() and worst <= 1.0, worst


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_roles_do_not_interfere(dtype):
    """dH = 0: dW1 is exactly zero while the output layer still steps. Zero output-layer gradients: dW1 equals the role-B-only
    launch bit for bit (and the output layer's moments only decay)."""
    import torch

    obs_len, n_act = _game_shape(2)
    net = _Net(3, obs_len, n_act, dtype)
    net.step.fill_(1.0)
    x, dh = _operands(5, 256, net.Kp, dtype)
    w2_before, w1_before = net.params[2][0].clone(), net.params[0][0].clone()
    net.set_grads(1, x, torch.zeros_like(dh))
    net.gw1.fill_(1.0)
    net.tail(2)
    torch.cuda.synchronize()
    assert bool((net.gw1[:obs_len] == 0).all()) and bool((net.gw1[obs_len:] == 1).all())
    assert bool((net.params[2][0] != w2_before).any()) and same_bits(net.params[0][0], w1_before) == -1
    net.set_grads(2, x, dh, zero_l2=True)
    alone = torch.zeros_like(net.gw1)
    net.tail(0, out=alone)
    net.tail(2)
    torch.cuda.synchronize()
    assert same_bits(net.gw1[:obs_len], alone[:obs_len]) == -1 and float(alone.float().abs().max()) > 0
