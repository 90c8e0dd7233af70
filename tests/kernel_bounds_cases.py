"""The case table of the guard-band sweep: one or more cases per C-ABI entry point that writes device memory supplied by the
caller (tests/test_kernel_bounds_gpu.py runs them; tests/test_kernel_bounds_cpu.py holds the table against _capi.SIGNATURES).

A case is (function, parameters). The function takes a buffer set `g` (guard_util.GuardSet or guard_util.PlainSet) as its first
argument, builds its inputs with the builders the oracle tests already have, registers them with `g.inp`, takes EVERY output
from `g.out` and calls the entry point once through hanabi_hip._capi. It is run twice, on a GuardSet and on a PlainSet, so
it must build the same inputs both times (fixed seeds, fresh envs and trees).

Every tail guard is `tail(tile_rows, row_elems)`: the rows one workgroup of the kernel covers (the constants below, each read
from the launch code named beside it) times the elements of one output row, never below guard_util.FRONT.

This module imports nothing that needs a device: torch and the builders are imported inside the case functions."""
import ctypes as C
import os

import numpy as np

from guard_util import FRONT

# ---- rows one workgroup covers, from the kernels ------------------------------------------------------------------------------
ENV_WAVES = 4        # env_kernel / env_kernel_shuf (csrc/env_kernel.hpp): 256 threads = 4 wavefronts of G games each
FUSED_ROWS = 128     # actor_fused_kernel, actor_fused_grouped_kernel, actor_env_fused_kernel (csrc/actor_fused.hip): FM
GEMM_ROWS = 256      # actor_gemm_kernel (csrc/actor.hip): BM
SELECT_ROWS = 128    # policy_select_kernel (csrc/actor.hip): SEL_T
RULE_ROWS = 128      # rule_kernel / rule_grouped_kernel (csrc/rule_agent.hip): one lane per game, 128 threads
LANE_ROWS = 256      # one lane per row in 256-thread workgroups: random_legal_kernel, get_kernel, the tallies, colour perms,
                     # train_tally_init_kernel, belief_history_step_kernel; and the 16-byte chunks of the grid-stride copies
WAVE_ROWS = 4        # one wavefront per row, four per workgroup: sample_kernel, per_sample_kernel, c51_kernel, every
                     # belief / search kernel but the history step (csrc/belief.hip: blocks = (rows + 3) / 4)
BLOCK_ROW = 1        # one workgroup per row: gather_kernel, per_sample_gather_kernel, c51_sparse_kernel
COLSUM_COLS = 64     # colsum_kernel / relu_bwd_colsum_kernel (csrc/learner.hip): 64 columns per workgroup, 16 row lanes
THIN_ROWS = 32       # thin_gemm_kernel / thin_forward_kernel (csrc/learner2.hip): a wavefront owns 32 rows x 16 columns
ADAM_PACK_ROWS = 8   # noisy_adam_pack_kernel: 8 rows x 128 columns per workgroup
CHUNK = 16           # bytes of one vector store

HID, K51 = 512, 51
# observation 658 / 1280 / 171 bytes, legal mask 20 / 48 / 11 bytes, packed rows 21 / 40 / 6 words, state rows 32 / 48 / 32 words
GAMES = {"full2": ("Hanabi-Full", 2), "full5": ("Hanabi-Full", 5), "small2": ("Hanabi-Small", 2)}
CODE = {"float32": 0, "bfloat16": 1, "float16": 2}

CASES = {}           # entry point -> [(function, parameter tuple)]


def tail(tile_rows, row_elems):
    return max(FRONT, int(tile_rows) * int(row_elems))


def case(entry, params):
    def deco(fn):
        CASES.setdefault(entry, []).extend((fn, tuple(p)) for p in params)
        return fn
    return deco


def edge_sizes(tile, block=None):
    """{1, T - 1, T + 1} of a row tile T and, where a workgroup holds several tiles, one row past a whole workgroup."""
    s = {1, tile - 1, tile + 1}
    if block is not None and block != tile:
        s.add(block + 1)
    return sorted(x for x in s if x >= 1)


# ---- small helpers (device side; called from case functions only) ---------------------------------------------------------
def _K():
    from hanabi_hip import _capi as K

    return K


def _cuda(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _call(name, *args):
    K = _K()
    K.check(getattr(K.lib(), name)(*args, K.current_stream()))


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


# =================================================================================================================================
# Env
# =================================================================================================================================
def _env(game_key, n, turns=6, shuffled=False, gpw=None):
    from search_util import _mid_game_env

    game, players = GAMES[game_key]
    env = _mid_game_env(game, players, n, turns, seed=3 + n)
    if gpw is not None:
        env.set_games_per_wave(gpw)
    if shuffled:
        env.set_color_shuffle(True)
    return env


# the per-game outputs of an env step, all nullable ([n] each); an observe writes the two agent_* ones only
STEP_OUTS = (("reward", "float32"), ("terminal", "int8"), ("agent_reward", "float32"), ("agent_step_type", "int8"), ("score", "int8"))


def _env_outs(g, env, T, with_bits, with_obs8, with_nullable, step=True):
    """The outputs of an env step (or, step=False, of an observe), each guarded by one workgroup's games T times its row length."""
    n = env.n
    o = {}
    o["bits"] = g.out("obs_bits", (n, env.obs_words), "int32", tail(T, env.obs_words)) if with_bits else None
    o["obs"] = g.out("obs", (n, env.obs_len), "int8", tail(T, env.obs_len)) if with_obs8 else None
    o["legal"] = g.out("legal", (n, env.num_actions), "int8", tail(T, env.num_actions))
    for name, dt in STEP_OUTS:
        o[name] = g.out(name, (n,), dt, tail(T, 1)) if with_nullable and (step or name.startswith("agent_")) else None
    return o


def _env_grid():
    """(game, G, n, shuffled, variant) over every games-per-wave and edge size; game and the output variant cycle."""
    out = []
    for sh in (False, True):
        i = 0
        for G in (16, 32, 64):
            for n in edge_sizes(G, ENV_WAVES * G):
                out.append((list(GAMES)[(i + (1 if sh else 0)) % 3], G, n, sh, i % 4))
                i += 1
    return out


@case("hb_env_observe", [p[:4] + (p[4] % 2,) for p in _env_grid()])
def env_observe(g, game, G, n, shuffled, variant):
    env = _env(game, n, shuffled=shuffled, gpw=G)
    o = _env_outs(g, env, ENV_WAVES * G, False, True, variant == 0, step=False)
    _call("hb_env_observe", env.h, _p(o["obs"]), _p(o["legal"]), _p(o["agent_reward"]), _p(o["agent_step_type"]))


@case("hb_env_observe_packed", _env_grid())
def env_observe_packed(g, game, G, n, shuffled, variant):
    env = _env(game, n, shuffled=shuffled, gpw=G)
    o = _env_outs(g, env, ENV_WAVES * G, True, variant & 1, variant & 2, step=False)
    _call("hb_env_observe_packed", env.h, _p(o["bits"]), _p(o["obs"]), _p(o["legal"]), _p(o["agent_reward"]),
          _p(o["agent_step_type"]))


@case("hb_env_step", [p[:4] + (p[4] % 2,) for p in _env_grid()])
def env_step(g, game, G, n, shuffled, variant):
    env = _env(game, n, shuffled=shuffled, gpw=G)
    act = g.inp("actions", env.random_legal_actions(seed=9, draw=77))
    o = _env_outs(g, env, ENV_WAVES * G, False, True, variant == 0)
    _call("hb_env_step", env.h, _p(act), _p(o["obs"]), _p(o["legal"]), _p(o["reward"]), _p(o["terminal"]), _p(o["agent_reward"]),
          _p(o["agent_step_type"]), _p(o["score"]))


@case("hb_env_step_packed", _env_grid())
def env_step_packed(g, game, G, n, shuffled, variant):
    env = _env(game, n, shuffled=shuffled, gpw=G)
    act = g.inp("actions", env.random_legal_actions(seed=9, draw=77))
    o = _env_outs(g, env, ENV_WAVES * G, True, variant & 1, variant & 2)
    _call("hb_env_step_packed", env.h, _p(act), _p(o["bits"]), _p(o["obs"]), _p(o["legal"]), _p(o["reward"]), _p(o["terminal"]),
          _p(o["agent_reward"]), _p(o["agent_step_type"]), _p(o["score"]))


@case("hb_env_step_select_packed", _env_grid())
def env_step_select_packed(g, game, G, n, shuffled, variant):
    import torch

    env = _env(game, n, shuffled=shuffled, gpw=G)
    gen = torch.Generator(device="cuda").manual_seed(n + G)
    q = g.inp("q", torch.randn(n, env.num_actions, device="cuda", generator=gen))
    sel = g.inp("sel_legal", env.legal.clone())
    T = ENV_WAVES * G
    acts = g.out("actions_out", (n,), "int32", tail(T, 1))
    o = _env_outs(g, env, T, True, variant & 1, variant & 2)
    K = _K()
    K.check(K.lib().hb_env_step_select_packed(env.h, _p(q), _p(sel), 0.25, (5 << 32) | 3, 11, (1 << 32) - 5, _p(acts), _p(o["bits"]),
                                              _p(o["obs"]), _p(o["legal"]), _p(o["reward"]), _p(o["terminal"]), _p(o["agent_reward"]),
                                              _p(o["agent_step_type"]), _p(o["score"]), K.current_stream()))


@case("hb_env_export_state", [(k, n) for k in GAMES for n in (1, 65)])
def env_export_state(g, game, n):
    env = _env(game, n)
    rows = g.out("rows", (n, env.state_words), "int32", tail(LANE_ROWS, env.state_words))   # a device-to-device copy: no tile
    _call("hb_env_export_state", env.h, _p(rows))


def _perm_sizes():
    out = []
    for k, (game, players) in GAMES.items():
        row = players * (5 if "Full" in game else 2)           # [players, colors] bytes per game
        per_wg = LANE_ROWS // row                               # color_perms_export_kernel: one lane per byte
        out += [(k, n, sh) for n in (1, per_wg, per_wg + 1) for sh in (False, True)]
    return out


@case("hb_env_color_perms", _perm_sizes())
def env_color_perms(g, game, n, shuffled):
    env = _env(game, n, shuffled=shuffled)
    row = env.players * env.cfg.colors
    out = g.out("perms", (n, env.players, env.cfg.colors), "uint8", tail(LANE_ROWS, 1) + row)
    _call("hb_env_color_perms", env.h, _p(out))


def _obs_rows(n, L, seed):
    rng = np.random.default_rng(seed)
    return (rng.random((n, L)) < 0.4).astype(np.int8)


# obs_pack_kernel: one wavefront per 64-byte chunk of a row, four per workgroup -> 4 / ceil(L / 64) rows per workgroup
@case("hb_obs_pack", [(L, n) for L in (658, 171, 64, 65, 1) for n in sorted({1, max(1, 4 // -(-L // 64)) + 1, 3, 5})])
def obs_pack(g, L, n):
    from replay_cases import words_for

    obs = g.inp("obs", _cuda(_obs_rows(n, L, L + n)))
    W = words_for(L)
    bits = g.out("bits", (n, W), "int32", tail(WAVE_ROWS, 2))      # a wavefront writes the two words of its chunk
    _call("hb_obs_pack", _p(obs), _p(bits), n, L)


# obs_unpack_kernel: one lane per 16-column chunk, 256 per workgroup -> 256 / ceil(L / 16) rows per workgroup
@case("hb_obs_unpack", [(L, n) for L in (658, 171, 16, 15, 1) for n in edge_sizes(max(2, LANE_ROWS // -(-L // 16)))])
def obs_unpack(g, L, n):
    from replay_cases import pack_rows

    bits = g.inp("bits", _cuda(pack_rows(_obs_rows(n, L, L + n), L)))
    obs = g.out("obs", (n, L), "int8", tail(LANE_ROWS, CHUNK))
    _call("hb_obs_unpack", _p(bits), _p(obs), n, L)


# obs_cast_kernel: grid-stride, one lane per 16-column chunk
@case("hb_obs_cast", [(L, n, dt) for L in (658, 171, 15) for n in edge_sizes(max(2, LANE_ROWS // max(1, L // 16)))
                      for dt in ("bfloat16", "float16")])
def obs_cast(g, L, n, dtype):
    obs = g.inp("obs", _cuda(_obs_rows(n, L, L + n)))
    ld = L + 6
    out = g.out("out", (n, ld), dtype, tail(LANE_ROWS, CHUNK))
    _call("hb_obs_cast", _p(obs), _p(out), CODE[dtype], n, L, ld)


@case("hb_random_legal_actions", [(A, n) for A in (20, 11, 48) for n in edge_sizes(LANE_ROWS)])
def random_legal_actions(g, A, n):
    rng = np.random.default_rng(A + n)
    legal = (rng.random((n, A)) < 0.5).astype(np.int8)
    legal[::7] = 0
    legal_d = g.inp("legal", _cuda(legal))
    acts = g.out("actions", (n,), "int32", tail(LANE_ROWS, 1))     # random_legal_kernel: one lane per game
    K = _K()
    K.check(K.lib().hb_random_legal_actions(_p(legal_d), n, A, (3 << 32) | 1, 5, (1 << 32) - 3, _p(acts), K.current_stream()))


# =================================================================================================================================
# One-kernel actor
# =================================================================================================================================
FUSED_SHAPES = [(658, 20), (1280, 48), (171, 11)]     # (observation bits, actions)


def _fused_inputs(g, obs_len, A, dtype, n, seed=5):
    """A packed network (_Fused), bit rows with garbage padding bits, a legal mask and a support, registered as inputs."""
    import test_actor_kernels_f64 as TA

    net = TA._Fused(obs_len, A, dtype, "moderate", seed=seed)
    for nm in ("w1f", "b1f", "w2f", "b2f"):
        g.inp(nm, getattr(net, nm))
    bits, _ = TA._bits_rows(n, obs_len, seed=n + A, garbage=True)
    bits_d = g.inp("obs_bits", _cuda(bits.view(np.int32)))
    legal_d = g.inp("legal", _cuda(TA._legal_cases(n, A, np.random.default_rng(n + A))))
    sup_d = g.inp("support", _cuda(TA.SUPPORTS["lin"].astype(np.float32)))
    return net, bits_d, legal_d, sup_d


def _fused_grid():
    return [sh + (dt, n) for n in edge_sizes(FUSED_ROWS) for dt in ("bfloat16", "float16") for sh in FUSED_SHAPES]


@case("hb_actor_fused_q_dt", [p + ("hb_actor_fused_q_dt",) for p in _fused_grid()])
@case("hb_actor_fused_q", [p + ("hb_actor_fused_q",) for p in _fused_grid() if p[2] == "bfloat16"])
def fused_q(g, obs_len, A, dtype, n, entry):
    net, bits, _, sup = _fused_inputs(g, obs_len, A, dtype, n)
    q = g.out("q", (n, A), "float32", tail(FUSED_ROWS, A))
    args = (_p(bits), n, obs_len, _p(net.w1f), _p(net.b1f), _p(net.w2f), _p(net.b2f), _p(sup), HID, A, K51, _p(q))
    if entry == "hb_actor_fused_q":
        _call("hb_actor_fused_q", *args)
    else:
        _call("hb_actor_fused_q_dt", *args, net.code)


@case("hb_actor_fused_act_dt", [p + ("hb_actor_fused_act_dt",) for p in _fused_grid()])
@case("hb_actor_fused_act", [p + ("hb_actor_fused_act",) for p in _fused_grid() if p[2] == "bfloat16"])
def fused_act(g, obs_len, A, dtype, n, entry):
    net, bits, legal, sup = _fused_inputs(g, obs_len, A, dtype, n)
    q = g.out("q", (n, A), "float32", tail(FUSED_ROWS, A))
    acts = g.out("actions", (n,), "int32", tail(FUSED_ROWS, 1))
    args = (_p(bits), _p(legal), n, obs_len, _p(net.w1f), _p(net.b1f), _p(net.w2f), _p(net.b2f), _p(sup), HID, A, K51, _p(q), 0.25,
            (0xABCD << 32) | 17, (5 << 32) | 3, (1 << 32) - 5, _p(acts))
    if entry == "hb_actor_fused_act":
        _call("hb_actor_fused_act", *args)
    else:
        _call("hb_actor_fused_act_dt", *args, net.code)


# n_rows must be a multiple of 128: one, two and three tiles; the middle (or only second) tile inactive
@case("hb_actor_fused_act_grouped", [sh + (dt, t) for t in (1, 2, 3) for dt in ("bfloat16", "float16") for sh in FUSED_SHAPES[::2]])
def fused_act_grouped(g, obs_len, A, dtype, n_tiles):
    import torch

    import test_actor_kernels_f64 as TA

    n = FUSED_ROWS * n_tiles
    net, bits, legal, sup = _fused_inputs(g, obs_len, A, dtype, n)
    net2 = TA._Fused(obs_len, A, dtype, "wide", seed=9)
    Tile = _K().HbFusedTile
    tiles = (Tile * n_tiles)()
    for t in range(n_tiles):
        nt = (net, net2)[t % 2]
        tiles[t] = Tile(nt.w1f.data_ptr(), nt.b1f.data_ptr(), nt.w2f.data_ptr(), nt.b2f.data_ptr(), sup.data_ptr(),
                        (1 << 32) - 5 + 1000 * t, 0 if t == 1 else 1, 0)
    tiles_d = g.inp("tiles", torch.frombuffer(bytearray(bytes(tiles)), dtype=torch.uint8).cuda())
    q = g.out("q", (n, A), "float32", tail(FUSED_ROWS, A))
    acts = g.out("actions", (n,), "int32", tail(FUSED_ROWS, 1))
    _call("hb_actor_fused_act_grouped", _p(tiles_d), n, _p(bits), _p(legal), obs_len, HID, A, K51, _p(q), 0.25, (9 << 32) | 1,
          (1 << 32) | 6, _p(acts), net.code)


# the policy kernel's workgroup steps its own 128 games: every env output is written by 128-row tiles
@case("hb_actor_fused_act_step", [(gk, dt, n, inplace) for gk in ("full2", "full5") for n in edge_sizes(FUSED_ROWS)
                                  for dt, inplace in (("bfloat16", False), ("float16", True))])
def fused_act_step(g, game, dtype, n, inplace):
    import hanabi_hip
    import test_actor_kernels_f64 as TA

    gname, players = GAMES[game]

    env = hanabi_hip.HanabiEnv(gname, players, n_games=n, seed=11 + n, packed=True)
    for t in range(4):
        env.step(env.random_legal_actions(seed=4, draw=t))
    K = _K()
    assert K.lib().hb_actor_fused_step_supported(env.h) == 1
    A, OL = env.num_actions, env.obs_len
    net = TA._Fused(OL, A, dtype, "moderate", seed=5)
    for nm in ("w1f", "b1f", "w2f", "b2f"):
        g.inp(nm, getattr(net, nm))
    sup = g.inp("support", _cuda(TA.SUPPORTS["lin"].astype(np.float32)))
    T = FUSED_ROWS
    q = g.out("q", (n, A), "float32", tail(T, A))
    acts = g.out("actions", (n,), "int32", tail(T, 1))
    if inplace:      # the step's observation / legal rows rewritten in place: in/out arguments
        bits_out = g.out("obs_bits_inout", (n, env.obs_words), "int32", tail(T, env.obs_words), init=env.obs_bits)
        legal_out = g.out("legal_inout", (n, A), "int8", tail(T, A), init=env.legal)
        bits_in, legal_in = bits_out, legal_out
    else:
        bits_in, legal_in = g.inp("obs_bits", env.obs_bits.clone()), g.inp("legal", env.legal.clone())
        bits_out = g.out("obs_bits_out", (n, env.obs_words), "int32", tail(T, env.obs_words))
        legal_out = g.out("legal_out", (n, A), "int8", tail(T, A))
    o = {nm: g.out(nm, (n,), dt, tail(T, 1)) for nm, dt in STEP_OUTS}
    K.check(K.lib().hb_actor_fused_act_step(env.h, _p(bits_in), _p(legal_in), n, OL, _p(net.w1f), _p(net.b1f), _p(net.w2f), _p(net.b2f),
                                            _p(sup), HID, A, K51, _p(q), 0.1, 99, 7, 4096, _p(acts), net.code, _p(bits_out),
                                            _p(legal_out), _p(o["reward"]), _p(o["terminal"]), _p(o["agent_reward"]),
                                            _p(o["agent_step_type"]), _p(o["score"]), K.current_stream()))


def _fused_pack_outs(g, obs_len, A):
    K = _K()
    f1, f2, fb = C.c_int64(), C.c_int64(), C.c_int32()
    K.check(K.lib().hb_actor_fused_sizes(obs_len, HID, A, K51, C.byref(f1), C.byref(f2), C.byref(fb)))
    # actor_fused_pack_kernel: one 16-byte chunk per lane, 256 lanes per workgroup
    w1f = g.out("w1f", (f1.value,), "uint8", tail(LANE_ROWS, CHUNK))
    w2f = g.out("w2f", (f2.value,), "uint8", tail(LANE_ROWS, CHUNK))
    b1f = g.out("b1f", (HID,), "float32", tail(LANE_ROWS, 1))
    b2f = g.out("b2f", (fb.value,), "float32", tail(LANE_ROWS, 1))
    return w1f, b1f, w2f, b2f


@case("hb_actor_fused_pack_thin", [sh + (dt, (3, 1, 2, 0, 3, 2)[2 * i + j]) for i, sh in enumerate(FUSED_SHAPES)
                                   for j, dt in enumerate(("bfloat16", "float16"))])
@case("hb_actor_fused_pack_dt", [sh + (dt, -1) for sh in FUSED_SHAPES for dt in ("bfloat16", "float16")])
@case("hb_actor_fused_pack", [sh + ("bfloat16", -2) for sh in FUSED_SHAPES])
def fused_pack(g, obs_len, A, dtype, thin):
    """thin: bit 0 = the w1t copy, bit 1 = the w2t copy (hb_actor_fused_pack_thin); -1: _pack_dt; -2: _pack."""
    import test_actor_kernels_f64 as TA

    w1, b1, w2, b2 = TA._fused_net(obs_len, A, dtype, "moderate", 7)
    w1_d = g.inp("w1", TA._dev(w1, dtype)[0])
    b1_d = g.inp("b1", TA._dev(b1, dtype)[0])
    w2_d = g.inp("w2", TA._dev(w2, dtype)[0])
    b2_d = g.inp("b2", TA._dev(b2, dtype)[0])
    w1f, b1f, w2f, b2f = _fused_pack_outs(g, obs_len, A)
    head = (_p(w1_d), HID + 8, _p(b1_d), _p(w2_d), A * K51 + 13, _p(b2_d), obs_len, HID, A, K51, _p(w1f), _p(b1f), _p(w2f), _p(b2f))
    if thin == -2:
        _call("hb_actor_fused_pack", *head)
    elif thin == -1:
        _call("hb_actor_fused_pack_dt", *head, CODE[dtype])
    else:
        kp = (obs_len + 63) // 64 * 64
        # the transposed copies: rows kp + 8 / HID + 8 elements apart, 8 elements (one chunk) per lane
        w1t = g.out("w1t", (HID, kp + 8), dtype, tail(LANE_ROWS, CHUNK // 2)) if thin & 1 else None
        w2t = g.out("w2t", (A * K51, HID + 8), dtype, tail(LANE_ROWS, CHUNK // 2)) if thin & 2 else None
        _call("hb_actor_fused_pack_thin", *head, _p(w1t), kp + 8, _p(w2t), HID + 8, CODE[dtype])


# =================================================================================================================================
# Two-kernel actor and selection
# =================================================================================================================================
@case("hb_actor_pack_weights", [(658, 512, 0, 704), (64, 147, 252, 64), (1, 256, 0, 64), (192, 2 * 129, 129, 192)])
def actor_pack_weights(g, k_rows, n_cols, group_cols, k_pad):
    import torch

    import test_actor_kernels_f64 as TA

    rng = np.random.default_rng(k_rows + n_cols)
    w = np.full((k_rows, n_cols + 5), np.nan)
    w[:, :n_cols] = rng.standard_normal((k_rows, n_cols)) * 3
    w_d = g.inp("w", TA._dev(w, "bfloat16")[0])
    b_d = g.inp("bias", TA._dev(rng.standard_normal(n_cols) * 100, "bfloat16")[0])
    n_out = int(TA._phys(n_cols - 1, group_cols)) + 1
    # pack_weights_kernel: 256 lanes per workgroup, one 16-byte chunk (8 bf16) each; entries no input maps to are not written,
    # so both outputs are in/out arguments that start as zeros
    wt = g.out("wt", (n_out, k_pad), "bfloat16", tail(LANE_ROWS, CHUNK // 2),
               init=torch.zeros((n_out, k_pad), dtype=torch.bfloat16, device="cuda"))
    bo = g.out("bias_out", (n_out,), "float32", tail(LANE_ROWS, 1), init=torch.zeros(n_out, device="cuda"))
    K = _K()
    job = K.HbPackJob(w_d.data_ptr(), b_d.data_ptr(), wt.data_ptr(), bo.data_ptr(), k_rows, n_cols, n_cols + 5, group_cols, k_pad)
    K.check(K.lib().hb_actor_pack_weights(C.byref(job), 1, K.current_stream()))


def _hidden_inputs(g, hidden, obs_len, n):
    import test_actor_kernels_f64 as TA

    rng = np.random.default_rng(hidden + obs_len + n)
    kp = (obs_len + 63) // 64 * 64
    w1 = rng.standard_normal((obs_len, hidden)) * (0.6 / np.sqrt(0.25 * obs_len + 1))
    w_d = TA._dev(w1, "bfloat16")[0]
    b_d = TA._dev(rng.standard_normal(hidden) * 0.1, "bfloat16")[0]
    w1t, b1f = TA._pack(w_d, b_d, obs_len, hidden, hidden, 0, kp, hidden)
    g.inp("w1t", w1t)
    g.inp("b1f", b1f)
    bits, obs_of = TA._bits_rows(n, obs_len, seed=n, garbage=True)
    obs8 = g.inp("obs", _cuda(obs_of(np.arange(n)).astype(np.int8)))
    bits_d = g.inp("obs_bits", _cuda(bits.view(np.int32)))
    return w1t, b1f, kp, obs8, bits_d


HIDDEN_GRID = [(h, L, n) for (h, L) in ((256, 171), (512, 658), (256, 1)) for n in edge_sizes(GEMM_ROWS)]


@case("hb_actor_hidden_packed", [p + (True,) for p in HIDDEN_GRID])
@case("hb_actor_hidden", [p + (False,) for p in HIDDEN_GRID])
def actor_hidden(g, hidden, obs_len, n, packed):
    w1t, b1f, kp, obs8, bits = _hidden_inputs(g, hidden, obs_len, n)
    h = g.out("h", (n, hidden), "bfloat16", tail(GEMM_ROWS, hidden))
    _call("hb_actor_hidden_packed" if packed else "hb_actor_hidden", _p(bits if packed else obs8), n, obs_len, _p(w1t), kp, _p(b1f),
          hidden, _p(h))


def _q_inputs(g, A, K, hidden, n):
    import test_actor_kernels_f64 as TA

    h_d, w2t, b2f, sup_d, _ = TA._actor_q_setup(A, K, hidden, n, "moderate", "lin", seed=K * 100 + A)
    for nm, t in (("h", h_d), ("w2t", w2t), ("b2f", b2f), ("support", sup_d)):
        g.inp(nm, t)
    legal = g.inp("legal", _cuda(TA._legal_cases(n, min(A, 64), np.random.default_rng(A))))
    return h_d, w2t, b2f, sup_d, legal


Q_GRID = [(A, K, hid, n) for (A, K, hid) in ((20, 51, 512), (11, 51, 64), (48, 51, 192), (6, 21, 512)) for n in edge_sizes(GEMM_ROWS)]


@case("hb_actor_q", Q_GRID)
def actor_q(g, A, K, hidden, n):
    h_d, w2t, b2f, sup_d, _ = _q_inputs(g, A, K, hidden, n)
    q = g.out("q", (n, A), "float32", tail(GEMM_ROWS, A))
    _call("hb_actor_q", _p(h_d), n, hidden, _p(w2t), _p(b2f), _p(sup_d), A, K, _p(q))


@case("hb_actor_q_select", [p + (tk,) for i, p in enumerate(Q_GRID) for tk in ((True, False) if i % 2 == 0 else (True,))])
def actor_q_select(g, A, K, hidden, n, with_tickets):
    import torch

    h_d, w2t, b2f, sup_d, legal = _q_inputs(g, A, K, hidden, n)
    q = g.out("q", (n, A), "float32", tail(GEMM_ROWS, A))
    acts = g.out("actions", (n,), "int32", tail(GEMM_ROWS, 1))
    nt = -(-n // GEMM_ROWS)
    tickets = None
    if with_tickets:     # zero before the first call, re-armed by the kernel: an in/out argument
        tickets = g.out("tickets", (nt,), "int32", tail(1, 1), init=torch.zeros(nt, dtype=torch.int32, device="cuda"))
    _call("hb_actor_q_select", _p(h_d), n, hidden, _p(w2t), _p(b2f), _p(sup_d), A, K, _p(q), _p(legal), 0.25, (1 << 32) | 3,
          (7 << 32) | 2, (1 << 32) - 5, _p(acts), _p(tickets))


@case("hb_policy_select", [(A, n) for A in (20, 11, 1, 64) for n in edge_sizes(SELECT_ROWS)])
def policy_select(g, A, n):
    import test_actor_kernels_f64 as TA

    rng = np.random.default_rng(A + n)
    q = g.inp("q", _cuda(rng.integers(-2, 3, (n, A)).astype(np.float32) * np.float32(0.125)))
    legal = g.inp("legal", _cuda(TA._legal_cases(n, A, rng)))
    acts = g.out("actions", (n,), "int32", tail(SELECT_ROWS, 1))
    _call("hb_policy_select", _p(q), _p(legal), n, A, 0.25, (5 << 32) | 1, (3 << 32) | 8, (1 << 32) - 5, _p(acts))


@case("hb_actor_act", [(h, L, A, n, pk) for (h, L, A) in ((512, 658, 20), (256, 171, 11)) for n in edge_sizes(GEMM_ROWS)
                       for pk in (False, True)])
def actor_act(g, hidden, obs_len, A, n, packed):
    import torch

    import test_actor_kernels_f64 as TA

    w1t, b1f, kp, obs8, bits = _hidden_inputs(g, hidden, obs_len, n)
    _, w2t, b2f, sup_d, _ = TA._actor_q_setup(A, K51, hidden, 1, "moderate", "lin", seed=A)
    for nm, t in (("w2t", w2t), ("b2f", b2f), ("support", sup_d)):
        g.inp(nm, t)
    legal = g.inp("legal", _cuda(TA._legal_cases(n, A, np.random.default_rng(A))))
    h = g.out("h", (n, hidden), "bfloat16", tail(GEMM_ROWS, hidden))
    q = g.out("q", (n, A), "float32", tail(GEMM_ROWS, A))
    acts = g.out("actions", (n,), "int32", tail(GEMM_ROWS, 1))
    nt = -(-n // GEMM_ROWS)
    tickets = g.out("tickets", (nt,), "int32", tail(1, 1), init=torch.zeros(nt, dtype=torch.int32, device="cuda"))
    _call("hb_actor_act", _p(bits if packed else obs8), 1 if packed else 0, _p(legal), n, obs_len, _p(w1t), kp, _p(b1f), hidden, _p(h),
          _p(w2t), _p(b2f), _p(sup_d), A, K51, _p(q), 0.25, 8, (1 << 33) | 5, 77, _p(acts), _p(tickets))


def _policy_act_grid():
    out = []
    for i, (A, K, pad) in enumerate(((20, 51, 4), (11, 51, 0), (48, 51, 5), (64, 64, 3))):
        gpw = 64 // A                                           # policy_kernel: a wavefront owns 64 / A games, four per workgroup
        for j, n in enumerate(sorted(set(edge_sizes(gpw, 4 * gpw) + [4 * gpw - 1]))):
            out.append((A, K, pad, n, list(CODE)[(i + j) % 3]))      # every dtype at every A, cycling over the sizes
    return out


@case("hb_policy_act", _policy_act_grid())
def policy_act(g, A, K, pad, n, dtype):
    import test_actor_kernels_f64 as TA

    rng = np.random.default_rng(A * K + pad + n)
    AK, rs = A * K, A * K + pad
    lg = np.full((n, rs), np.nan)
    lg[:, :AK] = rng.standard_normal((n, AK)) * 2
    lg_d = g.inp("logits", TA._dev(lg, dtype)[0])
    sup_d = g.inp("support", _cuda(np.linspace(-25.0, 25.0, K).astype(np.float32)))
    legal = g.inp("legal", _cuda(TA._legal_cases(n, A, rng)))
    T = 4 * (64 // A)
    q = g.out("q", (n, A), "float32", tail(T, A))
    acts = g.out("actions", (n,), "int32", tail(T, 1))
    _call("hb_policy_act", _p(lg_d), CODE[dtype], _p(legal), _p(sup_d), n, A, K, rs, 0.25, (1 << 33) | 4, (1 << 32) | 1, (1 << 32) - 5,
          _p(acts), _p(q))


# =================================================================================================================================
# Replay
# =================================================================================================================================
def _rings(g, cap, row, odt, A, row_tail):
    """The six rings as guarded in/out arguments that start as fill bytes (a slot nobody writes keeps them)."""
    return dict(obs_tm1=g.out("ring_obs_tm1", (cap, row), odt, row_tail), obs_t=g.out("ring_obs_t", (cap, row), odt, row_tail),
                act=g.out("ring_act", (cap, 1), "int8", tail(LANE_ROWS, 1)), lms=g.out("ring_lms", (cap, A), "int8", tail(LANE_ROWS, CHUNK)),
                rew=g.out("ring_rew", (cap, 1), "float32", tail(LANE_ROWS, 1)), term=g.out("ring_term", (cap, 1), "uint8", tail(LANE_ROWS, 1)))


# replay_insert_kernel: grid-stride over the 16-byte chunks of a segment, 256 per workgroup. Beside the shapes of
# replay_cases.INSERT_CASES (by name): 255 and 257 chunks in one segment, and in the second segment of a wrapping insert
# (name, capacity, rows, row length, A, start, packed)
INSERT_EDGES = {"chunks_255": ("chunks_255", 300, 255, 16, 20, 3, False), "chunks_257": ("chunks_257", 300, 257, 16, 11, 0, False),
                "wrap_chunks_255": ("wrap_chunks_255", 300, 260, 16, 20, 295, False),
                "wrap_chunks_257": ("wrap_chunks_257", 300, 260, 16, 11, 297, False),
                "packed_chunks_257": ("packed_chunks_257", 300, 257, 100, 20, 1, True)}     # 4 words = 16 bytes per row


@case("hb_replay_insert", [("bytes_not_x16",), ("wrap_unaligned_2nd_segment",), ("n_eq_cap_from_0",), ("n_eq_cap_wrapping",),
                           ("start_last_slot",), ("one_row_L658",), ("one_row_L1",), ("under_16_bytes",), ("grid_cap",),
                           ("packed_rows",)] + [(k,) for k in INSERT_EDGES])
def replay_insert(g, name):
    import replay_cases as RC

    ic = RC.InsertCase(*INSERT_EDGES[name]) if name in INSERT_EDGES else {c.name: c for c in RC.INSERT_CASES}[name]
    rng = np.random.default_rng(ic.cap * 31 + ic.start)
    form = (lambda a: RC.pack_rows(a, ic.L)) if ic.packed else (lambda a: a)
    first = RC.make_rows(rng, ic.n, ic.L, ic.A)[0]
    obs, legal, action, reward = RC.make_rows(rng, ic.n, ic.L, ic.A)
    st = rng.integers(0, 3, ic.n).astype(np.int8)
    row, odt = (RC.words_for(ic.L), "int32") if ic.packed else (ic.L, "int8")
    row_bytes = 4 * row if ic.packed else ic.L
    # replay_insert_kernel: grid-stride over 16-byte chunks, 256 lanes per workgroup
    row_tail = tail(LANE_ROWS, CHUNK // (4 if ic.packed else 1))
    last = g.out("last_obs", (ic.n, row), odt, row_tail, init=_cuda(form(first)))
    ins = [g.inp(nm, _cuda(a)) for nm, a in (("obs", form(obs)), ("legal", legal), ("actions", action), ("rewards", reward),
                                             ("step_type", st))]
    r = _rings(g, ic.cap, row, odt, ic.A, row_tail)
    _call("hb_replay_insert", _p(last), *(_p(t) for t in ins), _p(r["obs_tm1"]), _p(r["obs_t"]), _p(r["act"]), _p(r["lms"]),
          _p(r["rew"]), _p(r["term"]), ic.n, row_bytes, ic.A, ic.cap, ic.start)


DT3 = {"f32": "float32", "bf16": "bfloat16", "f16": "float16"}


def _gather_outs(g, B, x_ld, dname):
    # gather_kernel / per_sample_gather_kernel: one workgroup per x row (2 B workgroups), so one row of x_ld elements is a tile
    x = g.out("x", (2 * B, x_ld), DT3[dname], tail(BLOCK_ROW, x_ld))
    act = g.out("act", (B,), "int32", tail(BLOCK_ROW, 1))
    rew, term, disc = (g.out(nm, (B,), "float32", tail(BLOCK_ROW, 1)) for nm in ("rew", "term", "disc"))
    return x, act, rew, term, disc


def _ring_inputs(g, ring):
    for nm in ("obs_tm1", "obs_t", "act", "rew", "term"):
        g.inp("ring_" + nm, getattr(ring, nm))


# (case of replay_cases.CASES, ring state, n_step): int8 and packed rings, B 1 / 5 / 64, x_ld > L, a wrapped ring
GATHER = [("m40_i8_L658_pad", 7, 3), ("m40_i8_L33", 3, 1), ("o37_i8_L171", 8, 2), ("e8_i8_L1", 2, 1), ("h16_i8_L31_any", 3, 5),
          ("m40_pk_L658", 7, 3), ("o37_pk_L171", 20, 1), ("o37_pk_L33", 8, 2), ("e8_pk_L31", 3, 1), ("h16_pk_L32", 7, 5)]


@case("hb_replay_gather_packed", [c for c in GATHER if "_pk_" in c[0]])
@case("hb_replay_gather", [c for c in GATHER if "_i8_" in c[0]])
def replay_gather(g, name, state, n_step):
    import torch

    import replay_cases as RC
    import test_replay_kernels_oracle as TR

    rc = RC.BY_NAME[name]
    ring, orc = TR._filled(rc, state)
    _ring_inputs(g, ring)
    size_wp = g.inp("size_wp", torch.tensor([orc.size, orc.write_pointer], dtype=torch.int64, device="cuda"))
    idx = g.inp("idx", _cuda(RC.index_batches(rc, orc.size, state)[0]))
    B, dname = rc.B, rc.dtypes[0]
    x, act, rew, term, disc = _gather_outs(g, B, rc.x_ld, dname)
    _call("hb_replay_gather_packed" if rc.packed else "hb_replay_gather", _p(ring.obs_tm1), _p(ring.obs_t), _p(ring.act),
          _p(ring.rew), _p(ring.term), _p(idx), B, rc.L, _p(x), TR.DT[dname], rc.x_ld, _p(act), _p(rew), _p(term), _p(disc), n_step,
          rc.gamma, rc.cap, rc.n_ins, _p(size_wp))


@case("hb_per_sample_gather", [(i,) for i in range(8)])
def per_sample_gather(g, i):
    import torch

    import hanabi_hip
    import replay_cases as RC
    import test_replay_kernels_oracle as TR

    pc = RC.PSG_CASES[i]
    rc = RC.BY_NAME[pc.case]
    ring, orc = TR._filled(rc, pc.state)
    size = orc.size
    tree = hanabi_hip.SumTree(rc.cap)
    lazy = pc.lazy[-1]
    if lazy:
        tree.set_lazy_top(True)
    tree.fill_range_dev(0, size, torch.tensor([0.6], device="cuda"))
    p_idx, p_val = RC.psg_priorities(pc, size)
    tree.update_dev(_cuda(p_idx), _cuda(p_val))
    _ring_inputs(g, ring)
    size_wp = g.inp("size_wp", torch.tensor([size, orc.write_pointer], dtype=torch.int64, device="cuda"))
    counter = g.inp("counter", torch.tensor(7.0, dtype=torch.float32, device="cuda"))
    B, dname = pc.B, rc.dtypes[0]
    idx = g.out("idx", (B,), "int64", tail(BLOCK_ROW, 1))
    prob = g.out("prob", (B,), "float64", tail(BLOCK_ROW, 1))
    x, act, rew, term, disc = _gather_outs(g, B, rc.x_ld, dname)
    _call("hb_per_sample_gather", tree.h, pc.seed, _p(counter), B, _p(idx), _p(prob), _p(ring.obs_tm1), _p(ring.obs_t), _p(ring.act),
          _p(ring.rew), _p(ring.term), rc.L, 1 if rc.packed else 0, _p(x), TR.DT[dname], rc.x_ld, _p(act), _p(rew), _p(term),
          _p(disc), pc.n_step, rc.gamma, rc.cap, rc.n_ins, _p(size_wp))
    if lazy:
        tree.set_lazy_top(False)


# obl_insert_kernel: grid-stride over 16-byte chunks, 256 lanes per workgroup; n 1 / 63 / 65 wrap around a 96-slot ring
@case("hb_obl_insert", [(n, steps, rb) for n, steps, rb in ((1, 1, 24), (63, 2, 84), (65, 5, 171), (65, 3, 658), (1, 5, 171),
                                                           (63, 3, 24))])
def obl_insert(g, n, n_steps, row_bytes):
    cap, A = 96, 20 if row_bytes != 171 else 11
    start = cap - n // 2 - 1
    rng = np.random.default_rng(1000 * n_steps + row_bytes + n)
    term = (rng.random((n_steps, n)) < 0.3).astype(np.int8) * rng.integers(1, 3, (n_steps, n)).astype(np.int8)
    host = [("obs_tm1", rng.integers(-128, 128, (n, row_bytes)).astype(np.int8)), ("actions", rng.integers(0, A, n).astype(np.int32)),
            ("rewards", rng.integers(-3, 4, (n_steps, n)).astype(np.float32) + rng.random((n_steps, n)).astype(np.float32)),
            ("terminal", term), ("obs_t", rng.integers(-128, 128, (n, row_bytes)).astype(np.int8)),
            ("legal_t", rng.integers(0, 2, (n, A)).astype(np.int8))]
    ins = [g.inp(nm, _cuda(a)) for nm, a in host]
    r = _rings(g, cap, row_bytes, "int8", A, tail(LANE_ROWS, CHUNK))
    _call("hb_obl_insert", *(_p(t) for t in ins), _p(r["obs_tm1"]), _p(r["obs_t"]), _p(r["act"]), _p(r["lms"]), _p(r["rew"]),
          _p(r["term"]), n, n_steps, row_bytes, A, cap, start)


# =================================================================================================================================
# Sum tree (caller-owned outputs)
# =================================================================================================================================
def _tree(cap, lazy=False, n_prio=None):
    import hanabi_hip

    tree = hanabi_hip.SumTree(cap)
    if lazy:
        tree.set_lazy_top(True)
    rng = np.random.default_rng(cap)
    k = n_prio or cap
    idx = np.sort(rng.permutation(tree.capacity)[:k]).astype(np.int64)
    tree.update_dev(_cuda(idx), _cuda((rng.random(k) ** 2 + 0.01).astype(np.float32)))
    return tree


@case("hb_tree_sample", [(cap, n, wv) for cap in (64, 2048) for n in edge_sizes(WAVE_ROWS) + [64] for wv in (True, False)])
def tree_sample(g, cap, n, with_val):
    tree = _tree(cap, n_prio=min(cap, 200))
    q = g.inp("quantiles", _cuda(np.random.default_rng(n).random(n).astype(np.float32)))
    idx = g.out("idx", (n,), "int64", tail(WAVE_ROWS, 1))
    val = g.out("val", (n,), "float32", tail(WAVE_ROWS, 1)) if with_val else None
    _call("hb_tree_sample", tree.h, _p(q), _p(idx), _p(val), n)


@case("hb_tree_get", [(cap, n) for cap in (64, 2048) for n in edge_sizes(LANE_ROWS)])
def tree_get(g, cap, n):
    tree = _tree(cap)
    idx = g.inp("idx", _cuda(np.random.default_rng(n).integers(0, cap, n).astype(np.int64)))
    val = g.out("val", (n,), "float32", tail(LANE_ROWS, 1))
    _call("hb_tree_get", tree.h, _p(idx), _p(val), n)


@case("hb_tree_total", [(64, False), (2048, False), (2048, True)])
def tree_total(g, cap, lazy):
    tree = _tree(cap, lazy=lazy, n_prio=200)
    total = g.out("total", (1,), "float32", tail(1, 1))
    _call("hb_tree_total", tree.h, _p(total))


@case("hb_tree_export_nodes", [(2, False), (64, False), (2048, False), (2048, True)])
def tree_export_nodes(g, cap, lazy):
    tree = _tree(cap, lazy=lazy, n_prio=min(cap, 200))
    nodes = g.out("nodes", (2 * tree.capacity,), "float32", tail(LANE_ROWS, 4))    # a device-to-device copy of 2 * cap floats
    _call("hb_tree_export_nodes", tree.h, _p(nodes))


PER_GRID = [(cap, B) for cap in (64, 2048) for B in edge_sizes(WAVE_ROWS) + [64]]


@case("hb_per_sample", [p + (u,) for p in PER_GRID for u in (0, 1)])
def per_sample(g, cap, B, unit):
    tree = _tree(cap, lazy=cap > 1024, n_prio=min(cap, 200))
    u = np.random.default_rng(B).random(B) / (1 if unit else B)
    u_d = g.inp("u", _cuda(u))
    idx = g.out("idx", (B,), "int64", tail(WAVE_ROWS, 1))
    prob = g.out("prob", (B,), "float64", tail(WAVE_ROWS, 1))
    _call("hb_per_sample", tree.h, _p(u_d), B, unit, _p(idx), _p(prob))


@case("hb_per_sample_philox", PER_GRID)
def per_sample_philox(g, cap, B):
    import torch

    tree = _tree(cap, n_prio=min(cap, 200))
    counter = g.inp("counter", torch.tensor(3.0, dtype=torch.float32, device="cuda"))
    idx = g.out("idx", (B,), "int64", tail(WAVE_ROWS, 1))
    prob = g.out("prob", (B,), "float64", tail(WAVE_ROWS, 1))
    K = _K()
    K.check(K.lib().hb_per_sample_philox(tree.h, 0x1234ABCD5, _p(counter), B, _p(idx), _p(prob), K.current_stream()))


# the three update paths: < 96 entries (one workgroup), 96 .. 1024 (per 1024-leaf subtree), more (stamp + scatter)
@case("hb_per_update", [(64, 1), (64, 24), (4096, 120), (4096, 1100)])
def per_update(g, cap, n):
    import torch

    tree = _tree(cap, n_prio=min(cap, 200))
    rng = np.random.default_rng(cap + n)
    idx = g.inp("idx", _cuda(rng.permutation(cap)[:n].astype(np.int64)))
    td = g.inp("td", _cuda((rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 3, n)).astype(np.float32)))
    mx = g.out("max_prio", (1,), "float32", tail(1, 1), init=torch.zeros(1, device="cuda"))
    mn = g.out("min_prio", (1,), "float32", tail(1, 1), init=torch.full((1,), float("inf"), device="cuda"))
    K = _K()
    K.check(K.lib().hb_per_update(tree.h, _p(idx), _p(td), n, 0.6, _p(mx), _p(mn), K.current_stream()))
    # the leaves it wrote, through a caller-owned buffer
    got = g.out("leaves", (n,), "float32", tail(LANE_ROWS, 1))
    _call("hb_tree_get", tree.h, _p(idx), _p(got), n)


# =================================================================================================================================
# Learner
# =================================================================================================================================
LOSS_B = (1, 63, 65)
LOSS_SHAPES = ((20, 51), (48, 51), (20, 51), (11, 51), (5, 21))      # (actions, atoms), cycling over batch size x dtype
LOSS_GRID = [(B, dt, LOSS_SHAPES[(3 * i + j) % 5]) for i, B in enumerate(LOSS_B) for j, dt in enumerate(CODE)]


def _c51_inputs(g, B, dtype, A, K, with_bias, pad):
    import torch

    import test_learner_kernels_f64 as TL

    seed = 1000 * A + 10 * K + B
    rng = np.random.default_rng(seed + 7)
    bias_on = bo_d = bt_d = None
    if with_bias:
        bo = rng.standard_normal(A * K) * 0.5
        lo, hi = (0, 1) if A == 2 else (1, A - 1)
        bo[hi * K:(hi + 1) * K] = bo[lo * K:(lo + 1) * K]          # _c51_batch's exact selector tie stays a tie with the bias added
        bo_d, bias_on = TL._dev(bo, dtype)
        bt_d, _ = TL._dev(rng.standard_normal(A * K) * 0.5, dtype)
        g.inp("bias_online", bo_d)
        g.inp("bias_target", bt_d)
    d = TL._c51_batch(B, A, K, dtype, seed, bias_on, pad)
    f32 = lambda x: torch.as_tensor(np.asarray(x, np.float32)).cuda()
    t = dict(on=d["on_d"], tg=d["tg_d"], act=_cuda(d["act"].astype(np.int32)), rew=f32(d["rew"]), term=f32(d["term"]),
             prios=_cuda(d["prios"]), beta=f32([0.4]), disc=f32(d["disc"]), support=f32(d["support"]))
    for nm, x in t.items():
        g.inp(nm, x)
    args = (_p(t["on"]), _p(t["tg"]), CODE[dtype], _p(t["act"]), _p(t["rew"]), _p(t["term"]), _p(t["prios"]), _p(t["beta"]),
            _p(t["disc"]), 1, _p(t["support"]), B, A, K, d["rs"])
    return d, args, bo_d, bt_d


@case("hb_c51_loss_grad", [p + (i % 2 == 0,) for i, p in enumerate(LOSS_GRID)])
def c51_loss_grad(g, B, dtype, AK, with_bias):
    import torch

    A, K = AK
    d, args, bo, bt = _c51_inputs(g, B, dtype, A, K, with_bias, pad=True)
    # c51_kernel: one wavefront per sample, four per workgroup
    td = g.out("td", (B,), "float32", tail(WAVE_ROWS, 1))
    w = g.out("w", (B,), "float32", tail(WAVE_ROWS, 1))
    dlog = g.out("dlogits", (B, d["rs"]), dtype, tail(WAVE_ROWS, d["rs"]))
    cnt = g.out("update_counter", (1,), "float32", tail(1, 1), init=torch.full((1,), 5.0, device="cuda"))
    _call("hb_c51_loss_grad", *args, _p(td), _p(w), _p(dlog), _p(cnt), _p(bo), _p(bt))


@case("hb_c51_loss_sparse", [p + (i % 2 == 1,) for i, p in enumerate(LOSS_GRID)])
def c51_loss_sparse(g, B, dtype, AK, with_bias):
    import torch

    A, K = AK
    d, args, bo, bt = _c51_inputs(g, B, dtype, A, K, with_bias, pad=B != 63)
    # c51_sparse_kernel: one 64-lane workgroup per sample
    td = g.out("td", (B,), "float32", tail(BLOCK_ROW, 1))
    w = g.out("w", (B,), "float32", tail(BLOCK_ROW, 1))
    dl = g.out("dl", (B, 64), "float32", tail(BLOCK_ROW, 64))
    cnt = g.out("update_counter", (1,), "float32", tail(1, 1), init=torch.full((1,), 5.0, device="cuda")) if with_bias else None
    _call("hb_c51_loss_sparse", *args, _p(td), _p(w), _p(dl), _p(cnt), _p(bo), _p(bt))


# dqn_loss_kernel: ONE 256-lane workgroup strides over the batch
@case("hb_dqn_loss_sparse", [(B, dt, (i + j) % 2 + 1) for i, B in enumerate(LOSS_B + (255, 256)) for j, dt in enumerate(CODE)])
def dqn_loss_sparse(g, B, dtype, cs):
    import torch

    import test_learner_kernels_f64 as TL

    A = 11 if cs == 1 else 20
    rs = (A - 1) * cs + 1 + 5
    rng = np.random.default_rng(B * 10 + cs)
    on = np.full((2 * B, rs), np.nan)
    tg = np.full((B, rs), np.nan)
    on[:, 0:A * cs:cs] = rng.standard_normal((2 * B, A)) * 2
    tg[:, 0:A * cs:cs] = rng.standard_normal((B, A)) * 2
    f32 = lambda x: torch.as_tensor(np.asarray(x, np.float32)).cuda()
    t = dict(on=TL._dev(on, dtype)[0], tg=TL._dev(tg, dtype)[0], act=_cuda(rng.integers(0, A, B).astype(np.int32)),
             rew=f32(rng.integers(-2, 3, B)), term=f32(rng.random(B) < 0.25), prios=_cuda(10.0 ** rng.uniform(-8, 0, B)),
             beta=f32([0.4]), disc=f32(0.99 ** rng.integers(1, 4, B)))
    for nm, x in t.items():
        g.inp(nm, x)
    td = g.out("td", (B,), "float32", tail(LANE_ROWS, 1))
    w = g.out("w", (B,), "float32", tail(LANE_ROWS, 1))
    dl = g.out("dl", (B, 64), "float32", tail(LANE_ROWS, 64))
    _call("hb_dqn_loss_sparse", _p(t["on"]), _p(t["tg"]), CODE[dtype], _p(t["act"]), _p(t["rew"]), _p(t["term"]), _p(t["prios"]),
          _p(t["beta"]), _p(t["disc"]), B, A, cs, rs, _p(td), _p(w), _p(dl), None, None)


BWD_SHAPES = ((512, 20, 51), (100, 11, 51), (40, 5, 21))              # (hidden, actions, atoms)


@case("hb_c51_backward", [(B, dt) + BWD_SHAPES[(i + j) % 3] for i, B in enumerate(LOSS_B) for j, dt in enumerate(CODE)])
def c51_backward(g, B, dtype, hidden, A, K):
    import test_learner_kernels_f64 as TL

    AK = A * K
    rng = np.random.default_rng(hidden * 1000 + AK + B)
    h_ld = hidden + (3 if B == 63 else 0)
    w2_ld, dw2_ld = AK + 5, AK + 7
    dl = np.zeros((B, 64))
    dl[:, :K] = rng.standard_normal((B, K)) * 1e-3
    hm = np.full((B, h_ld), np.nan)
    hm[:, :hidden] = np.maximum(rng.standard_normal((B, hidden)), 0.0)
    w2 = np.full((hidden, w2_ld), np.nan)
    w2[:, :AK] = rng.standard_normal((hidden, AK)) * 0.05
    dl_d = g.inp("dl", _cuda(dl.astype(np.float32)))
    act_d = g.inp("act", _cuda(rng.integers(0, A, B).astype(np.int32)))
    h_d = g.inp("hidden", TL._dev(hm, dtype)[0])
    w2_d = g.inp("w2", TL._dev(w2, dtype)[0])
    # c51_backward_kernel: a workgroup writes a tile of dH rows or a slab of dW2 rows (at most 8 hidden units: JT <= 8); the
    # guards are a whole batch of dH and 8 rows of dW2
    dh = g.out("dh", (B, hidden), dtype, tail(B, hidden))
    db1 = g.out("db1", (hidden,), "float32", tail(1, hidden))
    dw2 = g.out("dw2", (hidden, dw2_ld), dtype, tail(8, dw2_ld))
    db2 = g.out("db2", (AK,), "float32", tail(1, AK))
    _call("hb_c51_backward", _p(dl_d), _p(act_d), _p(h_d), h_ld, _p(w2_d), w2_ld, CODE[dtype], B, hidden, A, K, _p(dh), _p(db1),
          _p(dw2), dw2_ld, _p(db2))


# 16 row lanes per workgroup: rows 1, 15, 17, and 1 025 (more than one pass of the 1 024 threads)
COLSUM_GRID = [(rows, cols, list(CODE)[(i + j) % 3]) for j, cols in enumerate(edge_sizes(COLSUM_COLS))
               for i, rows in enumerate((1, 15, 17, 1025))]


@case("hb_colsum", COLSUM_GRID)
def colsum(g, rows, cols, dtype):
    import test_learner_kernels_f64 as TL

    x = g.inp("x", TL._dev(np.random.default_rng(rows * 7 + cols).standard_normal((rows, cols)), dtype)[0])
    out = g.out("out", (cols,), "float32", tail(1, COLSUM_COLS))
    _call("hb_colsum", _p(x), CODE[dtype], rows, cols, _p(out))


@case("hb_relu_bwd_colsum", COLSUM_GRID)
def relu_bwd_colsum(g, rows, cols, dtype):
    import test_learner_kernels_f64 as TL

    rng = np.random.default_rng(rows * 7 + cols)
    x = TL._dev(rng.standard_normal((rows, cols)), dtype)[0]
    act = rng.standard_normal((rows, cols + 3))
    sel = rng.random((rows, cols)) < 0.3
    act[:, :cols][sel] = np.where(rng.random(sel.sum()) < 0.5, 0.0, -0.0)
    act_d = g.inp("act", TL._dev(act, dtype)[0])
    # relu_bwd_colsum_kernel: 16 row lanes x 64 columns per pass of a workgroup; dy is masked in place
    dy = g.out("dy", (rows, cols), dtype, tail(16, cols), init=x)
    out = g.out("out", (cols,), "float32", tail(1, COLSUM_COLS))
    _call("hb_relu_bwd_colsum", _p(dy), _p(act_d), cols + 3, CODE[dtype], rows, cols, _p(out))


@case("hb_thin_gemm", [(32, 16, 32, 1, "bfloat16", False, True, True), (64, 48, 64, 2, "float16", True, False, True),
                       (32, 48, 96, 2, "float16", False, True, False), (96, 16, 32, 1, "bfloat16", True, True, True)])
def thin_gemm(g, m, n, k, batch, dtype, out32, relu, with_bias):
    import test_learner_kernels_f64 as TL

    rng = np.random.default_rng(m + n + k)
    ldx, ldw, ldo = k + 8, k + 16, n + 4
    x = np.full((batch, m, ldx), np.nan)
    x[:, :, :k] = rng.standard_normal((batch, m, k)) * 0.5
    wt = np.full((batch, n, ldw), np.nan)
    wt[:, :, :k] = rng.standard_normal((batch, n, k)) * (1.0 / np.sqrt(k))
    x_d = g.inp("x", TL._dev(x, dtype)[0])
    w_d = g.inp("wt", TL._dev(wt, dtype)[0])
    b_d = g.inp("bias", TL._dev(rng.standard_normal((batch, n)) * 0.3, dtype)[0]) if with_bias else None
    out = g.out("out", (batch, m, ldo), "float32" if out32 else dtype, tail(THIN_ROWS, ldo))
    flags = (1 if relu else 0) | (2 if out32 else 0) | (4 if dtype == "float16" else 0)
    _call("hb_thin_gemm", _p(x_d), _p(w_d), _p(b_d), _p(out), m, n, k, ldx, ldw, ldo, batch, m * ldx, n * ldw, m * ldo, flags)


@case("hb_thin_forward", [(1, 32, 64, 32, 0, 0, "float16", False, False), (1, 64, 96, 96, 0, 0, "bfloat16", False, True),
                          (1, 64, 128, 96, 0, 0, "bfloat16", True, True),
                          (2, 32, 16, 32, 1, 1, "bfloat16", True, True), (2, 64, 16, 96, 2, 16, "bfloat16", True, True),
                          (2, 32, 16, 96, 30, 7, "float16", True, True), (2, 224, 16, 64, 3, 17, "bfloat16", True, True),
                          (2, 32, 16, 32, 30, 7, "bfloat16", False, False), (2, 64, 64, 64, 5, 33, "float16", True, True)])
def thin_forward(g, layer, B, n_round, k, A, K, dtype, out32, with_bias):
    """layer 1: n = n_round; layer 2: n = A K rounded up to a multiple of n_round. Strides carry padding columns."""
    import test_learner_kernels_f64 as TL

    rng = np.random.default_rng(layer * 1000 + B + k + A)
    n = n_round if layer == 1 else -(-A * K // n_round) * n_round
    entries = 1 if layer == 1 else 2
    ldx, ldw, ldo = k + 8, k + 16, n + 4
    x = np.full((entries, 2 * B, ldx), np.nan)
    x[:, :, :k] = rng.standard_normal((entries, 2 * B, k)) * 0.5
    if layer == 2:
        x[1, :B] = np.nan                    # the target network on obs_tm1: nobody may read it
    wt = np.full((entries, n, ldw), np.nan)
    wt[:, :, :k] = rng.standard_normal((entries, n, k)) * (1.0 / np.sqrt(k))
    x_d = g.inp("x", TL._dev(x, dtype)[0])
    w_d = g.inp("wt", TL._dev(wt, dtype)[0])
    b_d = g.inp("bias", TL._dev(rng.standard_normal((entries, n)) * 0.3, dtype)[0]) if with_bias else None
    act = None
    if layer == 2:
        a = rng.integers(0, A, B).astype(np.int32)
        a[::9] = -1                          # selects nothing
        act = g.inp("act", _cuda(a))
    out = g.out("out", (entries, 2 * B, ldo), "float32" if out32 else dtype, tail(THIN_ROWS, ldo))
    flags = (1 if layer == 1 else 0) | (2 if out32 else 0) | (4 if dtype == "float16" else 0)
    _call("hb_thin_forward", layer, _p(x_d), _p(w_d), _p(b_d), _p(out), _p(act), B, n, k, ldx, ldw, ldo, 2 * B * ldx,
          n * ldw, 2 * B * ldo, A, K, flags)


B1, B2, LR, EPS = (float(np.float32(x)) for x in (0.9, 0.999, 1e-3, 3.125e-5))


def _adam_tensor(g, tag, rng, rows, cols, grad_dtype, eff_dtype, shared, grad_pad, tile_elems):
    """test_learner_kernels_f64._AdamTensor with its weights, moments and merged tensor re-homed into guarded in/out buffers
    (eff rows are eff_ld = cols + 4 elements apart). tile_elems: the elements one workgroup of the kernel covers."""
    import test_learner_kernels_f64 as TL

    T = TL._AdamTensor(rng, rows, cols, grad_dtype, eff_dtype, shared, grad_pad=grad_pad)
    t_el = tail(1, tile_elems)
    T.p = [g.out(f"{tag}.{nm}", (rows, cols), "float32", t_el, init=t) for nm, t in zip(("w", "w_mu", "w_sigma"), T.p)]
    names = ("m_w", "v_w", "m_mu", "v_mu", "m_sigma", "v_sigma")
    mom = []
    for i, (nm, t) in enumerate(zip(names, T.mom)):
        mom.append(mom[i - 2] if shared and i in (2, 3) else g.out(f"{tag}.{nm}", (rows, cols), "float32", t_el, init=t))
    T.mom = mom
    T.eff = g.out(f"{tag}.eff", (rows, T.eff_ld), eff_dtype, tail(1, tile_elems) + 4 * rows, init=T.eff)
    g.inp(f"{tag}.noise", T.noise)
    g.inp(f"{tag}.grad", T.grad)
    return T


# noisy_adam_kernel: one element per lane, 256 per workgroup
@case("hb_noisy_adam", [(r, c, dt, sh) for (r, c) in ((7, 5), (40, 68), (1, 255), (1, 257)) for dt, sh in (("float32", False),
                                                                                                      ("bfloat16", True), ("float16", False))])
def noisy_adam(g, rows, cols, eff_dtype, shared):
    import torch

    rng = np.random.default_rng(rows + cols + int(shared))
    T = _adam_tensor(g, "t0", rng, rows, cols, "float32", eff_dtype, shared, 0, LANE_ROWS)
    step = g.inp("step", torch.tensor([1.0], device="cuda"))
    p, m = T.p, T.mom
    _call("hb_noisy_adam", _p(p[0]), _p(p[1]), _p(p[2]), _p(T.noise), _p(T.grad), _p(m[0]), _p(m[1]), _p(m[2]), _p(m[3]), _p(m[4]),
          _p(m[5]), _p(step), _p(T.eff), CODE[eff_dtype], rows * cols, cols, T.eff_ld, LR, B1, B2, EPS)


ADAM_SETS = {"one": [(24, 36)], "eight": [(8, 4), (3, 64), (17, 12), (1, 128), (40, 68), (2, 8), (5, 4), (9, 100)],
             "odd": [(8, 4), (3, 64), (17, 12), (1, 126), (40, 68), (2, 8), (5, 4), (9, 7)], "edge": [(1, 1020), (1, 1028), (1, 4)]}


class _env_var:
    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = os.environ.get(self.name)
        if self.value is None:
            os.environ.pop(self.name, None)
        else:
            os.environ[self.name] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop(self.name, None)
        else:
            os.environ[self.name] = self.old


# width: HB_ADAM_WIDTH (None = 4 elements per lane, "2", "1" = the scalar kernel); the "odd" set takes the scalar kernel anyway.
# noisy_adam_multiw_kernel: width elements per lane, 256 lanes per workgroup
@case("hb_noisy_adam_multi", [(s, w, gd, ed, sh) for s, w in (("one", None), ("eight", None), ("eight", "2"), ("eight", "1"), ("odd", None),
                                                             ("edge", None), ("edge", "2"), ("edge", "1"))
                              for gd, ed, sh in (("float32", "bfloat16", False), ("bfloat16", "float32", True), ("float16", "float16", False))])
def noisy_adam_multi(g, set_name, width, grad_dtype, eff_dtype, shared):
    import torch

    shapes = ADAM_SETS[set_name]
    rng = np.random.default_rng(len(shapes) + int(shared))
    ts = [_adam_tensor(g, f"t{i}", rng, r, c, grad_dtype, eff_dtype, shared, 4, LANE_ROWS * 4) for i, (r, c) in enumerate(shapes)]
    K = _K()
    tab = (K.HbAdamTensor * len(ts))()
    for i, T in enumerate(ts):
        T.table_entry(tab[i])
    step = g.inp("step", torch.tensor([2.0], device="cuda"))
    with _env_var("HB_ADAM_WIDTH", width):
        _call("hb_noisy_adam_multi", tab, len(ts), _p(step), 0.0, CODE[eff_dtype], LR, B1, B2, EPS)


# noisy_adam_pack_kernel: 8 rows x 128 columns per workgroup for a weight tensor, four elements per lane for a bias
@case("hb_noisy_adam_multi_pack", [(r, c, bc, gd, ed, sh) for (r, c, bc) in ((37, 136, 68), (7, 128, 4), (9, 132, 1028))
                                   for gd, ed, sh in (("float32", "bfloat16", False), ("bfloat16", "float16", True))])
def noisy_adam_multi_pack(g, rows, cols, bias_cols, grad_dtype, eff_dtype, shared):
    import torch

    rng = np.random.default_rng(rows + cols + int(shared))
    wt_t = _adam_tensor(g, "weight", rng, rows, cols, grad_dtype, eff_dtype, shared, 4, ADAM_PACK_ROWS * (cols + 4))
    bias_t = _adam_tensor(g, "bias", rng, 1, bias_cols, grad_dtype, eff_dtype, shared, 4, LANE_ROWS * 4)
    K = _K()
    tab, packs = (K.HbAdamTensor * 2)(), (K.HbAdamPack * 2)()
    wt_t.table_entry(tab[0])
    bias_t.table_entry(tab[1])
    wt_ld = (rows + 7) // 8 * 8 + 8
    # the transposed copy [cols][wt_ld]: a workgroup writes 128 of its rows, 8 elements (one 8-row group) in each
    wt = g.out("wt", (cols, wt_ld), eff_dtype, tail(128, wt_ld))
    bf32 = g.out("bias_f32", (bias_cols,), "float32", tail(LANE_ROWS, 4))
    packs[0].wt, packs[0].wt_ld = wt.data_ptr(), wt_ld
    packs[1].bias_f32 = bf32.data_ptr()
    step = g.inp("step", torch.tensor([2.0], device="cuda"))
    _call("hb_noisy_adam_multi_pack", C.cast(tab, C.c_void_p), C.cast(packs, C.c_void_p), 2, _p(step), 0.0, CODE[eff_dtype], LR, B1, B2,
          EPS)


# The learner's own call: W1, b1, W2, b2 of the one-hidden-layer network with every copy the forward kernels read — the
# transposed copies and the one-kernel actor's fragment-major copies (frag_kind 1 / 2, the output layer's through col_map).
# Entries of the fragment copies and of b2f that no weight maps to are not written: in/out arguments that start as zeros.
@case("hb_noisy_adam_multi_pack", [(L, 20, gd, ed, "net") for L, gd, ed in ((171, "bfloat16", "bfloat16"), (33, "float32", "float16"))])
def noisy_adam_multi_pack_network(g, obs_len, A, grad_dtype, eff_dtype, _tag):
    import torch

    K = _K()
    AK = A * K51
    rng = np.random.default_rng(obs_len + A)
    ts = [_adam_tensor(g, "W1", rng, obs_len, HID, grad_dtype, eff_dtype, True, 4, ADAM_PACK_ROWS * (HID + 4)),
          _adam_tensor(g, "b1", rng, 1, HID, "float32", eff_dtype, True, 4, LANE_ROWS * 4),
          _adam_tensor(g, "W2", rng, HID, AK, grad_dtype, eff_dtype, True, 4, ADAM_PACK_ROWS * (AK + 4)),
          _adam_tensor(g, "b2", rng, 1, AK, "float32", eff_dtype, True, 4, LANE_ROWS * 4)]
    f1, f2, fb = C.c_int64(), C.c_int64(), C.c_int32()
    K.check(K.lib().hb_actor_fused_sizes(obs_len, HID, A, K51, C.byref(f1), C.byref(f2), C.byref(fb)))
    host = (C.c_int32 * AK)()
    K.check(K.lib().hb_actor_fused_columns(A, host))
    col_map = g.inp("col_map", torch.tensor(list(host), dtype=torch.int32, device="cuda"))
    z = lambda n, dt: torch.zeros(n, dtype=dt, device="cuda")
    # a workgroup's 8 x 128 tile of 16-bit weights is 2 048 bytes of a fragment copy; the guards are two of them
    w1f = g.out("w1f", (f1.value,), "uint8", tail(2 * ADAM_PACK_ROWS, 128 * 2), init=z(f1.value, torch.uint8))
    w2f = g.out("w2f", (f2.value,), "uint8", tail(2 * ADAM_PACK_ROWS, 128 * 2), init=z(f2.value, torch.uint8))
    b1f = g.out("b1f", (HID,), "float32", tail(LANE_ROWS, 4))
    b2f = g.out("b2f", (fb.value,), "float32", tail(LANE_ROWS, 4), init=z(fb.value, torch.float32))
    w1t_ld, w2t_ld = (obs_len + 7) // 8 * 8 + 8, HID + 8
    w1t = g.out("w1t", (HID, w1t_ld), eff_dtype, tail(128, w1t_ld))
    w2t = g.out("w2t", (AK, w2t_ld), eff_dtype, tail(128, w2t_ld))
    tab, packs = (K.HbAdamTensor * 4)(), (K.HbAdamPack * 4)()
    for i, T in enumerate(ts):
        T.table_entry(tab[i])
    packs[0].wt, packs[0].wt_ld, packs[0].frag, packs[0].frag_kind = w1t.data_ptr(), w1t_ld, w1f.data_ptr(), 1
    packs[1].bias_f32 = b1f.data_ptr()
    packs[2].wt, packs[2].wt_ld, packs[2].frag, packs[2].frag_kind = w2t.data_ptr(), w2t_ld, w2f.data_ptr(), 2
    packs[2].col_map_dev = col_map.data_ptr()
    packs[3].bias_f32, packs[3].col_map_dev = b2f.data_ptr(), col_map.data_ptr()
    step = g.inp("step", torch.tensor([2.0], device="cuda"))
    _call("hb_noisy_adam_multi_pack", C.cast(tab, C.c_void_p), C.cast(packs, C.c_void_p), 4, _p(step), 0.0, CODE[eff_dtype], LR, B1, B2,
          EPS)


# =================================================================================================================================
# Partners and statistics
# =================================================================================================================================
def _rule_tables(n_sets):
    """(host table of the first set, device tables [n_sets][MAX_RULES], device n_rules [n_sets])"""
    import torch

    from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR

    K = _K()
    agents = [RulebasedAgent(r, seed=11 + i) for i, r in enumerate((PR.piers_rules, PR.iggi_rules, PR.flawed_rules)[:n_sets])]
    tab = (K.HbRule * (K.MAX_RULES * n_sets))()
    for s, a in enumerate(agents):
        for q in range(len(a.rules)):
            tab[s * K.MAX_RULES + q] = a._tab[q]
    rules = torch.frombuffer(bytearray(tab), dtype=torch.uint8).cuda()
    n_rules = torch.tensor([len(a.rules) for a in agents], dtype=torch.int32, device="cuda")
    return agents[0], rules, n_rules


@case("hb_rule_act", [(gk, n, (i + j) % 2 == 0) for i, gk in enumerate(GAMES) for j, n in enumerate(edge_sizes(RULE_ROWS))])
def rule_act(g, game, n, with_fired):
    env = _env(game, n, turns=8)
    rows = g.inp("state_rows", env.export_state())
    agent, _, _ = _rule_tables(1)
    acts = g.out("actions", (n,), "int32", tail(RULE_ROWS, 1))
    fired = g.out("fired", (n,), "int32", tail(RULE_ROWS, 1)) if with_fired else None
    K = _K()
    K.check(K.lib().hb_rule_act(C.byref(env.cfg), _p(rows), n, (1 << 32) - 7, agent._tab, len(agent.rules), 77, 5, _p(acts), _p(fired),
                                K.current_stream()))


# three blocks of block_rows games, the middle one skipped (set -1: nothing of it is written)
@case("hb_rule_act_blocks", [(gk, n, "hb_rule_act_blocks") for gk in ("full2", "small2") for n in edge_sizes(RULE_ROWS)])
@case("hb_rule_act_grouped", [(gk, n, "hb_rule_act_grouped") for gk in ("full2", "full5") for n in edge_sizes(RULE_ROWS)])
def rule_act_grouped(g, game, block_rows, entry):
    import torch

    env = _env(game, 3 * block_rows, turns=8)
    rows = g.inp("state_rows", env.export_state())
    _, rules, n_rules = _rule_tables(3)
    g.inp("rules", rules)
    g.inp("n_rules", n_rules)
    sob = g.inp("set_of_block", torch.tensor([2, -1, 0], dtype=torch.int32, device="cuda"))
    n = 3 * block_rows
    acts = g.out("actions", (n,), "int32", tail(RULE_ROWS, 1))
    fired = g.out("fired", (n,), "int32", tail(RULE_ROWS, 1))
    K = _K()
    K.check(getattr(K.lib(), entry)(C.byref(env.cfg), _p(rows), 3, block_rows, (1 << 32) - 7, _p(sob), _p(rules), _p(n_rules), 3, 77, 5,
                                    _p(acts), _p(fired), K.current_stream()))


def _stepped(game, n, turns=10):
    """An env a few moves in and the move just stepped (its reward / terminal / score are that step's outputs)."""
    env = _env(game, n, turns=turns)
    act = env.random_legal_actions(seed=21, draw=3)
    env.step(act)
    return env, act


def _tally_inputs(g, env, act):
    return [g.inp(nm, t.clone()) for nm, t in (("actions", act), ("reward", env.reward), ("terminal", env.terminal), ("score", env.score))]


# eval_tally_grouped_kernel (hb_eval_tally is its one-block form): one lane per game, 256 per workgroup, grid-stride
@case("hb_eval_tally_grouped", [(gk, n, 3) for gk in ("full2", "small2") for n in edge_sizes(LANE_ROWS)])
@case("hb_eval_tally", [(gk, n, 0) for gk in GAMES for n in edge_sizes(LANE_ROWS)])
def eval_tally(g, game, n, n_blocks):
    import torch

    nb = max(n_blocks, 1)
    env, act = _stepped(game, n * nb, turns=30 if "small" in game else 10)
    ins = _tally_inputs(g, env, act)
    K = _K()
    nc = K.lib().hb_eval_counters(C.byref(env.cfg))
    N = n * nb
    done0 = torch.zeros(N, dtype=torch.uint8, device="cuda")
    done0[::5] = 0x80                                            # some games finished earlier: ignored
    done = g.out("done", (N,), "uint8", tail(LANE_ROWS, 1), init=done0)
    # written once, on the turn a game ends: in/out arguments as far as this one turn goes
    final = g.out("final_score", (N,), "int8", tail(LANE_ROWS, 1), init=torch.full((N,), -1, dtype=torch.int8, device="cuda"))
    length = g.out("length", (N,), "int16", tail(LANE_ROWS, 1), init=torch.full((N,), -1, dtype=torch.int16, device="cuda"))
    c0 = torch.zeros(nb, nc, dtype=torch.int64, device="cuda")
    c0[:, 0] = n
    counters = g.out("counters", (nb, nc), "int64", tail(1, nc), init=c0)
    seat = 10 % env.players
    if n_blocks:
        _call("hb_eval_tally_grouped", C.byref(env.cfg), nb, n, seat, 10, *(_p(t) for t in ins), _p(done), _p(final), _p(length),
              _p(counters))
    else:
        _call("hb_eval_tally", C.byref(env.cfg), n, seat, 10, *(_p(t) for t in ins), _p(done), _p(final), _p(length), _p(counters))


# eval_response_grouped_kernel: one lane per game, 256 per workgroup; only the [seat] slab of resp is touched
@case("hb_eval_response_tally_grouped", [(gk, n, 3) for gk in ("full2", "small2") for n in edge_sizes(LANE_ROWS)])
@case("hb_eval_response_tally", [(gk, n, 0) for gk in GAMES for n in edge_sizes(LANE_ROWS)])
def eval_response_tally(g, game, n, n_blocks):
    import torch

    nb = max(n_blocks, 1)
    env, act = _stepped(game, n * nb)
    N, A, P = n * nb, env.num_actions, env.players
    act_d = g.inp("actions", act.clone())
    done0 = torch.zeros(N, dtype=torch.uint8, device="cuda")
    done0[::5] = 0x80
    done = g.inp("done", done0)
    rng = np.random.default_rng(N)
    prev = g.out("prev", (N,), "int32", tail(LANE_ROWS, 1), init=_cuda(rng.integers(-1, A, N).astype(np.int32)))
    resp = g.out("resp", (nb, P, A + 1, A), "int64", tail(1, (A + 1) * A), init=torch.zeros(nb, P, A + 1, A, dtype=torch.int64, device="cuda"))
    seat = 10 % P
    if n_blocks:
        _call("hb_eval_response_tally_grouped", C.byref(env.cfg), nb, n, seat, _p(act_d), _p(done), _p(prev), _p(resp))
    else:
        _call("hb_eval_response_tally", C.byref(env.cfg), n, seat, _p(act_d), _p(done), _p(prev), _p(resp))


@case("hb_train_tally_init", [(gk, n) for gk in GAMES for n in edge_sizes(LANE_ROWS)])
def train_tally_init(g, game, n):
    env = _env(game, n, turns=0 if n == 1 else 3)
    rows = g.inp("state_rows", env.export_state())
    lost = g.out("lost", (n,), "uint8", tail(LANE_ROWS, 1))        # train_tally_init_kernel: one lane per game
    length = g.out("length", (n,), "int16", tail(LANE_ROWS, 1))
    _call("hb_train_tally_init", C.byref(env.cfg), _p(rows), n, _p(lost), _p(length))


# n is a multiple of 128 by contract (tiles of 128 games): 128, 256 and one tile past a 256-lane workgroup
@case("hb_train_tally", [(gk, n) for gk in GAMES for n in (128, 256, 384)])
def train_tally(g, game, n):
    import torch

    env, act = _stepped(game, n, turns=30 if "small" in game else 10)
    ins = _tally_inputs(g, env, act)
    K = _K()
    nc = K.lib().hb_train_counters(C.byref(env.cfg))
    members = 3
    tm = g.inp("tile_member", torch.tensor([2, -1, 0][:n // 128], dtype=torch.int32, device="cuda"))
    rng = np.random.default_rng(n)
    lost = g.out("lost", (n,), "uint8", tail(LANE_ROWS, 1), init=_cuda(rng.choice([0, 1, 0x80], n).astype(np.uint8)))
    length = g.out("length", (n,), "int16", tail(LANE_ROWS, 1), init=_cuda(rng.integers(0, 30, n).astype(np.int16)))
    counters = g.out("counters", (members, nc), "int64", tail(1, nc), init=torch.zeros(members, nc, dtype=torch.int64, device="cuda"))
    _call("hb_train_tally", C.byref(env.cfg), n, 10 % env.players, *(_p(t) for t in ins), _p(tm), members, _p(lost), _p(length),
          _p(counters))


# =================================================================================================================================
# Search and belief (the kernels without guards of their own)
# =================================================================================================================================
BELIEF_GAMES = ("full2", "full5", "small2")
RK = (63, 65)                      # replicas / candidates on both sides of a wavefront's 64 lanes


def _roots(g, game, m, turns=7):
    env = _env(game, m, turns=turns)
    return env, g.inp("src_rows", env.export_state())


def _candidates(g, env, rows, Kn, seat=-1):
    """hb_belief_determinize's candidates of the roots (rows [m * Kn, SW], weights u32 bits in int32), as inputs."""
    from hanabi_hip.search import Determinizer

    import torch

    m = rows.shape[0]
    out = (torch.empty((m * Kn, env.state_words), dtype=torch.int32, device="cuda"), torch.empty((m * Kn,), dtype=torch.int32, device="cuda"))
    det, w = Determinizer(config=env.cfg).sample(rows, seat=seat, replicas=Kn, seed=5, draw=2, out=out)
    return g.inp("det_rows", det), g.inp("weights", w)


def _belief_grid(extra=()):
    out, i = [], 0
    for m in edge_sizes(WAVE_ROWS):
        for r in RK:
            out.append((BELIEF_GAMES[i % 3], m, r) + tuple(e[i % len(e)] for e in extra))
            i += 1
    return out


@case("hb_belief_determinize", _belief_grid(((-1, 0, 1),)))
def belief_determinize(g, game, m, replicas, seat):
    env, rows = _roots(g, game, m)
    SW = env.state_words
    out = g.out("out_rows", (m * replicas, SW), "int32", tail(WAVE_ROWS, SW))
    w = g.out("weight", (m * replicas,), "int32", tail(WAVE_ROWS, 1))
    K = _K()
    K.check(K.lib().hb_belief_determinize(C.byref(env.cfg), _p(rows), m, seat, replicas, (3 << 32) | 5, (1 << 32) | 2, (1 << 32) - 3,
                                          _p(out), _p(w), K.current_stream()))


@case("hb_search_reduce", [(m, (20, 48, 11)[i % 3], r, i % 3 != 1) for i, m in enumerate(edge_sizes(WAVE_ROWS)) for r in RK])
def search_reduce(g, m, A, replicas, with_best):
    rng = np.random.default_rng(m + A + replicas)
    score = g.inp("score", _cuda(rng.integers(0, 26, (m, A, replicas)).astype(np.int8)))
    wt = rng.integers(0, 1 << 20, (m, replicas)).astype(np.int32) * (rng.random((m, replicas)) < 0.8)
    weight = g.inp("weight", _cuda(wt.astype(np.int32)))
    legal = g.inp("legal", _cuda((rng.random((m, A)) < 0.6).astype(np.int8)))
    value = g.out("value", (m, A), "float32", tail(WAVE_ROWS, A))
    wsum = g.out("wsum", (m, A), "int64", tail(WAVE_ROWS, A))
    n_live = g.out("n_live", (m, A), "int32", tail(WAVE_ROWS, A))
    best = g.out("best", (m,), "int32", tail(WAVE_ROWS, 1)) if with_best else None
    _call("hb_search_reduce", _p(score), _p(weight), _p(legal), m, A, replicas, _p(value), _p(wsum), _p(n_live), _p(best))


# search_layout_kernel: one wavefront per SOURCE row (root x replica), which writes its n_cand output rows
@case("hb_search_layout", _belief_grid(((3, 20, 1),)))
def search_layout(g, game, m, replicas, n_cand):
    env, rows = _roots(g, game, m)
    det, w = _candidates(g, env, rows, replicas)
    SW, A = env.state_words, env.num_actions
    rng = np.random.default_rng(m + replicas)
    cand = rng.integers(0, A, (m, n_cand)).astype(np.int32)
    cand[rng.random((m, n_cand)) < 0.3] = -1
    cand_d = g.inp("cand", _cuda(cand))
    filler = g.inp("filler", _cuda(rng.integers(0, A, m).astype(np.int32)))
    n = m * n_cand * replicas
    rows_out = g.out("rows_out", (n, SW), "int32", tail(WAVE_ROWS * n_cand, SW))
    forced = g.out("forced_out", (n,), "int32", tail(WAVE_ROWS * n_cand, 1))
    done = g.out("done_out", (n,), "uint8", tail(WAVE_ROWS * n_cand, 1))
    n_played = g.out("n_played_out", (m,), "int32", tail(WAVE_ROWS, 1))
    _call("hb_search_layout", C.byref(env.cfg), _p(det), _p(w), _p(cand_d), _p(filler), m, n_cand, replicas, _p(rows_out), _p(forced),
          _p(done), _p(n_played))


@case("hb_search_compare", [(m, (3, 20, 64)[i % 3], r) for i, m in enumerate(edge_sizes(WAVE_ROWS)) for r in RK])
def search_compare(g, m, n_cand, replicas):
    rng = np.random.default_rng(m + n_cand + replicas)
    score = g.inp("score", _cuda(rng.integers(0, 26, (m, n_cand, replicas)).astype(np.int8)))
    wt = rng.integers(1, 1 << 20, (m, replicas)) * (rng.random((m, replicas)) < 0.8)
    weight = g.inp("weight", _cuda(wt.astype(np.int32)))
    cand = rng.integers(0, 20, (m, n_cand)).astype(np.int32)
    cand[rng.random((m, n_cand)) < 0.2] = -1
    cand_d = g.inp("cand", _cuda(cand))
    base = g.inp("base_slot", _cuda(rng.integers(-1, n_cand, m).astype(np.int32)))
    diff = g.out("diff", (m, n_cand), "float64", tail(WAVE_ROWS, n_cand))
    se = g.out("se", (m, n_cand), "float64", tail(WAVE_ROWS, n_cand))
    n_pair = g.out("n_pair", (m,), "int32", tail(WAVE_ROWS, 1))
    _call("hb_search_compare", _p(score), _p(weight), _p(cand_d), _p(base), m, n_cand, replicas, _p(diff), _p(se), _p(n_pair))


# belief_splice_alive_kernel: one wavefront per OUTPUT row, four per workgroup
@case("hb_belief_splice_alive", [p + (i % 2 == 0,) for i, p in enumerate(_belief_grid())])
@case("hb_belief_splice", [p + (None,) for p in _belief_grid()])
def belief_splice(g, game, m, n_cand, alive):
    env, rows = _roots(g, game, m)
    seat = 1
    det, _ = _candidates(g, env, rows, n_cand, seat=seat)
    SW = env.state_words
    out = g.out("out_rows", (n_cand, m, SW), "int32", tail(WAVE_ROWS, SW))
    if alive is None:
        _call("hb_belief_splice", C.byref(env.cfg), _p(rows), _p(det), m, seat, n_cand, _p(out))
    else:
        al = g.inp("alive", _cuda(np.random.default_rng(m).integers(0, 32, m).astype(np.uint8))) if alive else None
        _call("hb_belief_splice_alive", C.byref(env.cfg), _p(rows), _p(al), _p(det), m, seat, n_cand, _p(out))


def _select_inputs(g, game, m, n_cand, depth, flat):
    env, rows = _roots(g, game, m)
    det, w = _candidates(g, env, rows, n_cand)
    A = env.num_actions
    rng = np.random.default_rng(m + n_cand + depth)
    actual = rng.integers(0, 3, (depth, m)).astype(np.int32)
    hyp = rng.integers(0, 3, (depth, n_cand, m)).astype(np.int32)
    valid = (rng.random((depth, m)) < 0.8).astype(np.uint8)
    n_legal = rng.integers(0, A + 2, (depth, n_cand, m)).astype(np.int32)
    if flat:
        actual, hyp, valid = actual[0], hyp[0], valid[0]
    t = dict(hyp=g.inp("hyp_moves", _cuda(hyp)), actual=g.inp("actual", _cuda(actual)), valid=g.inp("valid", _cuda(valid)),
             n_legal=g.inp("n_legal", _cuda(n_legal)))
    return env, rows, det, w, t


def _select_outs(g, env, m, replicas, depth, flat):
    SW = env.state_words
    # belief_select_depth_kernel / belief_select_soft_kernel: one wavefront per ROOT, which writes its `replicas` output rows
    o = dict(rows=g.out("out_rows", (m * replicas, SW), "int32", tail(WAVE_ROWS * replicas, SW)),
             w=g.out("out_weight", (m * replicas,), "int32", tail(WAVE_ROWS * replicas, 1)),
             n_surv=g.out("n_surv", (m,) if flat else (depth, m), "int32", tail(WAVE_ROWS, 1)),
             fallback=g.out("fallback", (m,), "uint8", tail(WAVE_ROWS, 1)))
    return o


# (game, m, candidates K, replicas R): K and R on both sides of 64, R above and below K
SELECT_GRID = [(BELIEF_GAMES[(i + j) % 3], m, k, r) for i, m in enumerate(edge_sizes(WAVE_ROWS))
               for j, (k, r) in enumerate(((65, 63), (130, 65), (63, 1)))]


@case("hb_belief_select", [p + (i % 2 == 0,) for i, p in enumerate(SELECT_GRID)])
def belief_select(g, game, m, n_cand, replicas, with_valid):
    env, rows, det, w, t = _select_inputs(g, game, m, n_cand, 1, True)
    o = _select_outs(g, env, m, replicas, 1, True)
    _call("hb_belief_select", C.byref(env.cfg), _p(rows), _p(det), _p(w), _p(t["hyp"]), _p(t["actual"]),
          _p(t["valid"]) if with_valid else None, m, n_cand, replicas, _p(o["rows"]), _p(o["w"]), _p(o["n_surv"]), _p(o["fallback"]))


@case("hb_belief_select_depth", [p + ((1, 3, 8)[i % 3],) for i, p in enumerate(SELECT_GRID)])
def belief_select_depth(g, game, m, n_cand, replicas, depth):
    env, rows, det, w, t = _select_inputs(g, game, m, n_cand, depth, False)
    o = _select_outs(g, env, m, replicas, depth, False)
    used = g.out("depth_used", (m,), "int32", tail(WAVE_ROWS, 1))
    _call("hb_belief_select_depth", C.byref(env.cfg), _p(rows), _p(det), _p(w), _p(t["hyp"]), _p(t["actual"]), _p(t["valid"]), m, n_cand,
          replicas, depth, _p(o["rows"]), _p(o["w"]), _p(o["n_surv"]), _p(used), _p(o["fallback"]))


# n_cand < replicas is allowed here: (63 candidates, 65 replicas) as well
@case("hb_belief_select_soft", [p + ((1, 3, 8)[i % 3],) for i, p in enumerate(SELECT_GRID + [("full2", 5, 63, 65), ("full5", 3, 1, 130)])])
def belief_select_soft(g, game, m, n_cand, replicas, depth):
    from hanabi_hip.search import soft_table

    env, rows, det, w, t = _select_inputs(g, game, m, n_cand, depth, False)
    table = g.inp("p_table", soft_table(0.1, env.num_actions, "cuda"))
    o = _select_outs(g, env, m, replicas, depth, False)
    used = g.out("depth_used", (m,), "int32", tail(WAVE_ROWS, 1))
    ess = g.out("ess", (m,), "float32", tail(WAVE_ROWS, 1))
    K = _K()
    K.check(K.lib().hb_belief_select_soft(C.byref(env.cfg), _p(rows), _p(det), _p(w), _p(t["hyp"]), _p(t["n_legal"]), _p(t["actual"]),
                                          _p(t["valid"]), _p(table), m, n_cand, replicas, depth, (3 << 32) | 5, (1 << 32) | 2,
                                          (1 << 32) - 3, _p(o["rows"]), _p(o["w"]), _p(o["n_surv"]), _p(used), _p(o["fallback"]),
                                          _p(ess), K.current_stream()))


# belief_history_step_kernel: 256 lanes per workgroup, each moving one 16-byte item of the row buffer or the words of one game
HISTORY_FORMS = ((1, 7), (3, 7), (8, 4), (3, 3))                       # (depth, parts)


@case("hb_belief_history_step", [(gk, m) + HISTORY_FORMS[(i + j) % 4] for i, gk in enumerate(BELIEF_GAMES)
                                 for j, m in enumerate(edge_sizes(LANE_ROWS) + [7])])
def belief_history_step(g, game, m, depth, parts):
    """parts: bit 0 own move, bit 1 reset, bit 2 push (cur and prev rows)."""
    env = _env(game, m, turns=7)
    prev = env.export_state()
    env.step(env.random_legal_actions(seed=21, draw=3))
    cur = env.export_state()
    SW, A = env.state_words, env.num_actions
    rng = np.random.default_rng(m + depth)
    own = g.inp("own_moves", _cuda(rng.integers(0, A, m).astype(np.int32))) if parts & 1 else None
    reset = g.inp("reset", _cuda((rng.random(m) < 0.2).astype(np.uint8))) if parts & 2 else None
    cur_d = g.inp("cur_rows", cur) if parts & 4 else None
    prev_d = g.inp("prev_rows", prev) if parts & 4 else None
    hist0 = prev.repeat(depth, 1).reshape(depth, m, SW)
    hist = g.out("hist_rows", (depth, m, SW), "int32", tail(LANE_ROWS, CHUNK // 4), init=hist0)
    moves = g.out("hist_moves", (depth, m), "int32", tail(LANE_ROWS, 1), init=_cuda(rng.integers(-1, A, (depth, m)).astype(np.int32)))
    alive = g.out("hist_alive", (depth, m), "uint8", tail(LANE_ROWS, 1), init=_cuda(rng.integers(0, 32, (depth, m)).astype(np.uint8)))
    valid = g.out("hist_valid", (depth, m), "uint8", tail(LANE_ROWS, 1), init=_cuda(rng.integers(0, 2, (depth, m)).astype(np.uint8)))
    _call("hb_belief_history_step", C.byref(env.cfg), m, depth, 1, _p(own), _p(reset), _p(cur_d), _p(prev_d), _p(hist), _p(moves),
          _p(alive), _p(valid))


# =================================================================================================================================
# Entry points without a case, each with its reason
# =================================================================================================================================
_HOST = "host-only: no device memory is written"
_OWNED = "writes only memory the library owns"
EXEMPT = {
    "hb_last_error": _HOST, "hb_abi_version": _HOST, "hb_config_validate": _HOST, "hb_num_actions": _HOST, "hb_obs_len": _HOST,
    "hb_deck_size": _HOST, "hb_state_words": _HOST, "hb_obs_words": _HOST, "hb_env_num_games": _HOST, "hb_env_state": _HOST,
    "hb_env_color_shuffled": _HOST, "hb_tree_capacity": _HOST, "hb_tree_nodes": _HOST, "hb_actor_fused_supported": _HOST,
    "hb_actor_fused_sizes": _HOST, "hb_actor_fused_columns": _HOST + " (its output is a host array)",
    "hb_actor_fused_step_supported": _HOST, "hb_eval_counters": _HOST, "hb_eval_response_bins": _HOST, "hb_train_counters": _HOST,
    "hb_event_create": _HOST, "hb_event_destroy": _HOST, "hb_event_record": _HOST, "hb_stream_wait_event": _HOST,
    "hb_env_illegal_count": _HOST + " (reads a library counter into a host integer)",
    "hb_env_stats": _HOST + " (reads library counters into host integers)",
    "hb_tree_error_count": _HOST + " (reads a library counter into a host integer)",
    "hb_chain_run": "host-only dispatcher: it launches nothing of its own, every command forwards to an entry point of this table",
    "hb_env_create": _OWNED, "hb_env_destroy": _OWNED, "hb_env_set_decks": _OWNED + " (borrows a read-only deck buffer)",
    "hb_env_reset": _OWNED + " (state rows, deck pool)", "hb_env_import_state": _OWNED + " (state rows; seen through export_state)",
    "hb_env_set_color_shuffle": _OWNED, "hb_env_set_color_perms": _OWNED, "hb_env_set_games_per_wave": _HOST,
    "hb_env_set_async_refill": _HOST, "hb_env_set_refill_period": _HOST, "hb_env_set_profile_events": _HOST,
    "hb_tree_create": _OWNED, "hb_tree_destroy": _OWNED, "hb_tree_import_nodes": _OWNED + " (the heap; seen through export_nodes)",
    "hb_tree_set_lazy_top": _HOST, "hb_tree_set_ring": _HOST, "hb_tree_update": _OWNED + " (the heap; seen through export_nodes)",
    "hb_tree_fill_range": _OWNED + " (the heap; seen through export_nodes)",
    "hb_encode_rows": "every output guarded in tests/test_encode_rows_gpu.py",
    "hb_belief_score": "every output guarded in tests/test_belief_score_gpu.py",
    "hb_belief_carry": "every output guarded in tests/test_belief_carry_gpu.py",
}


def flat_cases():
    """[(entry, function, parameters)] in table order."""
    return [(entry, fn, p) for entry, lst in CASES.items() for fn, p in lst]


def case_id(entry, p):
    def s(v):
        if isinstance(v, bool):
            return "T" if v else "F"
        if isinstance(v, (tuple, list)):
            return "x".join(s(x) for x in v)
        return str(v)
    return entry[3:] + "-" + "-".join(s(v) for v in p)
