"""Colour-permuted frames (Other-Play, Hu et al. 2020) on the host.

A shuffled env (`HanabiEnv(color_shuffle=...)`) gives every game g and seat p a permutation sigma_{g,p} of the colours,
fixed for one deal: the seat sees true colour c as sigma(c). `HanabiEnv.color_perms()` returns them as `perms[g, p, c] =
sigma_{g,p}(c)`. The helpers here apply the same relabelling to logged data with numpy (torch tensors are accepted and
returned as tensors on their device); the tests use them as the independent check of the env kernel.

Only colour-carrying fields move, by whole colour blocks: the other players' cards, fireworks, discards, the last move's
revealed colour and card, and every knowledge slot's plausible identities and revealed-colour bits. Moves: reveal-colour
uid 2H + o*C + c becomes 2H + o*C + sigma(c); every other uid is colour-free.
"""
import math

import numpy as np

__all__ = ["permutation", "perm_index", "seat_mask", "layout", "compose", "invert", "permute_obs", "permute_legal",
           "permute_actions", "unpermute_actions"]


def permutation(index, C):
    """The index-th permutation of 0..C-1 in lexicographic order (Lehmer decode): sigma as an int array, sigma[c] = sigma(c).
    Index 0 is the identity."""
    index = int(index)
    if not 0 <= index < math.factorial(C):
        raise ValueError(f"permutation index {index} out of range for {C} colours")
    pool, out = list(range(C)), []
    for i in range(C):
        d, index = divmod(index, math.factorial(C - 1 - i))
        out.append(pool.pop(d))
    return np.array(out, dtype=np.int64)


def perm_index(draw, C):
    """The permutation index the env takes from one 32-bit Philox output word: (draw * C!) >> 32."""
    return (int(draw) * math.factorial(C)) >> 32


def seat_mask(spec, players):
    """The per-game seat bit mask for a `color_shuffle` argument: True (every seat), False / None (none), an int mask, or an
    iterable of seat numbers. Raises ValueError for a seat outside 0..players-1."""
    if spec is None or spec is False:
        return 0
    if spec is True:
        return (1 << players) - 1
    if isinstance(spec, (int, np.integer)):
        m = int(spec)
    else:
        m = 0
        for s in spec:
            s = int(s)
            if not 0 <= s < players:
                raise ValueError(f"seat {s} is not one of the {players} seats")
            m |= 1 << s
    if m < 0 or m >> players:
        raise ValueError(f"seat mask {m:#x} names a seat past the {players} players")
    return m


def layout(cfg):
    """Section offsets of the canonical observation for an hb_config-like object (players, colors, ranks, hand_size,
    max_info, max_life): the formulas of Cfg in csrc/env_kernel.hpp."""
    P, C, R, H = cfg.players, cfg.colors, cfg.ranks, cfg.hand_size
    bits = C * R
    cpc = sum(3 if r == 0 else (1 if r == R - 1 else 2) for r in range(R))
    D = C * cpc
    fw = (P - 1) * H * bits + P + (D - P * H)
    disc = fw + bits + cfg.max_info + cfg.max_life
    la = disc + D
    o4 = la + P + 4 + P
    o8 = o4 + C + R + H + H
    kn = la + (P + 4 + P + C + R + H + H + bits + 2)
    slot = bits + C + R
    return dict(P=P, C=C, R=R, H=H, BITS=bits, CPC=cpc, D=D, FW_OFF=fw, DISC_OFF=disc, O4=o4, O8=o8, KN_OFF=kn, KN_SLOT=slot,
                OBS_LEN=kn + P * H * slot, A=2 * H + (P - 1) * (C + R))


def compose(sigma, tau):
    """(sigma o tau)(c) = sigma(tau(c)), elementwise over leading axes."""
    sigma, tau = np.asarray(sigma), np.asarray(tau)
    return np.take_along_axis(sigma, tau, axis=-1)


def invert(sigma):
    """sigma^-1 along the last axis."""
    sigma = np.asarray(sigma)
    inv = np.empty_like(sigma)
    np.put_along_axis(inv, sigma, np.broadcast_to(np.arange(sigma.shape[-1]), sigma.shape), axis=-1)
    return inv


def _host(x):
    try:
        import torch

        if isinstance(x, torch.Tensor):
            return x.detach().cpu().numpy(), x
    except ImportError:
        pass
    return np.asarray(x), None


def _like(a, ref):
    if ref is None:
        return a
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(ref.device)


def _seat_perms(perms, seat, n):
    """sigma of the observing seat of every game: [n, C]. `perms` is [n, P, C] (or [n, C] / [C], already one seat's)."""
    p = _host(perms)[0].astype(np.int64)
    if p.ndim == 1:
        return np.broadcast_to(p, (n, p.shape[0]))
    if p.ndim == 2:
        return np.broadcast_to(p, (n, p.shape[1])) if p.shape[0] != n else p
    s = np.broadcast_to(np.asarray(_host(seat)[0], dtype=np.int64), (n,))
    return p[np.arange(n), s]


def _block_map(sig, L, blocks):
    """Destination index of every position of an [n, L] row: blocks = (base, C, width) groups of colour-major blocks."""
    n, C = sig.shape
    fwd = np.broadcast_to(np.arange(L, dtype=np.int64), (n, L)).copy()
    for base, width in blocks:
        j = np.arange(width)
        for c in range(C):
            fwd[:, base + c * width + j] = base + sig[:, c, None] * width + j
    return fwd


def _obs_blocks(lay):
    L = lay
    out = [((k * L["BITS"]), L["R"]) for k in range((L["P"] - 1) * L["H"])]      # other hands: one-hot c*R + r
    out += [(L["FW_OFF"], L["R"]), (L["DISC_OFF"], L["CPC"]), (L["O4"], 1), (L["O8"], L["R"])]
    for s in range(L["P"] * L["H"]):
        b = L["KN_OFF"] + s * L["KN_SLOT"]
        out += [(b, L["R"]), (b + L["BITS"], 1)]                                  # plausible identities, revealed colour
    return out


def permute_obs(obs, perms, seat, cfg):
    """Observation rows in the observing seat's frame: obs [n, obs_len] int8 0/1 or bit-packed [n, ceil(obs_len / 32)] 32-bit
    words (bit i = word i >> 5, bit i & 31); perms [n, P, C] sigma(c) (hanabi_hip env.color_perms()); seat: the observing seat,
    an int or [n]. Same dtype and form as `obs`."""
    x, ref = _host(obs)
    lay = layout(cfg)
    L = lay["OBS_LEN"]
    n = x.shape[0]
    packed = x.shape[1] != L
    if packed:
        if x.shape[1] != (L + 31) // 32:
            raise ValueError(f"rows of {x.shape[1]} entries are neither {L} bytes nor {(L + 31) // 32} words")
        w = x.astype(np.uint32)
        bits = ((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(n, -1)[:, :L].astype(np.int8)
    else:
        bits = x
    sig = _seat_perms(perms, seat, n)
    fwd = _block_map(sig, L, _obs_blocks(lay))
    out = np.zeros_like(bits)
    np.put_along_axis(out, fwd, bits, axis=1)
    if packed:
        pad = np.zeros((n, x.shape[1] * 32), np.uint64)
        pad[:, :L] = out
        words = (pad.reshape(n, -1, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)
        out = words.view(np.int32).astype(x.dtype) if x.dtype.kind == "i" else words.astype(x.dtype)
    return _like(out, ref)


def permute_legal(legal, perms, seat, cfg):
    """Legal-move rows [n, A] (0/1 bytes, or one bit per move in an integer word per row) in the acting seat's frame: the
    reveal-colour moves of each target move by sigma."""
    x, ref = _host(legal)
    lay = layout(cfg)
    n = x.shape[0]
    sig = _seat_perms(perms, seat, n)
    base, C = 2 * lay["H"], lay["C"]
    if x.ndim == 1:   # bit masks
        m = x.astype(np.uint64)
        out = m.copy()
        for o in range(lay["P"] - 1):
            for c in range(C):
                out &= ~np.uint64(1 << (base + o * C + c))
            for c in range(C):
                bit = (m >> np.uint64(base + o * C + c)) & np.uint64(1)
                out |= bit << (np.uint64(base + o * C) + sig[:, c].astype(np.uint64))
        return _like(out.astype(x.dtype), ref)
    fwd = _block_map(sig, x.shape[1], [(base + o * C, 1) for o in range(lay["P"] - 1)])
    out = np.zeros_like(x)
    np.put_along_axis(out, fwd, x, axis=1)
    return _like(out, ref)


def _map_actions(actions, perms, seat, cfg, inverse):
    x, ref = _host(actions)
    lay = layout(cfg)
    a = x.astype(np.int64)
    n = a.shape[0]
    sig = _seat_perms(perms, seat, n)
    if inverse:
        sig = invert(sig)
    base, C = 2 * lay["H"], lay["C"]
    xc = a - base
    rc = (xc >= 0) & (xc < (lay["P"] - 1) * C)
    o, c = np.divmod(np.where(rc, xc, 0), C)
    mapped = base + o * C + sig[np.arange(n), c]
    return _like(np.where(rc, mapped, a).astype(x.dtype), ref)


def permute_actions(actions, perms, seat, cfg):
    """Move uids [n] from the true frame into the acting seat's frame (reveal colour c -> sigma(c))."""
    return _map_actions(actions, perms, seat, cfg, inverse=False)


def unpermute_actions(actions, perms, seat, cfg):
    """Move uids [n] from the acting seat's frame back to the true colours (sigma^-1): what the env applies."""
    return _map_actions(actions, perms, seat, cfg, inverse=True)
