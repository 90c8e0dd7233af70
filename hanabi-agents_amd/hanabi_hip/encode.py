"""The stateless observation encoder: the network's view of state rows that belong to no env.

`encode_rows(cfg, rows, seat=None)` is hb_encode_rows (csrc/encode_rows.hip) on torch tensors: the
canonical observation and the legal-move mask of every row of `rows` [n, state_words] (the layout `HanabiEnv.export_state`
writes: logged rows, determinized rows, the slabs of a belief), for each row's own seat to act or for one observer `seat`.
It is what `env.import_state(rows); env.observe()` gives on a scratch env, bit for bit, without the env, its deck pool or any
change to anything.

`encode_rows_ref` is the same function in plain numpy over the row layout of DESIGN.md section 3: the CPU reference the kernel
is tested against (tests/test_encode_rows_cpu.py holds it to the C oracle). It never touches the library's kernels.
"""
import ctypes as C

import numpy as np

from . import _capi as K


def _sizes(cfg):
    L = K.lib()
    return (L.hb_state_words(C.byref(cfg)), L.hb_obs_len(C.byref(cfg)), L.hb_obs_words(C.byref(cfg)),
            L.hb_num_actions(C.byref(cfg)))


def _seat(cfg, seat):
    s = -1 if seat is None else int(seat)
    if not -1 <= s < cfg.players:
        raise ValueError(f"seat {seat} out of range: None (each row's seat to act) or 0..{cfg.players - 1}")
    return s


def encode_rows(cfg, rows, seat=None, out=None, int8=False):
    """rows [n, state_words] int32 on the GPU -> (obs, legal). obs: the bit-packed rows [n, obs_words] int32 (`HanabiEnv.obs_bits`'
    form), or with int8=True the 0/1 rows [n, obs_len] int8; legal [n, num_actions] int8. seat=None: each row's seat to act;
    seat=o: seat o observes every row, and legal is all zero where it is not the one to act. `out`: an optional (obs, legal) pair
    to write into. The rows are not changed."""
    import torch

    SW, obs_len, obs_words, A = _sizes(cfg)
    s = _seat(cfg, seat)
    if not isinstance(rows, torch.Tensor) or not rows.is_cuda:
        raise K.HbError("the state rows must be a tensor on the GPU (there is no CPU path)")
    if rows.dtype != torch.int32 or rows.dim() != 2 or rows.shape[1] != SW or not rows.is_contiguous():
        raise ValueError(f"state rows are a contiguous int32 tensor of shape [n, {SW}], got {rows.dtype} {tuple(rows.shape)}")
    n, dev = rows.shape[0], rows.device
    oshape, odtype = ((n, obs_len), torch.int8) if int8 else ((n, obs_words), torch.int32)
    if out is None:
        obs = torch.empty(oshape, dtype=odtype, device=dev)
        legal = torch.empty((n, A), dtype=torch.int8, device=dev)
    else:
        obs, legal = out
        for t, shape, dtype, name in ((obs, oshape, odtype, "obs"), (legal, (n, A), torch.int8, "legal")):
            if not isinstance(t, torch.Tensor) or t.shape != shape or t.dtype != dtype or t.device != dev or not t.is_contiguous():
                raise ValueError(f"out: {name} must be a contiguous {dtype} tensor of shape {shape} on {dev}, got "
                                 f"{getattr(t, 'dtype', type(t).__name__)} {tuple(getattr(t, 'shape', ()))} on {getattr(t, 'device', None)}")
    if n == 0:      # (an empty tensor has no address to hand over: nothing to encode, as hb_encode_rows' n_rows == 0)
        return obs, legal
    with torch.cuda.device(dev):
        K.check(K.lib().hb_encode_rows(C.byref(cfg), K.dptr(rows), n, s, None if int8 else K.dptr(obs), K.dptr(obs) if int8 else None,
                                       K.dptr(legal), K.current_stream()))
    return obs, legal


def encode_rows_ref(cfg, rows, seat=None):
    """The same function in numpy: rows [n, state_words] (any 32-bit integer array) -> (obs int8 [n, obs_len], legal int8
    [n, num_actions]). Row layout: word 0 = deck size (6 bits) | information tokens << 6 (4) | lives << 10
    (3) | seat to act << 13 (3); word 1 = firework height of colour c << 3c (3 bits each) | cards held by seat p << 15 + 3p (3);
    word 2 = the last move: valid | player << 1 | type << 4 (0 play, 1 discard, 2 reveal colour, 3 reveal rank) | slot << 6 |
    target offset << 9 | colour << 12 | rank << 15 | scored << 18 | token returned << 19 | touched slots << 20; words 8-9 = the
    discard thermometers, already in the observation's order; word 10 + p = seat p's cards, 5 bits each (colour * ranks + rank);
    words 10 + P + 2p, + 1 = seat p's knowledge, 12 bits a slot: plausible colours (5), plausible ranks << 5 (5), colour
    revealed << 10, rank revealed << 11."""
    P, Cc, R, H = cfg.players, cfg.colors, cfg.ranks, cfg.hand_size
    s = _seat(cfg, seat)
    r = np.ascontiguousarray(np.asarray(rows)).view(np.uint32).astype(np.int64)
    n = r.shape[0]
    bits = Cc * R
    per_colour = sum(3 if k == 0 else (1 if k == R - 1 else 2) for k in range(R))
    D = Cc * per_colour
    A = 2 * H + (P - 1) * (Cc + R)
    g = np.arange(n)
    w0, w1, w2 = r[:, 0], r[:, 1], r[:, 2]
    deck, info, life, cur = w0 & 63, (w0 >> 6) & 15, (w0 >> 10) & 7, (w0 >> 13) & 7
    o = cur if s < 0 else np.full(n, s, np.int64)
    hand_n = np.stack([(w1 >> (15 + 3 * p)) & 7 for p in range(P)], axis=1)                       # [n, P]
    cards = np.stack([np.stack([(r[:, 10 + p] >> (5 * i)) & 31 for i in range(H)], axis=1) for p in range(P)], axis=1)  # [n, P, H]
    kn64 = np.stack([r[:, 10 + P + 2 * p] | (r[:, 10 + P + 2 * p + 1] << 32) for p in range(P)], axis=1)   # (< 2^60: fits int64)
    know = np.stack([(kn64 >> (12 * i)) & 0xFFF for i in range(H)], axis=2)                     # [n, P, H]
    held = np.arange(H)[None, None, :] < hand_n[:, :, None]                                     # [n, P, H]

    out, legal = [], np.zeros((n, A), np.int8)
    # 1. the other seats' hands, observer-relative, then one "hand is short" flag per seat (the observer's first)
    for rel in range(1, P):
        who = (o + rel) % P
        for i in range(H):
            have = held[g, who, i]
            sec = np.zeros((n, bits), np.int8)
            sec[g[have], cards[g, who, i][have]] = 1
            out.append(sec)
            # a hint is legal when a token is left and it touches a card
            ok = have & (info > 0)
            legal[g[ok], 2 * H + (rel - 1) * Cc + cards[g, who, i][ok] // R] = 1
            legal[g[ok], 2 * H + (P - 1) * Cc + (rel - 1) * R + cards[g, who, i][ok] % R] = 1
    out.append(np.stack([hand_n[g, (o + rel) % P] < H for rel in range(P)], axis=1).astype(np.int8))
    own_n = hand_n[g, o]
    own = np.arange(H)[None, :] < own_n[:, None]
    legal[:, :H] = own & (info < cfg.max_info)[:, None]       # discards
    legal[:, H:2 * H] = own                                   # plays
    # 2. the board: deck, fireworks, information and life tokens
    therm = lambda v, length: (np.arange(length)[None, :] < v[:, None]).astype(np.int8)
    out.append(therm(deck, D - P * H))
    fw = np.stack([(w1 >> (3 * c)) & 7 for c in range(Cc)], axis=1)
    out.append((np.arange(R)[None, None, :] == (fw - 1)[:, :, None]).astype(np.int8).reshape(n, bits))
    out.append(therm(info, cfg.max_info))
    out.append(therm(life, cfg.max_life))
    # 3. the discards
    disc = r[:, 8] | (r[:, 9] << 32)
    out.append(np.stack([(disc >> k) & 1 for k in range(D)], axis=1).astype(np.int8))
    # 4. the last move, observer-relative
    valid = (w2 & 1) == 1
    mtype, slot, toff = (w2 >> 4) & 3, (w2 >> 6) & 7, (w2 >> 9) & 7
    colour, rank = (w2 >> 12) & 7, (w2 >> 15) & 7
    scored, token, touched = (w2 >> 18) & 1, (w2 >> 19) & 1, (w2 >> 20) & 31
    actor = (((w2 >> 1) & 7) - o) % P
    target = (actor + toff) % P
    reveal, card_move = valid & (mtype >= 2), valid & (mtype <= 1)

    def one_hot(length, where, index):
        sec = np.zeros((n, length), np.int8)
        sec[g[where], index[where]] = 1
        return sec

    out.append(one_hot(P, valid, actor))
    out.append(one_hot(4, valid, mtype))
    out.append(one_hot(P, reveal, target))
    out.append(one_hot(Cc, valid & (mtype == 2), colour))
    out.append(one_hot(R, valid & (mtype == 3), rank))
    out.append((np.stack([(touched >> i) & 1 for i in range(H)], axis=1) * reveal[:, None]).astype(np.int8))
    out.append(one_hot(H, card_move, slot))
    out.append(one_hot(bits, card_move, colour * R + rank))
    play = valid & (mtype == 0)
    out.append(np.stack([play & (scored == 1), play & (token == 1)], axis=1).astype(np.int8))
    # 5. card knowledge, the observer's own hand first
    for rel in range(P):
        who = (o + rel) % P
        for i in range(H):
            k = know[g, who, i]
            have = held[g, who, i]
            cp = np.stack([(k >> c) & 1 for c in range(Cc)], axis=1)
            rp = np.stack([(k >> (5 + q)) & 1 for q in range(R)], axis=1)
            sec = np.concatenate([(cp[:, :, None] & rp[:, None, :]).reshape(n, bits), cp * ((k >> 10) & 1)[:, None],
                                  rp * ((k >> 11) & 1)[:, None]], axis=1)
            out.append((sec * have[:, None]).astype(np.int8))
    obs = np.concatenate(out, axis=1)
    assert obs.shape[1] == K.lib().hb_obs_len(C.byref(cfg))
    legal[o != cur] = 0
    return obs, legal
