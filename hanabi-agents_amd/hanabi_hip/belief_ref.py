"""The belief kernels restated in numpy (csrc/belief.hip, include/hanabi_hip.h): what the tests and the probe scripts hold
hb_belief_select_soft, hb_belief_carry and hb_belief_score against, the same arithmetic written without anything of the kernels'
layout. Nothing here runs on a GPU, and nothing in the package's own code paths calls it.
"""

_M32, _M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF


def _philox_np(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on numpy arrays (broadcast) -> the four output words as uint64 arrays below 2^32."""
    import numpy as np

    c0, c1, c2, c3 = (np.asarray(x, np.uint64) & np.uint64(_M32) for x in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = int(k0) & _M32, int(k1) & _M32
    lo, sh = np.uint64(_M32), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ np.uint64(k0), p1 & lo, (p0 >> sh) ^ c3 ^ np.uint64(k1), p0 & lo
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return c0, c1, c2, c3


def belief_select_soft_ref(src_rows, det_rows, weights, hyp_moves, n_legal, actual, valid, p_table, replicas, seed, draw,
                           first_row_id=0, details=False):
    """hb_belief_select_soft restated in numpy, the same arithmetic in the same order (include/hanabi_hip.h): arrays shaped as
    belief_select_soft's tensors (32-bit words of either sign) -> (rows uint32 [m * R, SW], weights uint32 [m * R], n_surv int32
    [D, m], depth_used int32 [m], fallback uint8 [m], ess float32 [m]). details=True appends a dict of the intermediate figures:
    lik float64 [m, K], q and W uint64 [m, K], T uint64 [m], target uint64 [m, R] and pick int64 [m, R] (-1: dead)."""
    import numpy as np

    u32 = lambda x: (np.asarray(x).astype(np.int64) & _M32).astype(np.uint32)
    src, det = u32(src_rows), u32(det_rows)
    (m, SW), R = src.shape, int(replicas)
    hyp, nl, act = np.asarray(hyp_moves).astype(np.int64), np.asarray(n_legal).astype(np.int64), np.asarray(actual).astype(np.int64)
    D, Kn = hyp.shape[0], hyp.shape[1]
    assert hyp.shape == nl.shape == (D, Kn, m) and act.shape == (D, m) and det.shape == (m * Kn, SW)
    w = u32(weights).reshape(m, Kn).astype(np.uint64)
    table = np.asarray(p_table, np.float64)
    A = table.shape[1] - 1
    run = ((src[:, 0] >> np.uint32(19)) & np.uint32(3)) == 0
    usable = np.ones((D, m), bool) if valid is None else np.asarray(valid).reshape(D, m) != 0
    chain = np.cumprod(usable & run[None], axis=0).astype(bool)   # [D, m]: entry d is one of the root's L leading valid ones
    L = chain.sum(0).astype(np.int32)
    live = w != 0
    lik, on = np.where(live, 1.0, 0.0), live.copy()
    n_surv = np.zeros((D, m), np.int32)
    for d in range(D):
        match, n = hyp[d].T == act[d][:, None], nl[d].T   # [m, K]
        factor = np.where((n >= 1) & (n <= A), table[np.where(match, 0, 1), np.clip(n, 0, A)], 0.0)
        lik = np.where(chain[d][:, None] & live, lik * factor, lik)
        on = on & match & chain[d][:, None]
        n_surv[d] = on.sum(1)
    mx = lik.max(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(mx[:, None] > 0, np.floor(lik / mx[:, None] * 16777216.0), 0.0).astype(np.uint64)
    W = w * q
    T = W.sum(1, dtype=np.uint64)
    Wf = W.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ess = np.where(T > 0, T.astype(np.float64) * T.astype(np.float64) / (Wf * Wf).sum(1), 0.0).astype(np.float32)
    rid = [(int(first_row_id) + i) & _M64 for i in range(m)]
    x = _philox_np(0x10000 + np.arange(R, dtype=np.uint64)[None], int(draw) & _M32, np.array([v & _M32 for v in rid], np.uint64)[:, None],
                   np.array([v >> 32 for v in rid], np.uint64)[:, None], int(seed) & _M32, ((int(seed) >> 32) ^ (int(draw) >> 32)) & _M32)
    u = (x[0] << np.uint64(32)) | x[1]   # [m, R]
    target, pick = np.zeros((m, R), np.uint64), np.full((m, R), -1, np.int64)
    rows, ow = np.empty((m * R, SW), np.uint32), np.zeros(m * R, np.uint32)
    prefix = np.cumsum(W, axis=1, dtype=np.uint64)
    for i in range(m):
        if T[i] == 0:
            rows[i * R:(i + 1) * R] = src[i]
            continue
        target[i] = np.array([(int(v) * int(T[i])) >> 64 for v in u[i]], np.uint64)
        pick[i] = np.searchsorted(prefix[i], target[i], side="right")   # the first k whose inclusive prefix exceeds the target
        rows[i * R:(i + 1) * R] = det[i * Kn + pick[i]]
        ow[i * R:(i + 1) * R] = 1
    out = (rows, ow, n_surv, L, np.where(L == 0, 2, 0).astype(np.uint8), ess)
    return out + (dict(lik=lik, q=q, W=W, T=T, target=target, pick=pick),) if details else out


def belief_carry_ref(cfg, cur_rows, old_rows, old_weights, own_slot, revealed, drew, seat, n_particles, seed, draw, first_row_id=0,
                     draw_weight=True, details=False):
    """hb_belief_carry restated in numpy, particle by particle in plain loops over Python lists (nothing of the kernel's layout):
    arrays shaped as belief_carry's tensors (32-bit words of either sign) -> (rows uint32 [m * K, SW], weights uint32 [m * K]).
    draw_weight=False is the deliberately wrong variant with g = 1 (step 5 left out) that the tests hold against the right one.
    details=True appends a list with one dict per particle: `dead` (the step that killed it, or 0), `kept`, `g`, `ns`. Runs
    without a GPU."""
    import numpy as np

    u32 = lambda x: (np.asarray(x).astype(np.int64) & _M32).astype(np.uint32)
    cur, old = u32(cur_rows), u32(old_rows)
    (m, SW), Kn, st = cur.shape, int(n_particles), int(seat)
    ow = u32(old_weights)
    slot_a, rev_a, drew_a = (np.asarray(x).astype(np.int64) for x in (own_slot, revealed, drew))
    assert old.shape == (m * Kn, SW) and ow.shape == (m * Kn,) and slot_a.shape == rev_a.shape == drew_a.shape == (m,)
    P, H, Rk, Cn = cfg.players, cfg.hand_size, cfg.ranks, cfg.colors
    assert 0 <= st < P
    D = Cn * sum(3 if r == 0 else 1 if r == Rk - 1 else 2 for r in range(Rk))
    seed, draw = int(seed) & _M64, int(draw) & _M64
    rows, w, info = np.empty((m * Kn, SW), np.uint32), np.zeros(m * Kn, np.uint32), []

    def allows(kn, c):
        return c // Rk < Cn and bool((kn >> (c // Rk)) & 1) and bool((kn >> (5 + c % Rk)) & 1)

    for o in range(m * Kn):
        i = o // Kn
        rows[o] = cur[i]
        note = dict(dead=0, kept=[], g=1, ns=[])
        info.append(note)
        w0, w1 = int(cur[i, 0]), int(cur[i, 1])
        if ow[o] == 0 or (w0 >> 19) & 3 != 0 or (w0 >> 13) & 7 != st:   # 1. not usable
            note["dead"] = 1
            continue
        old_hand, slot = int(old[o, 10 + st]), int(slot_a[i])
        fields = [(old_hand >> (5 * s)) & 31 for s in range(H)]
        if slot >= 0 and (slot >= H or fields[slot] != int(rev_a[i])):   # 2. the card I played is not the one that was seen
            note["dead"] = 2
            continue
        kept = note["kept"] = [f for s, f in enumerate(fields) if s != slot and f != 31]
        n_hand = min((w1 >> (15 + 3 * st)) & 7, H)
        if len(kept) > n_hand:
            note["dead"] = 2
            continue
        hand = int(cur[i, 10 + st])
        know = int(cur[i, 10 + P + 2 * st]) | int(cur[i, 10 + P + 2 * st + 1]) << 32
        deck_pos = D - min(w0 & 63, D)
        deck = np.ascontiguousarray(cur[i, 10 + 3 * P:], dtype="<u4").view(np.uint8)
        pool = [(hand >> (5 * l)) & 31 for l in range(n_hand)] + [int(deck[q]) for q in range(deck_pos, D)]   # 3.
        free = [True] * len(pool)
        new_hand = hand
        for s, c in enumerate(kept):   # 4. the kept cards, where they now sit
            where = [l for l in range(len(pool)) if free[l] and pool[l] == c]
            if not where or not allows((know >> (12 * s)) & 0xFFF, c):
                note["dead"] = 4
                break
            free[where[0]] = False
            new_hand = (new_hand & ~(31 << (5 * s))) | (c << (5 * s))
        if note["dead"]:
            continue
        g = 1
        if draw_weight and int(drew_a[i]) >= 0:   # 5. the partner's draw
            g += sum(1 for l in range(len(pool)) if free[l] and pool[l] == int(drew_a[i]))
        note["g"] = g
        rid = (int(first_row_id) + o) & _M64
        rnd = _philox_np(128 + np.arange(64), draw & _M32, rid & _M32, rid >> 32, seed & _M32, ((seed >> 32) ^ (draw >> 32)) & _M32)
        weight = g
        for s in range(len(kept), n_hand):   # 6. the new slots: the determinizer's step
            kn = (know >> (12 * s)) & 0xFFF
            cand = [l for l in range(len(pool)) if free[l] and allows(kn, pool[l])]
            note["ns"].append(len(cand))
            if not cand:
                note["dead"] = 6
                break
            pick = cand[(int(rnd[0][s]) * len(cand)) >> 32]
            free[pick] = False
            weight *= len(cand)
            new_hand = (new_hand & ~(31 << (5 * s))) | (pool[pick] << (5 * s))
        if note["dead"]:
            continue
        rest = sorted((l for l in range(len(pool)) if free[l]), key=lambda l: (int(rnd[1][l]) & ~63) | l)   # 7. the deck
        rows[o, 10 + st] = new_hand
        bytes_out = rows[o, 10 + 3 * P:].view(np.uint8)
        for j, l in enumerate(rest):
            bytes_out[deck_pos + j] = pool[l]
        w[o] = weight & _M32
    return (rows, w, info) if details else (rows, w)


def belief_score_ref(cfg, true_rows, det_rows, weights, seat, replicas):
    """hb_belief_score restated in numpy, row by row and replica by replica in plain loops (nothing of the kernel's layout): arrays
    shaped as belief_score's tensors (32-bit words of either sign) -> a dict of numpy arrays: truth int8 [m, H], hit int64
    [m, H], joint, wsum int64 [m], n_live int32 [m], counts int64 [m, H, NC], prior int8 [m, H, NC]. Runs without a GPU;
    `BeliefScore(**belief_score_ref(...))` gives the figures."""
    import numpy as np

    u32 = lambda x: (np.asarray(x).astype(np.int64) & _M32).astype(np.uint32)
    rows, det = u32(true_rows), u32(det_rows)
    (m, SW), R = rows.shape, int(replicas)
    w = u32(weights).reshape(m, R)
    assert det.shape == (m * R, SW)
    P, H, Rk, NC = cfg.players, cfg.hand_size, cfg.ranks, cfg.colors * cfg.ranks
    D = cfg.colors * sum(3 if r == 0 else 1 if r == Rk - 1 else 2 for r in range(Rk))
    out = dict(truth=np.full((m, H), -1, np.int8), hit=np.zeros((m, H), np.int64), joint=np.zeros(m, np.int64),
               wsum=np.zeros(m, np.int64), n_live=np.zeros(m, np.int32), counts=np.zeros((m, H, NC), np.int64),
               prior=np.zeros((m, H, NC), np.int8))
    for i in range(m):
        w0, w1 = int(rows[i, 0]), int(rows[i, 1])
        st = int(seat) if int(seat) >= 0 else (w0 >> 13) & 7
        if (w0 >> 19) & 3 != 0 or st >= P:
            continue
        hand = int(rows[i, 10 + st])
        know = int(rows[i, 10 + P + 2 * st]) | int(rows[i, 10 + P + 2 * st + 1]) << 32
        n = min((w1 >> (15 + 3 * st)) & 7, H)
        true = [(hand >> (5 * s)) & 31 for s in range(n)]
        deck = np.ascontiguousarray(rows[i, 10 + 3 * P:], dtype="<u4").view(np.uint8)
        pool = true + [int(deck[q]) for q in range(D - min(w0 & 63, D), D)]
        for s in range(n):
            out["truth"][i, s] = true[s]
            kn = (know >> (12 * s)) & 0xFFF
            for c in range(NC):
                if (kn >> (c // Rk)) & 1 and (kn >> (5 + c % Rk)) & 1:
                    out["prior"][i, s, c] = pool.count(c)
        for r in range(R):
            wr = int(w[i, r])
            if wr == 0:
                continue
            out["wsum"][i] += wr
            out["n_live"][i] += 1
            word = int(det[i * R + r, 10 + st])
            cards = [(word >> (5 * s)) & 31 for s in range(n)]
            for s in range(n):
                if cards[s] < NC:
                    out["counts"][i, s, cards[s]] += wr
            if all(c < NC and c == t for c, t in zip(cards, true)):
                out["joint"][i] += wr
        for s in range(n):
            if true[s] < NC:
                out["hit"][i, s] = out["counts"][i, s, true[s]]
    return out


LEAF_SCALE = 4   # a depth-limited search keeps its leaf values in quarter points, in the int8 buffer the reduce kernels read


def _mix32_np(x):
    """The 32-bit finalizer of leaf_dither_ref on int64 arrays (or Python ints) below 2^32: xor-shift 16, times 0x7FEB352D, xor-shift
    15, times 0x846CA68B, xor-shift 16, every product taken mod 2^32 from 16-bit halves of the constant so that no intermediate
    reaches 2^49 (nothing ever wraps: plain signed 64-bit arithmetic gives the same bits everywhere)."""
    def mul(x, c):
        return (x * (c & 0xFFFF) + (((x * (c >> 16)) & 0xFFFF) << 16)) & _M32

    x = x ^ (x >> 16)
    x = mul(x, 0x7FEB352D)
    x = x ^ (x >> 15)
    x = mul(x, 0x846CA68B)
    return x ^ (x >> 16)


def leaf_dither_ref(seed, draw, first_row_id, m, replicas):
    """The dither of a depth-limited search's stochastic rounding: u [m, replicas] float64 in [0, 1), a multiple of 2^-24 and a pure
    function of (seed, draw, row id = first_row_id + i * replicas + r) — the row id of the replica, so every slot of a replica
    rounds with the same u. h = 0x9E3779B9; for each 32-bit word v of (seed lo, seed hi, draw lo, draw hi, row id lo, row id hi)
    in that order h = mix32(h ^ v); u = (h >> 8) * 2^-24. ("Depth-limited rollouts".)"""
    import numpy as np

    m, R = int(m), int(replicas)
    seed, draw = int(seed) & _M64, int(draw) & _M64
    h = 0x9E3779B9
    for v in (seed & _M32, seed >> 32, draw & _M32, draw >> 32):
        h = _mix32_np(h ^ v)
    rid = int(first_row_id) + np.arange(m * R, dtype=np.int64).reshape(m, R)
    h = _mix32_np(np.int64(h) ^ (rid & _M32))
    h = _mix32_np(h ^ ((rid >> 32) & _M32))
    return (h >> 8).astype(np.float64) * 2.0 ** -24


def search_leaf_ref(done, final_score, score, q, legal, u, max_score):
    """The leaf step of a depth-limited search in numpy (the specification of `hanabi_hip.search.search_leaf`): done [m, C, R]
    uint8 (hb_eval_tally's status byte), final_score and score [m, C, R] int8 (the tally's final score; the env's current score),
    q [m, C, R, A] float (None: leaf="score", v = 0), legal [m, C, R, A] (!= 0: legal), u [m, R] float64 (leaf_dither_ref) ->
    leaf4 [m, C, R] int8, the value of every rollout game in quarter points:

      bit 7 of done set (finished before the horizon, or never played):  4 * final_score
      else, with v = the largest FINITE q over the legal moves (0 when there is none; NaN and +-inf entries are passed over)
      and x = 4 * (score + v) in float64:                                clamp(floor(x + u[i, r]), 0, 4 * max_score)

    Stochastic rounding: E_u[leaf4] = x wherever the clamp is inactive."""
    import numpy as np

    done, fs, sc = np.asarray(done), np.asarray(final_score).astype(np.int64), np.asarray(score).astype(np.float64)
    m, Cn, R = done.shape
    u = np.asarray(u, np.float64).reshape(m, 1, R)
    v = np.zeros((m, Cn, R), np.float64)
    if q is not None:
        qq = np.asarray(q).astype(np.float64)
        ok = (np.asarray(legal) != 0) & np.isfinite(qq)
        v = np.where(ok.any(-1), np.where(ok, qq, -np.inf).max(-1), 0.0)
    x = LEAF_SCALE * (sc + v)
    run = np.clip(np.floor(x + u), 0, LEAF_SCALE * int(max_score))
    return np.where((done & 0x80) != 0, LEAF_SCALE * fs, run.astype(np.int64)).astype(np.int8)


def belief_enumerate_ref(cfg, rows, seat, hist_rows, hist_moves, hist_alive, hist_valid, draws, move_fn, max_hands, replicas, seed,
                         draw, first_row_id=0, details=False):
    """hb_belief_enumerate (include/hanabi_hip_exact.h) restated in plain loops over roots and hands, with nothing of the kernel's
    layout: rows [m, SW] the states now, `seat` the observer, the history in PartnerHistory's layout (hist_rows [D, m, SW],
    hist_moves [D, m], hist_alive / hist_valid [D, m] or None, draws a list of D ints; hist_rows None or empty: D = 0) -> a dict
    of numpy arrays: status uint8 [m], space int64 [m], mass int64 [D + 1, m], n_hands int32 [D + 1, m], depth_used int32 [m],
    fallback uint8 [m], marg and marg0 int64 [m, H, NC], hands uint32 [m, R].

    The partners' moves are the caller's to supply (nothing here knows a rule): for each entry d, ONE call

        move_fn(rows [k, SW] uint32, mover_seat [k] int64, draws[d], root [k] int64) -> uids [k]

    with the hypothetical states of every hand that has reproduced the entries before d: row j is the state of root root[j] (the
    partner's draws are keyed by its game id, first_game_id + root[j]: the caller's to apply) in which seat mover_seat[j] moves.
    details=True appends, per root, the list of (cards, mass, pass) of every hand in enumeration order (None unless status 0)."""
    import numpy as np

    u32 = lambda x: (np.asarray(x).astype(np.int64) & _M32).astype(np.uint32)
    cur = u32(rows)
    (m, SW), R, st = cur.shape, int(replicas), int(seat)
    D = 0 if hist_rows is None else len(hist_rows)
    P, H, Rk, Cn = cfg.players, cfg.hand_size, cfg.ranks, cfg.colors
    NC = Cn * Rk
    deck_n = Cn * sum(3 if r == 0 else 1 if r == Rk - 1 else 2 for r in range(Rk))
    assert 0 <= st < P and 0 <= D <= 8 and R >= 1 and int(max_hands) >= 1
    if D:
        hrows, hmoves = u32(hist_rows), np.asarray(hist_moves).astype(np.int64)
        assert hrows.shape == (D, m, SW) and hmoves.shape == (D, m) and len(draws) == D
        alive = None if hist_alive is None else np.asarray(hist_alive).astype(np.int64).reshape(D, m)
        valid = None if hist_valid is None else np.asarray(hist_valid).astype(np.int64).reshape(D, m)
    out = dict(status=np.zeros(m, np.uint8), space=np.zeros(m, np.int64), mass=np.zeros((D + 1, m), np.int64),
               n_hands=np.zeros((D + 1, m), np.int32), depth_used=np.zeros(m, np.int32), fallback=np.zeros(m, np.uint8),
               marg=np.zeros((m, H, NC), np.int64), marg0=np.zeros((m, H, NC), np.int64), hands=np.zeros((m, R), np.uint32))
    hands = [None] * m    # per enumerated root: [cards tuple, mass, pass count, still matching]
    depth_of = [0] * m    # L_i
    for i in range(m):
        w0, w1, own = int(cur[i, 0]), int(cur[i, 1]), int(cur[i, 10 + st])
        out["hands"][i, :] = own
        if (w0 >> 19) & 3 != 0:
            out["status"][i] = 2
            continue
        n = min((w1 >> (15 + 3 * st)) & 7, H)
        know = int(cur[i, 10 + P + 2 * st]) | int(cur[i, 10 + P + 2 * st + 1]) << 32
        deck = np.ascontiguousarray(cur[i, 10 + 3 * P:], dtype="<u4").view(np.uint8)
        pool = [(own >> (5 * s)) & 31 for s in range(n)] + [int(deck[q]) for q in range(deck_n - min(w0 & 63, deck_n), deck_n)]
        cnt = [pool.count(c) for c in range(NC)]
        allowed = []
        for s in range(n):
            kn = (know >> (12 * s)) & 0xFFF
            allowed.append([c for c in range(NC) if cnt[c] > 0 and (kn >> (c // Rk)) & 1 and (kn >> (5 + c % Rk)) & 1])
        N = 1
        for a in allowed:
            N *= len(a)
        out["space"][i] = N
        if N > int(max_hands):
            out["status"][i] = 1
            continue
        L = 0
        while L < D and (valid is None or valid[L, i] != 0):
            L += 1
        depth_of[i] = L
        mine = hands[i] = []
        for e in range(N):
            cards, mass, x = [], 1, e
            for s in range(n):
                c = allowed[s][x % len(allowed[s])]
                x //= len(allowed[s])
                mass *= max(cnt[c] - cards.count(c), 0)
                cards.append(c)
            mine.append([tuple(cards), mass, 0, mass > 0])
    for d in range(D):   # the hands that have reproduced every entry before d, of the roots that have an entry d
        batch = []
        for i in range(m):
            if hands[i] is None or d >= depth_of[i]:
                continue
            prev = hrows[d, i]
            mover = (int(prev[0]) >> 13) & 7
            word, bits = int(prev[10 + st]), 0xFF if alive is None else int(alive[d, i])
            for h in hands[i]:
                if not h[3]:
                    continue
                if mover >= P:   # a row that names no seat reproduces nothing
                    h[3] = False
                    continue
                w, t = word, 0   # hb_belief_splice_alive's rule: the alive occupied slots take the hand's cards as a prefix
                for s in range(5):
                    if (word >> (5 * s)) & 31 != 31 and (bits >> s) & 1 and t < len(h[0]):
                        w = (w & ~(31 << (5 * s))) | (h[0][t] << (5 * s))
                        t += 1
                row = prev.copy()
                row[10 + st] = w
                batch.append((i, h, mover, row))
        if not batch:
            continue
        uids = np.asarray(move_fn(np.stack([b[3] for b in batch]), np.array([b[2] for b in batch], np.int64), int(draws[d]),
                                  np.array([b[0] for b in batch], np.int64))).astype(np.int64)
        assert uids.shape == (len(batch),)
        for (i, h, _, _), uid in zip(batch, uids):
            h[3] = int(uid) == int(hmoves[d, i])
            h[2] += 1 if h[3] else 0
    seed, draw = int(seed) & _M64, int(draw) & _M64
    for i in range(m):
        if hands[i] is None:
            continue
        L, mine = depth_of[i], hands[i]
        for k in range(L + 1):
            out["mass"][k, i] = sum(h[1] for h in mine if h[2] >= k)
            out["n_hands"][k, i] = sum(1 for h in mine if h[2] >= k and h[1] > 0)
        used = max(k for k in range(L + 1) if k == 0 or out["mass"][k, i] > 0)
        out["depth_used"][i] = used
        out["fallback"][i] = 2 if L == 0 else 1 if used == 0 else 0
        for cards, mass, passed, _ in mine:
            for s, c in enumerate(cards):
                out["marg0"][i, s, c] += mass
                if passed >= used:
                    out["marg"][i, s, c] += mass
        T = int(out["mass"][used, i])
        if T == 0:
            continue
        rid = (int(first_row_id) + i) & _M64
        x = _philox_np(0x10000 + np.arange(R, dtype=np.uint64), draw & _M32, rid & _M32, rid >> 32, seed & _M32,
                       ((seed >> 32) ^ (draw >> 32)) & _M32)
        own = int(cur[i, 10 + st])
        for r in range(R):
            target = (((int(x[0][r]) << 32) | int(x[1][r])) * T) >> 64
            run = 0
            for cards, mass, passed, _ in mine:
                if passed >= used:
                    run += mass
                    if run > target:
                        w = own | 0x1FFFFFF
                        for s, c in enumerate(cards):
                            w = (w & ~(31 << (5 * s))) | (c << (5 * s))
                        out["hands"][i, r] = w
                        break
    if details:
        out["details"] = [None if h is None else [(x[0], x[1], x[2]) for x in h] for h in hands]
    return out
