"""Per-game models of the two score tallies and the crafted steps they are held to (helper module).

`eval_tally_model` restates hb_eval_tally (csrc/eval.hip) and `train_tally_model` / `train_tally_init_model` restate hb_train_tally
and hb_train_tally_init (csrc/train_tally.hip) from the contract in include/hanabi_hip.h: one game after another, plain Python
integers, no wavefront, no ballot, no workgroup. They are a third statement beside the kernels and the numpy recount of
tests/test_partner_pool_gpu.py and share nothing with either.

`crafted_steps` is what played games cannot give: it chooses what sits in every lane of every wavefront. Uids from [-2, A + 2)
with every move kind, rewards from {+1, 0, -s}, endings at every score, endings with and without lives left, misplays that end
nothing, games finished (or never armed) beforehand, and whole wavefronts set to one pattern. tests/test_tally_model_cpu.py
holds its coverage to conditions on the models' output, so it cannot quietly stop reaching a case.

`wrong=` selects one deliberate mistake of a model (WRONG); only the teeth of tests/test_tally_model_cpu.py pass it.
"""
import collections

import numpy as np

Dims = collections.namedtuple("Dims", "P H C R A max_life B max_info deck")

VARIANTS = [("Hanabi-Full", 2), ("Hanabi-Full", 5), ("Hanabi-Small", 3), ("Hanabi-Very-Small", 4)]   # B = 26, 26, 11, 6
WRONG = ("sq_is_sum", "misplay_lt", "bomb_gt", "rank_boundary_by_ranks", "seat_stride_5")
TILE = 128          # games per pool tile (hb_train_tally)
UNARMED = 0x80


def dims_of(cfg):
    """The numbers the tallies depend on, from an hb_config (the oracle's or the library's). Deck: 3 + 2 (R - 2) + 1 cards of a
    colour; moves (App. A.2 order): H discards, H plays, (P - 1) C colour hints, (P - 1) R rank hints."""
    P, H, C, R = cfg.players, cfg.hand_size, cfg.colors, cfg.ranks
    return Dims(P, H, C, R, 2 * H + (P - 1) * (C + R), cfg.max_life, C * R + 1, cfg.max_info, C * (3 + 2 * (R - 2) + 1))


def eval_counters(d):
    return 2 + d.B + 5 * d.P


def train_counters(d):
    return 6 + d.B + 5 * d.P


def move_kind(d, uid, wrong=None):
    """0 discard, 1 play, 2 reveal colour, 3 reveal rank; None: the uid is no move."""
    uid = int(uid)
    if uid < 0 or uid >= d.A:
        return None
    if uid < d.H:
        return 0
    if uid < 2 * d.H:
        return 1
    n_colour_hints = (d.P - 1) * (d.R if wrong == "rank_boundary_by_ranks" else d.C)
    return 2 if uid < 2 * d.H + n_colour_hints else 3


def _clamp_bin(d, score):
    return min(max(int(score), 0), d.B - 1)


def _is_misplay(kind, reward, wrong):
    return kind == 1 and (float(reward) < 0 if wrong == "misplay_lt" else float(reward) <= 0)


def _is_bomb(d, lost, wrong):
    return lost > d.max_life if wrong == "bomb_gt" else lost >= d.max_life


def eval_tally_model(d, seat, turn, actions, reward, terminal, score, done, final_score, length, counters, wrong=None):
    """One hb_eval_tally call -> the new (done, final_score, length, counters); counters a list of Python ints."""
    done, final_score, length = np.array(done, np.uint8), np.array(final_score, np.int8), np.array(length, np.int16)
    c = [int(x) for x in counters]
    stride = 5 if wrong == "seat_stride_5" else 4
    moves0, mis0 = 2 + d.B, 2 + d.B + 4 * d.P
    for g in range(len(done)):
        st = int(done[g])
        if st & 0x80:
            continue
        kind = move_kind(d, actions[g], wrong)
        mis = _is_misplay(kind, reward[g], wrong)
        lost = (st & 0x7F) + (1 if mis else 0)
        if kind is not None:
            c[moves0 + stride * seat + kind] += 1
        if mis:
            c[mis0 + seat] += 1
        if terminal[g] != 0:
            c[0] -= 1
            c[1 + _clamp_bin(d, score[g])] += 1
            if _is_bomb(d, lost, wrong):
                c[1 + d.B] += 1
            final_score[g], length[g], done[g] = int(score[g]), turn + 1, 0x80 | lost
        elif mis:
            done[g] = lost
    return done, final_score, length, c


def train_tally_model(d, seat, actions, reward, terminal, score, tile_member, n_members, lost, length, counters, wrong=None, log=None):
    """One hb_train_tally call -> the new (lost, length, counters); counters [n_members] lists of Python ints. `log`, a Counter,
    collects what the call met (the generator's coverage; no part of the contract)."""
    lost, length = np.array(lost, np.uint8), np.array(length, np.int16)
    c = [[int(x) for x in row] for row in counters]
    stride = 5 if wrong == "seat_stride_5" else 4
    B = d.B
    for g in range(len(lost)):
        m = int(tile_member[g // TILE])
        if m < 0 or m >= n_members:
            continue
        row = c[m]
        kind = move_kind(d, actions[g], wrong)
        mis = _is_misplay(kind, reward[g], wrong)
        st = int(lost[g])
        armed = not st & UNARMED
        lives = (st & 0x7F) + (1 if mis else 0)
        moves = int(length[g]) + 1
        if kind is not None:
            row[6 + B + stride * seat + kind] += 1
        if mis:
            row[6 + B + 4 * d.P + seat] += 1
        if terminal[g] != 0:
            b = _clamp_bin(d, score[g])
            row[0] += 1
            row[1] += b
            row[2] += b if wrong == "sq_is_sum" else b * b
            row[3 + b] += 1
            if armed:
                row[5 + B] += 1
                row[4 + B] += moves
                if _is_bomb(d, lives, wrong):
                    row[3 + B] += 1
            lost[g], length[g] = 0, 0
        elif armed:
            lost[g], length[g] = lives, moves
        if log is not None:
            ended = terminal[g] != 0
            log["out_of_range"] += kind is None
            log["misplay_live"] += mis and not ended
            log["end_unarmed"] += ended and not armed
            log["end_bomb"] += ended and armed and lives >= d.max_life
            log["end_lives_left"] += ended and armed and lives < d.max_life
            log["end_exact"] += ended and armed and mis and lives == d.max_life
            log["longest"] = max(log["longest"], moves if ended and armed else 0)
    return lost, length, c


def train_tally_init_model(d, rows):
    """hb_train_tally_init on state rows [n, SW] (layout: DESIGN.md section 3) -> (lost, length): a game is armed at the first
    move of a deal, i.e. with the deck less the hands, every information token, no firework and no discard."""
    rows = np.asarray(rows)
    lost, length = np.zeros(len(rows), np.uint8), np.zeros(len(rows), np.int16)
    for g, row in enumerate(rows):
        w0, w1 = int(row[0]), int(row[1])
        fireworks = sum((w1 >> (3 * col)) & 7 for col in range(5))
        dealt = (w0 & 63 == d.deck - d.P * d.H and (w0 >> 6) & 15 == d.max_info and fireworks == 0 and int(row[8]) == 0 and int(row[9]) == 0)
        lost[g] = 0 if dealt else UNARMED
    return lost, length


# ---- crafted steps -------------------------------------------------------------------------------------------------------------

Crafted = collections.namedtuple("Crafted", "steps done0 lost0 length0 schedule")


def _uid_of_kind(d, kind, r):
    lo = (0, d.H, 2 * d.H, 2 * d.H + (d.P - 1) * d.C)[kind]
    hi = (d.H, 2 * d.H, 2 * d.H + (d.P - 1) * d.C, d.A)[kind]
    return lo + int(r) % (hi - lo)


def wave_schedule(n):
    """{(turn, wave): pattern} for the waves n games have. Wave 0: nobody ends and every lane misplays, then only lane 0 ends,
    then only lane 63. Wave 1 (if there is one): lane l ends at score l mod B on turn 0. Wave 2 (else 0): every lane still live
    ends on one score on turn 3 and so is finished before turn 4. With one wave the B-scores pattern takes turn 3."""
    nw = (n + 63) // 64
    s = {(0, 0): "all_misplay", (1, 0): "lane0", (2, 0): "lane63"}
    s[(0, 1) if nw > 1 else (3, 0)] = "distinct"
    s.setdefault((3, 2 % nw), "same")
    s.setdefault((4, 2 % nw), "finished")
    return s


def crafted_steps(d, n, turns, seed, p_end=0.2):
    """`turns` steps of n games and their initial per-game state, seeded and deterministic. Returns Crafted(steps, done0, lost0,
    length0, schedule): steps[t] = dict(actions int32, reward float32, terminal int8, score int8); done0 is hb_eval_tally's
    status byte, lost0 / length0 are hb_train_tally's (low bits shared). Scores stay in 0 .. B-1.

    A wave with an all-lanes-end pattern is kept live until then: no status bit 7 at the start, no ending before its turn."""
    rng = np.random.default_rng(seed)
    B, A = d.B, d.A
    sched = wave_schedule(n)
    low = rng.choice(np.array([0, 1, 2], np.uint8), n, p=[0.6, 0.25, 0.15])
    done0 = np.where(rng.random(n) < 0.12, low | 0x80, low).astype(np.uint8)
    lost0 = np.where(rng.random(n) < 0.25, np.minimum(low, 1) | UNARMED, low).astype(np.uint8)           # {0, 1, 2, 0x80, 0x81}
    length0 = rng.integers(0, 60, n).astype(np.int16)
    near = rng.random(n) < 0.1
    length0[near] = 32767 - turns - rng.integers(0, 3, int(near.sum()))                                    # never past int16 in `turns` steps
    keep_live = {}                                                                                          # wave -> first turn it may end on
    for (t, w), what in sched.items():
        if what in ("distinct", "same"):
            keep_live[w] = t
            done0[64 * w:64 * w + 64] &= 0x7F
    done0[0] &= 0x7F                                                                                        # lanes 0 and 63 of wave 0 are
    done0[min(n - 1, 63)] &= 0x7F                                                                           # live when their turn comes
    if turns >= 2:
        length0[0], lost0[0] = 32765, 0                                                                     # ends on turn 1 at length 32 767
    lives = low.astype(np.int64)                                                                            # the generator's own count
    steps = []
    for t in range(turns):
        act, rew = np.zeros(n, np.int32), np.zeros(n, np.float32)
        term, score = np.zeros(n, np.int8), np.zeros(n, np.int8)
        u = rng.random((n, 5))
        r = rng.integers(0, 1 << 30, (n, 3))
        for g in range(n):
            w, lane = divmod(g, 64)
            what = sched.get((t, w))
            kind = int(r[g, 0]) % 4
            if what == "all_misplay":
                kind = 1
            act[g] = _uid_of_kind(d, kind, r[g, 1])
            if u[g, 0] < 0.06 and what is None:
                act[g] = (-2, -1, A, A + 1)[int(r[g, 1]) % 4]
                kind = None
            s = int(r[g, 2]) % B if u[g, 1] < 0.5 else (5 * g + 3 * t) % B                                  # the score, should it end
            mis = False
            if kind == 1:
                if what == "all_misplay" or u[g, 2] < 0.6:
                    mis = True
                    rew[g] = 0.0 if u[g, 3] < 0.5 else -float(1 + int(r[g, 2]) % (B - 1))
                else:
                    rew[g] = 1.0
            elif u[g, 2] < 0.1:
                rew[g] = -float(1 + int(r[g, 2]) % (B - 1))                                                 # (no play: no misplay)
            ends = u[g, 4] < (0.7 if mis and lives[g] + 1 == d.max_life else p_end)
            if mis and ends and u[g, 3] < 0.75:
                s = 0                                                                                       # as the env reports a bomb-out
            if what == "all_misplay":
                ends = False
            elif what == "lane0":
                ends = lane == 0
            elif what == "lane63":
                ends = lane == 63
            elif what == "distinct":
                ends, s = True, lane % B
            elif what == "same":
                ends, s = True, (7 * w + 3) % B
            elif t < keep_live.get(w, 0):
                ends = False
            term[g], score[g] = ends, s
            lives[g] = 0 if ends else lives[g] + mis
        steps.append(dict(actions=act, reward=rew, terminal=term, score=score))
    return Crafted(steps, done0, lost0, length0, sched)


def eval_run(d, cr, turn0=0, counters0=None, wrong=None):
    """The eval model over the crafted steps (seat = turn mod P; final_score and length start at -1): yields (t, done,
    final_score, length, counters) after every turn."""
    n = len(cr.done0)
    done, final, length = cr.done0.copy(), np.full(n, -1, np.int8), np.full(n, -1, np.int16)
    c = [int((cr.done0 & 0x80 == 0).sum())] + [0] * (eval_counters(d) - 1) if counters0 is None else list(counters0)
    for t, s in enumerate(cr.steps):
        done, final, length, c = eval_tally_model(d, (turn0 + t) % d.P, turn0 + t, s["actions"], s["reward"], s["terminal"], s["score"],
                                                  done, final, length, c, wrong=wrong)
        yield t, done, final, length, c


def train_run(d, cr, tile_member, n_members, seat0=0, counters0=None, wrong=None, log=None):
    """The training model over the crafted steps (seat = (seat0 + t) mod P): yields (t, lost, length, counters) after every step."""
    lost, length = cr.lost0.copy(), cr.length0.copy()
    c = [[0] * train_counters(d) for _ in range(n_members)] if counters0 is None else counters0
    for t, s in enumerate(cr.steps):
        lost, length, c = train_tally_model(d, (seat0 + t) % d.P, s["actions"], s["reward"], s["terminal"], s["score"], tile_member,
                                            n_members, lost, length, c, wrong=wrong, log=log)
        yield t, lost, length, c


def score_counter_row(d, scores, lengths=(), bombouts=0):
    """A counter row of hb_train_tally made from an explicit list of final scores (and the lengths of the tracked ones)."""
    row = [0] * train_counters(d)
    for s in scores:
        row[0] += 1
        row[1] += s
        row[2] += s * s
        row[3 + s] += 1
    row[3 + d.B], row[4 + d.B], row[5 + d.B] = bombouts, sum(lengths), len(lengths)
    return row
