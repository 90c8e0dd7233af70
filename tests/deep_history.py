"""Deep games of all twelve variants for the kernels that build the conditioned belief (helper module):
hb_belief_history_step, hb_belief_splice_alive / hb_belief_splice and hb_belief_score.

`play(game, players)` is the open-handed driver of tests/deep_play.py on the CPU oracle with a fifth of its moves random (rank
hints and hints past the next seat come only from the random share), every ply's exported rows AND the int32 moves handed to the
oracle. On top of it stands an identity model of every seat's hand in plain Python lists: every dealt card has a serial number, a
play or discard of slot s removes list element s, a draw appends. It knows nothing of masks, of 5-bit fields or of word 2; what it
reads of a row is the hand sizes of word 1, the deck count, the seat to act and the status bits. `Model` is one observer's
expected partner history of depth D after every call of `SearchPlayer`'s protocol, generalised to P seats:

  * at a ply the observer itself made, one call with `own_moves` only (-1 where the game was over: nobody moved);
  * at every other ply, one call with the push only (cur = the rows after the ply, prev = the rows before it).

Nothing here touches the GPU or the library's kernels."""
import collections
import functools

import numpy as np

import deep_rows as DR
from deep_play import VARIANTS, open_hand_moves   # noqa: F401  (VARIANTS: re-exported for the tests)
from oracle import oracle_py as O

P_RAND = 0.2
DEPTHS = (1, 8)

Play = collections.namedtuple("Play", "rows moves hands")


def running(rows):
    return ((rows[..., 0] >> 19) & 3) == 0


def seat_of(rows):
    return ((rows[..., 0] >> 13) & 7).astype(np.int64)


def deck_of(rows):
    return (rows[..., 0] & 63).astype(np.int64)


def hand_n(rows, p):
    return ((rows[..., 1] >> (15 + 3 * p)) & 7).astype(np.int64)


def _identity(cfg, rows, moves):
    """hands[t][g][p]: the serial numbers seat p of game g holds in rows[t], oldest first (tuples). The oracle's rows decide
    whether a card was drawn: the mover's hand size in word 1 after the ply, checked against the deck count."""
    T, N = moves.shape
    P, H = cfg.players, cfg.hand_size
    now = [[list(range(p * H, (p + 1) * H)) for p in range(P)] for _ in range(N)]
    serial = [P * H] * N
    for g in range(N):
        assert all(int(hand_n(rows[0, g], p)) == H for p in range(P))
    hands = [[tuple(tuple(h) for h in game) for game in now]]
    for t in range(T):
        for g in range(N):
            prev, cur = rows[t, g], rows[t + 1, g]
            if running(prev):
                mover, u = int(seat_of(prev)), int(moves[t, g])
                assert mover == t % P, "a running game is at the same ply as every other (no re-deal: flags 0)"
                if u < 2 * H:   # uids 0 .. H - 1 discard slot u, H .. 2H - 1 play slot u - H
                    del now[g][mover][u if u < H else u - H]
                    drew = int(hand_n(cur, mover)) == len(now[g][mover]) + 1
                    if drew:
                        now[g][mover].append(serial[g])
                        serial[g] += 1
                    assert int(deck_of(cur)) == int(deck_of(prev)) - (1 if drew else 0)
                else:
                    assert int(deck_of(cur)) == int(deck_of(prev))
            else:
                assert not running(cur) and np.array_equal(prev, cur), "a finished game stays as it is"
            assert all(int(hand_n(cur, p)) == len(now[g][p]) for p in range(P)), (t, g)
        hands.append([tuple(tuple(h) for h in game) for game in now])
    return hands


@functools.lru_cache(maxsize=None)
def play(game, players):
    """48 oracle games (seed 9, flags 0) driven for deep_rows.STEPS plies by `open_hand_moves` with default_rng(4) and 20 % random
    moves: rows [T + 1, 48, SW] uint32 (rows[t] = the export before ply t), moves [T, 48] int32 (what the oracle was handed; 0 in
    a finished game, which ignores it) and hands, the identity model. Read only: shared."""
    cfg = O.make_config(game, players, 0)
    env = O.OracleEnv(cfg, DR.N_GAMES, seed=DR.ENV_SEED)
    legal, rng = env.observe()["legal"], np.random.default_rng(DR.RNG_SEED)
    rows, moves = [np.asarray(env.export_state()).astype(np.uint32).copy()], []
    for _ in range(DR.STEPS[game]):
        mv = np.asarray(open_hand_moves(cfg, rows[-1], legal, rng, P_RAND), np.int32).copy()
        legal = env.step(mv)["legal"]
        moves.append(mv)
        rows.append(np.asarray(env.export_state()).astype(np.uint32).copy())
    assert env.illegal_count() == 0
    rows, moves = np.stack(rows), np.stack(moves)
    assert not running(rows[-1]).any(), "a game is still running after STEPS plies"
    rows.setflags(write=False)
    moves.setflags(write=False)
    return Play(rows, moves, _identity(cfg, rows, moves))


def config(game, players):
    return O.make_config(game, players, 0)


class Model:
    """One observer's expected partner history of depth D, from zeros, advanced call by call: `rows` [D, N, SW] uint32, `moves`
    [D, N] int32, `alive` and `valid` [D, N] uint8 as PartnerHistory keeps them, and `stored[d][g]`, the serials of the observer's
    hand in rows[d][g] (() for an entry never pushed).

        for call in model.calls():   # call: dict(t, own, cur, prev); own [N] int32 or None, cur / prev [N, SW] uint32 or None
            ...                      # model.rows / moves / alive / valid are the state AFTER that call; model.now = rows[t + 1]

    rows[0] = the export before the ply; moves[0] = the move the driver made, where cur's word 2 has its valid bit set, else -1
    (of a game that was over before the ply: the last move made in it, which is what its rows go on recording); alive[d] bit s =
    the serial in slot s of the stored hand is in the observer's hand now; valid[0] = prev running and cur running."""

    def __init__(self, game, players, seat, depth):
        self.play, self.cfg, self.seat, self.depth = play(game, players), config(game, players), int(seat), int(depth)
        T, N = self.play.moves.shape
        SW = self.play.rows.shape[2]
        self.rows = np.zeros((depth, N, SW), np.uint32)
        self.moves = np.zeros((depth, N), np.int32)
        self.alive = np.zeros((depth, N), np.uint8)
        self.valid = np.zeros((depth, N), np.uint8)
        self.stored = [[()] * N for _ in range(depth)]
        self.now, self.t = self.play.rows[0], -1

    def calls(self):
        pl, P, D, o = self.play, self.cfg.players, self.depth, self.seat
        T, N = pl.moves.shape
        last = np.full(N, -1, np.int32)   # the last move made in each game
        for t in range(T):
            prev, cur = pl.rows[t], pl.rows[t + 1]
            last = np.where(running(prev), pl.moves[t], last).astype(np.int32)
            if t % P == o:
                call = dict(t=t, own=np.where(running(prev), pl.moves[t], -1).astype(np.int32), cur=None, prev=None)
            else:
                call = dict(t=t, own=None, cur=cur, prev=prev)
                for a in (self.rows, self.moves, self.valid):
                    a[1:] = a[:-1].copy()
                self.stored = [[h[o] for h in pl.hands[t]]] + self.stored[:-1]
                self.rows[0] = prev
                self.moves[0] = np.where((cur[:, 2] & 1) != 0, last, -1)
                self.valid[0] = running(prev) & running(cur)
            for g in range(N):
                held = set(pl.hands[t + 1][g][o])
                for d in range(D):
                    self.alive[d, g] = sum(1 << s for s, card in enumerate(self.stored[d][g]) if card in held)
            self.now, self.t = cur, t
            yield call


def move_kind(cfg, uid):
    """(kind, offset) of a move uid: kind 'discard' / 'play' / 'colour' / 'rank'; offset = how many seats after
    the mover a hint's target sits (1: the next seat), 0 for a card move."""
    H, P, C, R = cfg.hand_size, cfg.players, cfg.colors, cfg.ranks
    if uid < H:
        return "discard", 0
    if uid < 2 * H:
        return "play", 0
    if uid < 2 * H + (P - 1) * C:
        return "colour", (uid - 2 * H) // C + 1
    return "rank", (uid - 2 * H - (P - 1) * C) // R + 1


@functools.lru_cache(maxsize=None)
def counts(game, players):
    """What the corpus reaches. Over the valid pushes (a ply with prev and cur both running): `rank` hints, `rank_far` and
    `colour_far` (hints to a seat other than the next one), `short_observer` (the seats other than the mover that hold a short hand
    in prev: the pushes a short-handed observer sees), `deck0` (prev has nothing left to draw). Over all observers' histories of depth 8, after every call, the valid
    entries: `dead` (at least one slot of the stored hand has left the observer's hand) and `short_stored` (the stored hand is
    short). `finished_push`: the plies whose prev is running and whose cur is finished."""
    pl, cfg = play(game, players), config(game, players)
    P, H = cfg.players, cfg.hand_size
    T, N = pl.moves.shape
    c = dict.fromkeys(("rank", "rank_far", "colour_far", "short_observer", "deck0", "dead", "short_stored", "finished_push"), 0)
    for t in range(T):
        prev, cur = pl.rows[t], pl.rows[t + 1]
        ok = running(prev) & running(cur)
        c["finished_push"] += int((running(prev) & ~running(cur)).sum())
        for g in np.flatnonzero(ok):
            kind, off = move_kind(cfg, int(pl.moves[t, g]))
            c["rank"] += kind == "rank"
            c["rank_far"] += kind == "rank" and off >= 2
            c["colour_far"] += kind == "colour" and off >= 2
            c["short_observer"] += sum(len(pl.hands[t][g][p]) < H for p in range(P) if p != t % P)
            c["deck0"] += int(deck_of(prev[g])) == 0
    for seat in range(P):
        m = Model(game, players, seat, 8)
        for _ in m.calls():
            for d, g in zip(*np.nonzero(m.valid)):
                n = len(m.stored[d][g])
                c["dead"] += int(m.alive[d, g]) != (1 << n) - 1
                c["short_stored"] += n < H
    return {k: int(v) for k, v in c.items()}


@functools.lru_cache(maxsize=None)
def splice_plies(game, players):
    """The three plies at which the splice tests take the histories: the ply of the first push on an empty deck, the ply before
    which the most (game, seat) pairs of running games hold a short hand (the first such ply), and one mid-game ply: a third of
    the way to the first of the other two, but at least two rounds of the table in, or half-way through the plies that push
    anything where the games are shorter than that (Very-Small with 5 players: one round, ply 1)."""
    pl, cfg = play(game, players), config(game, players)
    T = pl.moves.shape[0]
    ok = [running(pl.rows[t]) & running(pl.rows[t + 1]) for t in range(T)]
    first0 = next(t for t in range(T) if (ok[t] & (deck_of(pl.rows[t]) == 0)).any())
    short = [sum(int((running(pl.rows[t]) & (hand_n(pl.rows[t], p) < cfg.hand_size)).sum()) for p in range(cfg.players)) for t in range(T)]
    most = int(np.argmax(short))
    pushing = sum(1 for t in range(T) if ok[t].any())
    mid = max(min(first0, most) // 3, min(2 * cfg.players, (pushing - 1) // 2))
    return tuple(sorted({mid, first0, most}))
