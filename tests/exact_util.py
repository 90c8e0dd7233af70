"""What the exact-belief tests share (tests/test_belief_exact_cpu.py, tests/test_belief_exact_gpu.py; helper module).

  * `rule_games`: games of a named rule-list team (tests/playout_util.teams) played on the CPU oracle with the real keys — the
    rule walk of ply t is keyed (seed, t + 1, game id) exactly as tests/playout_util.oracle_playout keys it —, every ply's rows
    and moves, and an identity model of every hand (the deck position each card was dealt from), and `history_at`: one
    observer's partner history of depth D at a ply, in PartnerHistory's layout, from that model alone.
  * `oracle_move_fn`: belief_enumerate_ref's `move_fn` on the CPU RULE ORACLE. The oracle walks rules on its own env, not on a
    row, so the hypothetical state is REACHED: the game's deck with the observer's cards exchanged for the hand, replayed with
    the game's own moves up to the entry's ply. A hand that the current hints allow gets the same hints on the way, so the state
    reached is the spliced row word for word (asserted, the deck bytes aside, which no rule reads).
  * `brute_force`: the independent model of mass and marg0, by itertools.permutations of the physical pool elements.
  * `full2p`: the Full 2-player fixture of deep rows and the max_hands the tests run it with.

Nothing here touches the GPU or the library's kernels."""
import collections
import functools
import itertools

import numpy as np

import deep_rows as DR
from oracle import oracle_py as O
from playout_util import DEAL_SEED, rules_of, teams

Games = collections.namedtuple("Games", "cfg game players team rules seed first_game_id rows moves pos")


def deck_size(cfg):
    return cfg.colors * sum(3 if r == 0 else 1 if r == cfg.ranks - 1 else 2 for r in range(cfg.ranks))


def running(rows):
    return ((rows[..., 0] >> 19) & 3) == 0


def hand_n(row, p):
    return int((int(row[1]) >> (15 + 3 * p)) & 7)


def hand_cards(row, p, n=5):
    return [(int(row[10 + p]) >> (5 * s)) & 31 for s in range(n)]


def deck_bytes(cfg, row):
    return np.ascontiguousarray(np.asarray(row)[10 + 3 * cfg.players:], dtype="<u4").view(np.uint8)[:deck_size(cfg)].astype(np.int64)


@functools.lru_cache(maxsize=None)
def rule_games(game, players, team, n, seed=DEAL_SEED, first_game_id=0):
    """n oracle games of `team` played to the end: rows [T + 1, n, SW] uint32 (rows[t] = the export before ply t), moves [T, n]
    int32, pos[t][g][p] = the deck positions the cards of seat p's hand in rows[t] were dealt from, oldest first. Read only."""
    cfg = O.make_config(game, players, 0)
    env = O.OracleEnv(cfg, n, seed=seed, first_game_id=first_game_id)
    P, H = players, cfg.hand_size
    rules = [rules_of(r) for r in teams()[team](players)]
    rows, moves = [np.asarray(env.export_state()).astype(np.uint32).copy()], []
    now = [[list(range(p * H, (p + 1) * H)) for p in range(P)] for _ in range(n)]
    serial = [P * H] * n
    pos = [[tuple(tuple(h) for h in g) for g in now]]
    t = 0
    while running(rows[-1]).any():
        act, _ = env.rule_act(rules[t % P], seed, t + 1)
        env.step(act)
        cur = np.asarray(env.export_state()).astype(np.uint32).copy()
        for g in range(n):
            if not running(rows[-1][g]):
                continue
            u, mover = int(act[g]), t % P
            if u < 2 * H:
                del now[g][mover][u % H]
                if hand_n(cur[g], mover) == len(now[g][mover]) + 1:
                    now[g][mover].append(serial[g])
                    serial[g] += 1
            assert all(hand_n(cur[g], p) == len(now[g][p]) for p in range(P))
        moves.append(np.asarray(act, np.int32).copy())
        rows.append(cur)
        pos.append([tuple(tuple(h) for h in g) for g in now])
        t += 1
    assert env.illegal_count() == 0
    rows, moves = np.stack(rows), np.stack(moves)
    rows.setflags(write=False)
    moves.setflags(write=False)
    return Games(cfg, game, players, team, rules, seed, first_game_id, rows, moves, pos)


def history_at(G, t, depth, games=None):
    """The partner history of the seat to act at ply t (t % P), depth `depth`, newest first, for the games `games` (default
    all): dict(seat, cur [m, SW], rows [D, m, SW], moves [D, m] int32, alive [D, m] uint8, valid [D, m] uint8, draws [D],
    plies [D]). Entry d is the d-th latest ply before t that another seat made (an entry before the first ply is invalid and
    all zeros); alive bit s: the card in slot s of the observer's hand then is in its hand now; valid: the game was running
    before and after that ply."""
    P = G.players
    seat = t % P
    games = list(range(G.rows.shape[1])) if games is None else list(games)
    plies = [x for x in range(t - 1, -1, -1) if x % P != seat][:depth]
    m, SW = len(games), G.rows.shape[2]
    out = dict(seat=seat, cur=G.rows[t][games].copy(), rows=np.zeros((depth, m, SW), np.uint32), moves=np.zeros((depth, m), np.int32),
               alive=np.zeros((depth, m), np.uint8), valid=np.zeros((depth, m), np.uint8), draws=[0] * depth, plies=plies)
    for d, x in enumerate(plies):
        out["rows"][d] = G.rows[x][games]
        out["moves"][d] = G.moves[x][games]
        out["valid"][d] = running(G.rows[x][games]) & running(G.rows[x + 1][games])
        out["draws"][d] = x + 1
        for j, g in enumerate(games):
            held = set(G.pos[t][g][seat])
            out["alive"][d, j] = sum(1 << s for s, card in enumerate(G.pos[x][g][seat]) if card in held)
    return out


def oracle_move_fn(G, games, seat):
    """belief_enumerate_ref's move_fn for roots that are games `games` of G observed by `seat`, every entry's draw being its
    ply + 1 (history_at's): the CPU rule oracle on the state REACHED by replaying the game on a deck that deals the hypothetical
    hand. Asserts that the state reached is the row it was handed (every word before the deck)."""
    cfg, P = G.cfg, G.players
    D, W_DECK = deck_size(cfg), 10 + 3 * P

    def fn(rows, movers, draw, root):
        ply = int(draw) - 1
        out = np.zeros(len(rows), np.int32)
        for j in range(len(rows)):
            g = games[int(root[j])]
            deck = deck_bytes(cfg, G.rows[0][g]).copy()
            before = G.rows[ply][g]
            where = G.pos[ply][g][seat]
            undealt = list(range(D - int(before[0] & 63), D))
            pool = collections.Counter([int(deck[p]) for p in where] + [int(deck[q]) for q in undealt])
            hand = hand_cards(rows[j], seat, len(where))
            pool.subtract(hand)
            assert min(pool.values()) >= 0, "the hand is not made of pool cards"
            for s, p in enumerate(where):
                deck[p] = hand[s]
            for q, c in zip(undealt, sorted(pool.elements())):
                deck[q] = c
            env = O.OracleEnv(cfg, 1, seed=G.seed, first_game_id=G.first_game_id + g, decks=deck.astype(np.uint8)[None])
            for x in range(ply):
                env.step(G.moves[x][g:g + 1])
            state = np.asarray(env.export_state()).astype(np.uint32)[0]
            assert env.illegal_count() == 0 and np.array_equal(state[:W_DECK], np.asarray(rows[j], np.uint32)[:W_DECK]), (g, ply, hand)
            assert int(movers[j]) == (int(state[0]) >> 13) & 7
            act, _ = env.rule_act(G.rules[int(movers[j])], G.seed, int(draw))
            out[j] = act[0]
        return out

    return fn


def brute_force(cfg, row, seat):
    """The V0 belief of one running row by brute force: every permutation of the PHYSICAL pool elements (the seat's hand slots,
    then the undealt deck positions) into (slots, deck) in which every slot's card is plausible under its knowledge bits. ->
    (hands: Counter {cards tuple: arrangements}, slots: int64 [H, NC] arrangements with card c in slot s, arrangements per
    distinct choice of physical cards for the slots = (pool - n)!)."""
    P, H, Rk, NC = cfg.players, cfg.hand_size, cfg.ranks, cfg.colors * cfg.ranks
    n = min(hand_n(row, seat), H)
    deck, D = deck_bytes(cfg, row), deck_size(cfg)
    pool = hand_cards(row, seat, n) + [int(deck[q]) for q in range(D - min(int(row[0]) & 63, D), D)]
    know = int(row[10 + P + 2 * seat]) | int(row[10 + P + 2 * seat + 1]) << 32
    ok = [[c < NC and bool((know >> (12 * s + c // Rk)) & 1) and bool((know >> (12 * s + 5 + c % Rk)) & 1) for c in range(32)]
          for s in range(n)]
    hands, slots = collections.Counter(), np.zeros((H, NC), np.int64)
    for perm in itertools.permutations(range(len(pool))):
        cards = tuple(pool[perm[s]] for s in range(n))
        if all(ok[s][cards[s]] for s in range(n)):
            hands[cards] += 1
            for s in range(n):
                slots[s, cards[s]] += 1
    per_pick = 1
    for x in range(2, len(pool) - n + 1):
        per_pick *= x
    return hands, slots, per_pick


@functools.lru_cache(maxsize=None)
def late_rows(game, players=2, max_pool=8, take=6):
    """Up to `take` running rows of the deep corpus whose seat to act has a pool of 2 .. max_pool elements, spread over the
    corpus, and that seat per row."""
    c = DR.corpus(game, players)
    cfg = O.make_config(game, players, 0)
    idx = []
    for i in np.flatnonzero(c.running):
        row = c.rows[i]
        seat = (int(row[0]) >> 13) & 7
        if 2 <= hand_n(row, seat) + min(int(row[0]) & 63, deck_size(cfg)) <= max_pool:
            idx.append(i)
    idx = DR._spread(idx, take)
    rows = np.ascontiguousarray(c.rows[idx])
    return cfg, rows, [(int(r[0]) >> 13) & 7 for r in rows]


FULL2P_MAX_HANDS = 1 << 12


@functools.lru_cache(maxsize=None)
def full2p():
    """The Full 2-player fixture: the picked deep rows (tests/deep_rows.pick: cards to draw, empty decks, short hands, finished
    rows, a fresh deal), seen from seat 0, with FULL2P_MAX_HANDS. -> (cfg, rows [m, 32] uint32)."""
    return O.make_config("Hanabi-Full", 2, 0), np.ascontiguousarray(DR.pick("Hanabi-Full", 2).rows)
