"""Deep, high-scoring games for the env / encoder / rule tests (helper module).

Uniform-random legal play loses a game of Hanabi-Full to three misplays within about fifteen moves: the deck never runs out,
no stack is completed, the fireworks never pass 7 of 25. `open_hand_moves` is an open-handed driver: it looks at its own
cards in the exported state rows and plays what is playable, so the games it drives reach what a trained agent and the search
roll-outs live in: empty decks, short hands, completed stacks, the final round with points on the board, the max-score ending
and the re-deals out of them. It is numpy / plain Python over state rows (layout: DESIGN.md section 3) and the only source of
moves of the deep-play tests: the same int32 array goes to the oracle and to the HIP env.

`Tally` counts what a run reached, from the oracle's outputs alone; tests/test_deep_play_cpu.py holds it to floors, so the
corpus cannot quietly stop reaching these states.
"""
import numpy as np

from oracle import oracle_py as O

FLAGS = O.FLAG_AUTO_RESET | O.FLAG_RESET_START_NEXT
N_GAMES = 130          # two waves and a partial one at every games-per-wave (8, 16, 32, 64)
P_RAND = 0.05
SEED = 5
FIRST_GAME_ID = 12345
RULE_SEED = 77
STEPS = {"Hanabi-Full": 200, "Hanabi-Small": 80, "Hanabi-Very-Small": 60}


def steps_of(game, players):
    """Length of a variant's run. Five players lose three lives to the driver's 5 % of random moves so rarely (a random move is
    a play one time in ten) that the first score-0 endings of Hanabi-Full fall at steps 679, 956 and 994: that run is
    lengthened to keep the corpus' floor of one such ending with some room."""
    return 1000 if (game, players) == ("Hanabi-Full", 5) else STEPS[game]


VARIANTS = [(g, p) for g in ("Hanabi-Full", "Hanabi-Small", "Hanabi-Very-Small") for p in (2, 3, 4, 5)]

# the single-rule lists, (kind, arg, threshold); kinds as in include/hanabi_hip.h (HB_RULE_*)
RULES = ([(k, 0, 0.0) for k in (0, 1, 2, 3, 4, 5, 6, 7)] + [(8, 8, 0.0), (8, 3, 0.0), (9, 0, 0.0)] +
         [(10, 0, 0.6), (10, 1, 0.8), (10, 0, 0.25), (11, 0, 0.9), (11, 0, 0.5)] + [(k, 0, 0.0) for k in (12, 13, 14, 15)])
HAIL_MARY = 12
NEED_LIVES = (10, 1, 0.8)   # play_probably_safe(0.8, needs more than one life)


def fields(cfg, rows):
    """The scalar fields of state rows [n, SW] uint32 as int64 arrays."""
    r = np.asarray(rows).astype(np.int64)
    n, P = r.shape[0], cfg.players
    d = dict(deck=r[:, 0] & 63, info=(r[:, 0] >> 6) & 15, life=(r[:, 0] >> 10) & 7, seat=(r[:, 0] >> 13) & 7)
    d["fireworks"] = np.stack([(r[:, 1] >> (3 * c)) & 7 for c in range(cfg.colors)], axis=1)
    d["hand_n"] = np.stack([(r[:, 1] >> (15 + 3 * p)) & 7 for p in range(P)], axis=1)
    d["cards"] = np.stack([np.stack([(r[:, 10 + p] >> (5 * i)) & 31 for i in range(cfg.hand_size)], axis=1) for p in range(P)], axis=1)
    d["own_n"] = d["hand_n"][np.arange(n), d["seat"]]
    d["own"] = d["cards"][np.arange(n), d["seat"]]
    return d


def _first(mask):
    """Index of the first True of every row of `mask`, -1 where there is none."""
    return np.where(mask.any(1), mask.argmax(1), -1)


def open_hand_moves(cfg, rows, legal, rng, p_rand):
    """One move uid per game, int32 [n]. The first rule that applies decides:
      1. no legal move: 0;
      2. with probability p_rand a uniform legal move;
      3. the lowest own slot whose card is playable: play it;
      4. below max_info: the lowest own slot whose card is already played or held twice in the own hand: discard it;
      5. with a token left: the lowest legal hint;
      6. below max_info: discard the slot of highest rank that is not the top rank (the lowest such slot);
      7. the lowest legal uid.
    The draws of `rng` are part of the definition: games in order, one rng.random() per game that has a legal move, then one
    rng.choice over its legal uids when that fell below p_rand."""
    legal = np.asarray(legal) != 0
    n, hs, R = legal.shape[0], cfg.hand_size, cfg.ranks
    f = fields(cfg, rows)
    held = np.arange(hs)[None, :] < f["own_n"][:, None]
    colour, rank = np.minimum(f["own"] // R, cfg.colors - 1), f["own"] % R
    pile = np.take_along_axis(f["fireworks"], colour, axis=1)
    twice = (f["own"][:, :, None] == f["own"][:, None, :]) & held[:, :, None] & held[:, None, :] & ~np.eye(hs, dtype=bool)[None]
    may_discard = (f["info"] < cfg.max_info)[:, None]
    play = _first(held & (rank == pile))
    dead = _first(held & may_discard & ((rank < pile) | twice.any(2)))
    hint = _first(legal[:, 2 * hs:] & (f["info"] > 0)[:, None])
    spare = held & may_discard & (rank < R - 1)
    high = _first(spare & (rank == np.where(spare, rank, -1).max(1, keepdims=True)))
    move = np.where(play >= 0, hs + play, np.where(dead >= 0, dead, np.where(hint >= 0, 2 * hs + hint, np.where(high >= 0, high, _first(legal)))))
    move = np.where(legal.any(1), move, 0).astype(np.int32)
    for g in range(n):
        if legal[g].any() and rng.random() < p_rand:
            move[g] = rng.choice(np.flatnonzero(legal[g]))
    return move


class Tally:
    """What a run reached. `step` takes the oracle's state rows before a move, the moves, its step outputs and the rows after."""

    def __init__(self, cfg):
        self.cfg = cfg
        self.max_score = cfg.colors * cfg.ranks
        self.end_max = self.end_deck_empty_scored = self.end_zero = 0
        self.deck0_states = self.info0_states = self.short_hand_states = 0
        self.max_fireworks = 0
        self.completed_with_token = self.completed_without_token = 0
        self.episodes = self.score_sum = 0

    def state(self, rows):
        f = fields(self.cfg, rows)
        self.deck0_states += int((f["deck"] == 0).sum())
        self.info0_states += int((f["info"] == 0).sum())
        self.short_hand_states += int((f["hand_n"] < self.cfg.hand_size).any(1).sum())
        self.max_fireworks = max(self.max_fireworks, int(f["fireworks"].sum(1).max()))

    def step(self, before, act, out, after):
        cfg, hs = self.cfg, self.cfg.hand_size
        b = fields(cfg, before)
        term, score = out["terminal"] != 0, out["score"].astype(np.int64)
        self.end_max += int((term & (score == self.max_score)).sum())
        self.end_deck_empty_scored += int((term & (b["deck"] == 0) & (score > 0) & (score < self.max_score)).sum())
        self.end_zero += int((term & (score == 0)).sum())
        self.episodes += int(term.sum())
        self.score_sum += int(score[term].sum())
        self.max_fireworks = max(self.max_fireworks, int(score.max()))
        # a play of the top rank onto its stack completes it; the token comes back unless all of them are there
        act = np.asarray(act)
        slot = np.clip(act - hs, 0, hs - 1)
        card = b["own"][np.arange(len(act)), slot]
        is_play = (act >= hs) & (act < 2 * hs) & (slot < b["own_n"])
        pile = b["fireworks"][np.arange(len(act)), np.minimum(card // cfg.ranks, cfg.colors - 1)]
        done = is_play & (card % cfg.ranks == cfg.ranks - 1) & (pile == cfg.ranks - 1)
        self.completed_with_token += int((done & (b["info"] < cfg.max_info)).sum())
        self.completed_without_token += int((done & (b["info"] == cfg.max_info)).sum())
        # where the game goes on, the row's last-move word says the same of a play: scored (bit 18), token returned (bit 19)
        last = np.asarray(after)[:, 2].astype(np.int64)
        live = ~term & is_play
        assert np.array_equal(((last >> 18) & 1 == 1)[live], (card % cfg.ranks == pile)[live])
        assert np.array_equal(((last >> 19) & 1 == 1)[live], (done & (b["info"] < cfg.max_info))[live])
        self.state(after)

    def as_dict(self):
        return {k: v for k, v in vars(self).items() if isinstance(v, int)}


def sections(cfg, deck_size):
    """Start of every section of the observation, and its length."""
    P, hs, bits = cfg.players, cfg.hand_size, cfg.colors * cfg.ranks
    s = dict(hands=0)
    s["flags"] = (P - 1) * hs * bits
    s["deck"] = s["flags"] + P
    s["fireworks"] = s["deck"] + deck_size - P * hs
    s["info"] = s["fireworks"] + bits
    s["life"] = s["info"] + cfg.max_info
    s["discards"] = s["life"] + cfg.max_life
    s["last"] = s["discards"] + deck_size
    s["last_scored"] = s["last"] + P + 4 + P + cfg.colors + cfg.ranks + hs + hs + bits
    s["knowledge"] = s["last_scored"] + 2
    s["end"] = s["knowledge"] + P * hs * (bits + cfg.colors + cfg.ranks)
    return s


def check_states(cfg, deck_size, rows, obs):
    """Card conservation on the raw rows and the structure of the observation of every game, all
    games at once: every section that restates the state row says what the row says, for the seat to act."""
    r = np.asarray(rows).astype(np.int64)
    o = np.asarray(obs).astype(np.int64)
    n, P, hs, R, Cc = r.shape[0], cfg.players, cfg.hand_size, cfg.ranks, cfg.colors
    bits = Cc * R
    f = fields(cfg, rows)
    s = sections(cfg, deck_size)
    assert o.shape[1] == s["end"] and set(np.unique(o)) <= {0, 1}
    assert (f["info"] <= cfg.max_info).all() and (f["life"] <= cfg.max_life).all() and (f["life"] >= 1).all()
    assert (f["hand_n"] <= hs).all() and (f["hand_n"] >= hs - 1).all() and (f["fireworks"] <= R).all()
    copies = np.array([3 if k == 0 else (1 if k == R - 1 else 2) for k in range(R)] * Cc)
    # conservation: hands + discards + fireworks + the rest of the deck = the whole deck, card identity by identity
    cnt = np.zeros((n, bits), np.int64)
    held = np.arange(hs)[None, None, :] < f["hand_n"][:, :, None]
    for p in range(P):
        for i in range(hs):
            ok = held[:, p, i]
            assert (f["cards"][ok, p, i] < bits).all() and (f["cards"][~ok, p, i] == 31).all()
            np.add.at(cnt, (np.flatnonzero(ok), f["cards"][ok, p, i]), 1)
    disc = np.unpackbits(np.ascontiguousarray(np.asarray(rows)[:, 8:10]).view(np.uint8).reshape(n, 8), axis=1, bitorder="little")
    assert not disc[:, deck_size:].any()
    pos = 0
    for k in range(bits):
        th = disc[:, pos:pos + copies[k]].astype(np.int64)
        assert (np.diff(th, axis=1) <= 0).all()                       # a thermometer
        cnt[:, k] += th.sum(1)
        pos += copies[k]
    for c in range(Cc):
        for k in range(R):
            cnt[:, c * R + k] += f["fireworks"][:, c] > k
    deck = np.ascontiguousarray(np.asarray(rows)[:, 10 + 3 * P:]).view(np.uint8).reshape(n, -1)[:, :deck_size]
    for k in range(deck_size):
        ok = k >= deck_size - f["deck"]
        np.add.at(cnt, (np.flatnonzero(ok), deck[ok, k]), 1)
    assert (cnt == copies[None]).all(), "cards are not conserved"
    # the observation of the seat to act
    g = np.arange(n)
    for rel in range(1, P):
        who = (f["seat"] + rel) % P
        for i in range(hs):
            want = np.zeros((n, bits), np.int64)
            ok = held[g, who, i]
            want[np.flatnonzero(ok), f["cards"][g, who, i][ok]] = 1
            lo = ((rel - 1) * hs + i) * bits
            assert np.array_equal(o[:, lo:lo + bits], want), "another seat's hand"
    for rel in range(P):
        assert np.array_equal(o[:, s["flags"] + rel], (f["hand_n"][g, (f["seat"] + rel) % P] < hs).astype(np.int64)), "missing-card flag"
    therm = lambda v, length: (np.arange(length)[None, :] < v[:, None]).astype(np.int64)
    assert np.array_equal(o[:, s["deck"]:s["fireworks"]], therm(f["deck"], deck_size - P * hs)), "deck thermometer"
    fw = np.zeros((n, Cc, R), np.int64)
    for c in range(Cc):
        ok = f["fireworks"][:, c] > 0
        fw[np.flatnonzero(ok), c, f["fireworks"][ok, c] - 1] = 1
    assert np.array_equal(o[:, s["fireworks"]:s["info"]], fw.reshape(n, bits)), "fireworks"
    assert np.array_equal(o[:, s["info"]:s["life"]], therm(f["info"], cfg.max_info)), "information tokens"
    assert np.array_equal(o[:, s["life"]:s["discards"]], therm(f["life"], cfg.max_life)), "life tokens"
    assert np.array_equal(o[:, s["discards"]:s["last"]], disc[:, :deck_size].astype(np.int64)), "discards"
    last = r[:, 2]
    assert np.array_equal(o[:, s["last"]:s["knowledge"]].any(1), (last & 1) == 1), "last action present"
    played = ((last >> 4) & 3) == 0                                   # "scored" and "information token" are shown for plays only
    assert np.array_equal(o[:, s["last_scored"]], (last >> 18) & 1 & played), "last action: scored"
    assert np.array_equal(o[:, s["last_scored"] + 1], (last >> 19) & 1 & played), "last action: information token"
    kn = o[:, s["knowledge"]:].reshape(n, P, hs, bits + Cc + R)
    for rel in range(P):
        who = (f["seat"] + rel) % P
        for i in range(hs):
            ok = held[g, who, i]
            k = kn[:, rel, i]
            assert not k[~ok].any(), "knowledge of an empty slot"
            assert (k[ok, bits:bits + Cc].sum(1) <= 1).all() and (k[ok, bits + Cc:].sum(1) <= 1).all()
            # the card itself is always among its plausible identities
            assert (k[np.flatnonzero(ok), f["cards"][g, who, i][ok]] == 1).all(), "a card is not plausible to its holder"
