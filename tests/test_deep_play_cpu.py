"""The deep-play corpus on the CPU oracle alone (tests/deep_play.py).

* The corpus is a real test: each of the twelve variants, driven by `open_hand_moves`, reaches empty decks, short hands, the
  final round with points on the board, the max-score ending and a stack short of it at least as often as the floors below.
  The floors are at most half of what the smallest variant gave when the driver was first measured; under uniform-random play
  the same tally is zero, which is why the driver exists.
* Each rule alone, at every state of the corpus: the move of every single-rule list is legal, every kind fires and declines.
* Card conservation and the structure of the observation on those states, against the state row.
* Hand-worked known answers on explicit decks, derived from SURVEY App. A: the max-score ending, the deck running out with
  points on the board, a 5 played with all tokens there.
"""
import functools

import numpy as np
import pytest

import deep_play as D
from oracle import oracle_py as O
from test_oracle_env import _unpack, canonical_deck
from test_rule_agents import deck_with_prefix

FULL = [v for v in D.VARIANTS if v[0] == "Hanabi-Full"]
SMALL = [v for v in D.VARIANTS if v[0] != "Hanabi-Full"]


@functools.lru_cache(maxsize=None)
def corpus(game, players, driver="open"):
    """One run of a variant on the oracle: the tally, how often each entry of RULES fired / declined / was illegal, and the
    first broken invariant (None when all hold)."""
    cfg = O.make_config(game, players, D.FLAGS)
    orc = O.OracleEnv(cfg, D.N_GAMES, seed=D.SEED, first_game_id=D.FIRST_GAME_ID)
    rng = np.random.default_rng(D.SEED)
    tally = D.Tally(cfg)
    fired, declined, illegal = (np.zeros(len(D.RULES), np.int64) for _ in range(3))
    out, rows = orc.observe(), orc.export_state()
    tally.state(rows)
    broken = None
    after_empty = np.zeros(D.N_GAMES, np.int64)      # moves made on an empty deck, per game in progress
    g = np.arange(D.N_GAMES)
    for t in range(D.steps_of(game, players)):
        try:
            D.check_states(cfg, orc.deck_size, rows, out["obs"])
            if t % 8 == 0:                           # the vectorised decoding against test_oracle_env's, game by game
                f = D.fields(cfg, rows)
                for k in range(D.N_GAMES):
                    s = _unpack(cfg, rows[k])
                    assert (s["deck_size"], s["info"], s["life"], s["cur"]) == (f["deck"][k], f["info"][k], f["life"][k], f["seat"][k])
                    assert s["fireworks"] == list(f["fireworks"][k]) and s["hand_n"] == list(f["hand_n"][k])
                    assert all(s["hands"][p] == list(f["cards"][k, p, :s["hand_n"][p]]) for p in range(players))
        except AssertionError as e:
            broken = broken or f"step {t}: {e}"
        if driver == "open":
            for i, rule in enumerate(D.RULES):
                act, which = orc.rule_act([rule], D.RULE_SEED, t)
                ok = (act >= 0) & (act < orc.num_actions)
                illegal[i] += int((~ok).sum()) + int((out["legal"][g[ok], act[ok]] == 0).sum())
                fired[i] += int((which == 0).sum())
                declined[i] += int((which == 1).sum())
            act = D.open_hand_moves(cfg, rows, out["legal"], rng, D.P_RAND)
        else:
            act = O.random_legal_actions(out["legal"], 4321, t, first_game_id=D.FIRST_GAME_ID)
        before = D.fields(cfg, rows)
        out = orc.step(act)
        after = orc.export_state()
        tally.step(rows, act, out, after)
        # A.5: after the draw that empties the deck every player moves exactly once more
        after_empty += before["deck"] == 0
        term = out["terminal"] != 0
        slot = np.clip(act - cfg.hand_size, 0, cfg.hand_size - 1)
        card = before["own"][g, slot]
        misplay = (act >= cfg.hand_size) & (act < 2 * cfg.hand_size) & \
            (card % cfg.ranks != before["fireworks"][g, np.minimum(card // cfg.ranks, cfg.colors - 1)])
        out_of_cards = term & (out["score"] < cfg.colors * cfg.ranks) & ~(misplay & (before["life"] == 1))
        if not ((after_empty[out_of_cards] == players).all() and (after_empty[~term] < players).all()):
            broken = broken or f"step {t}: not exactly {players} moves on the empty deck"
        after_empty[term] = 0
        rows = after
    assert orc.illegal_count() == 0
    # every ending is one of the three: a score between 0 and the maximum is only kept by running out of cards
    assert tally.episodes == tally.end_max + tally.end_zero + tally.end_deck_empty_scored
    return dict(tally=tally, fired=fired, declined=declined, illegal=illegal, broken=broken)


@pytest.mark.parametrize("game,players", D.VARIANTS)
def test_corpus_reaches_the_deep_states(game, players):
    t = corpus(game, players)["tally"]
    print(game, players, t.as_dict())
    cfg = t.cfg
    assert t.end_max >= 8
    assert t.end_deck_empty_scored >= 50
    assert t.deck0_states >= 150
    assert t.info0_states >= 25
    assert t.short_hand_states >= 30
    assert t.max_fireworks >= cfg.colors * cfg.ranks - 1
    assert t.end_zero >= 1
    assert t.completed_with_token + t.completed_without_token >= cfg.colors * t.end_max


def test_random_legal_play_reaches_none_of_it():
    """Why the driver exists: the play every other differential test uses never empties the deck and never wins."""
    t = corpus("Hanabi-Full", 2, driver="random")["tally"]
    print(t.as_dict())
    assert t.deck0_states == 0 and t.end_max == 0
    assert t.completed_with_token + t.completed_without_token == 0 and t.end_deck_empty_scored == 0
    assert t.episodes > D.N_GAMES


@pytest.mark.parametrize("game,players", D.VARIANTS)
def test_every_rule_alone_is_legal(game, players):
    c = corpus(game, players)
    assert not c["illegal"].any(), [D.RULES[i] for i in np.flatnonzero(c["illegal"])]
    assert ((c["fired"] + c["declined"]) == D.N_GAMES * D.steps_of(game, players)).all()


def _by_kind(counts):
    out = np.zeros(16, np.int64)
    for (kind, _, _), v in zip(D.RULES, counts):
        out[kind] += v
    return out


@pytest.mark.parametrize("game,players", FULL)
def test_every_rule_fires_and_declines_on_full(game, players):
    c = corpus(game, players)
    fired, declined = _by_kind(c["fired"]), _by_kind(c["declined"])
    print(game, players, "fired", dict(zip(D.RULES, c["fired"])), "declined", dict(zip(D.RULES, c["declined"])))
    assert (fired[1:15] >= 20).all() and (declined[1:15] >= 20).all(), (fired, declined)
    for rule, f, d in zip(D.RULES, c["fired"], c["declined"]):   # and so does every argument / threshold of a kind
        assert 1 <= rule[0] <= 14 and f >= 20 and d >= 20 or rule[0] in (0, 15), (rule, f, d)
    assert declined[0] == 0 and fired[15] == 0          # legal_random always fires, tell_most_information never


@pytest.mark.parametrize("game,players", SMALL)
def test_rules_that_need_a_spare_life_stay_silent_in_small_games(game, players):
    c = corpus(game, players)
    print(game, players, "fired", dict(zip(D.RULES, c["fired"])))
    for rule, n in zip(D.RULES, c["fired"]):
        if rule[0] == D.HAIL_MARY or rule == D.NEED_LIVES:
            assert n == 0, rule                          # max_life = 1: never more than one life
        elif rule[0] == 15:
            assert n == 0
        else:
            assert n > 0, rule
    assert c["declined"][0] == 0


@pytest.mark.parametrize("game,players", D.VARIANTS)
def test_invariants_on_deep_states(game, players):
    assert corpus(game, players)["broken"] is None


# ---- hand-worked known answers (explicit decks, no auto-reset) ---------------------------------------------

def _ones(o, lo, hi):
    return [int(i) for i in np.flatnonzero(o[lo:hi]) + lo]


def test_kat_five_plays_reach_the_maximum_score():
    """Very-Small, 2 players (1 colour, hands of 2, 3 tokens, 1 life): deck 1 3 2 4 5 | 1 1 2 3 4 (ranks). P0 = 1 3, P1 = 2 4;
    each plays its slot 0 in turn, P0 draws the 5 after its first play and holds it in slot 0 at its third.
    Observation, A.6 with bits = 5, hs = 2, P = 2, D = 10: hands 10 | flags 2 | deck 6 -> fireworks [18, 23) | info [23, 26) |
    life [26] | discards [27, 37) | last action: actor [37, 39) type [39, 43) target [43, 45) colour [45] rank [46, 51)
    outcome [51, 53) position [53, 55) card [55, 60) scored 60, info token 61 | knowledge [62, 106)."""
    cfg = O.make_config("Hanabi-Very-Small", 2)
    env = O.OracleEnv(cfg, 1, decks=np.array([[0, 2, 1, 3, 4, 0, 0, 1, 2, 3]], np.uint8))
    assert env.obs_len == 106 and env.num_actions == 10
    for k in range(4):
        out = env.step([2])                               # play slot 0: uid = hand_size + 0
        assert (out["reward"][0], out["terminal"][0], out["score"][0]) == (1, 0, k + 1)
        assert _ones(out["obs"][0], 18, 23) == [18 + k]
    out = env.step([2])                                   # P0 plays the 5
    o = out["obs"][0]
    assert (out["reward"][0], out["terminal"][0], out["score"][0]) == (1, 1, 5)
    st = env.export_state()[0]
    assert (st[0] >> 19) & 3 == 2                         # status: fireworks complete
    assert (st[1] & 7) == 5 and (st[0] >> 10) & 7 == 1    # the stack at 5, the life still there
    assert (st[0] >> 6) & 15 == 3                         # all three tokens were there: none comes back
    assert (st[2] >> 18) & 3 == 1                         # last move: scored, no token
    # the next seat is P1, which has moved before: LAST, with its own +1 and P0's +1 since its move
    assert out["agent_step_type"][0] == 2 and out["agent_reward"][0] == 2
    assert _ones(o, 18, 23) == [18 + 4]                   # fireworks at rank 5
    assert _ones(o, 23, 27) == [23, 24, 25, 26]           # 3 tokens, 1 life
    assert _ones(o, 27, 37) == []                         # nothing was discarded
    # actor P0 at offset (0 - 1) mod 2 = 1, play, position 0, card rank 5, scored without a token
    assert _ones(o, 37, 62) == [37 + 1, 39 + 0, 53 + 0, 55 + 4, 60]


def test_kat_deck_runs_out_with_points_on_the_board():
    """Full, 2 players, canonical deck: P0 = R1 R1 R1 R2 R2, P1 = R3 R3 R4 R4 R5. P0 plays R1 and R2 (2 points, 38 cards
    left), then P1 hints the rank of P0's oldest card and P0 discards its oldest card, 38 times over: P0's 38th discard draws
    the last card. Exactly two more moves: P1 plays its R3 (3 points) and cannot draw, P0 discards and cannot draw.
    Offsets: SURVEY A.6's table for 2 players (flags 125 observer / 126 partner, deck [127, 167), fireworks [167, 192),
    last action [253, 308), knowledge 308 + 35 * slot, the partner's slots 5-9)."""
    cfg = O.make_config("Hanabi-Full", 2)
    env = O.OracleEnv(cfg, 1, decks=canonical_deck(cfg)[None])
    out = env.step([5])                                   # P0 plays slot 0 (R1), draws
    out = env.step([15])                                  # P1 reveals rank 1 (uid 2*5 + 5 + 0): P0 still holds R1s; 7 tokens
    out = env.step([5 + 2])                               # P0 = R1 R1 R2 R2 Y1: slot 2 is an R2
    assert out["score"][0] == 2 and out["obs"][0][127:167].sum() == 38
    for k in range(38):
        oldest = int(env.export_state()[0][10]) & 31
        out = env.step([15 + oldest % 5])                 # P1: the rank of P0's oldest card (always a legal hint)
        assert out["legal"][0, 0] == 1 and out["terminal"][0] == 0
        out = env.step([0])                               # P0 discards slot 0 and draws
        o = out["obs"][0]
        assert o[127:167].sum() == 37 - k and out["terminal"][0] == 0 and out["score"][0] == 2
        assert not o[125:127].any()                       # every hand is full, also right after the last card was drawn
    assert env.export_state()[0][0] & 63 == 0
    # first of the two last moves: P1 plays slot 0 (R3 on a red stack at 2) and has no card to draw
    out = env.step([5])
    o = out["obs"][0]                                     # observer: P0
    assert (out["reward"][0], out["terminal"][0], out["score"][0]) == (1, 0, 3)
    assert _ones(o, 125, 127) == [126]                    # the partner is one card short, the observer is not
    assert [int(np.argmax(o[25 * i:25 * i + 25])) if o[25 * i:25 * i + 25].any() else None for i in range(5)] == [2, 3, 3, 4, None]
    assert not o[308 + 9 * 35:658].any() and o[308 + 8 * 35:308 + 9 * 35].any()   # its fifth knowledge slot is empty
    assert not o[127:167].any() and _ones(o, 167, 192) == [167 + 2]
    assert _ones(o, 253, 308) == [253 + 1, 255 + 0, 276 + 0, 281 + 2, 306]        # P1's play of R3 scored, no token (a 3)
    assert out["legal"][0].any()
    # the second: P0 discards; the game is over with its three points kept
    out = env.step([0])
    o = out["obs"][0]                                     # observer: P1
    assert (out["reward"][0], out["terminal"][0], out["score"][0]) == (0, 1, 3)
    assert out["agent_step_type"][0] == 2 and out["agent_reward"][0] == 1          # P1: its own R3 since its move
    st = env.export_state()[0]
    assert (st[0] >> 19) & 3 == 3 and (st[0] >> 10) & 7 == 3
    assert [(st[1] >> (15 + 3 * p)) & 7 for p in range(2)] == [4, 4]
    assert _ones(o, 125, 127) == [125, 126]               # both hands are short now
    assert not o[100:125].any() and not o[308 + 4 * 35:308 + 5 * 35].any() and not o[308 + 9 * 35:658].any()
    assert _ones(o, 167, 192) == [167 + 2] and _ones(o, 253, 259) == [253 + 1, 255 + 1]   # P0 at offset 1 discarded


R1, R2, R3, R4, R5, Y1, Y2, Y3 = 0, 1, 2, 3, 4, 5, 6, 7


def test_kat_a_five_played_with_all_tokens_returns_none():
    """Full, 2 players. P0 = R1 R3 R5 Y1 Y1, P1 = R2 R4 Y2 Y2 Y3: five plays of slot 0 complete the red stack with the 8
    tokens untouched, so no token comes back and the last action is "scored" without "information token" (A.5 step 3).
    The same stack with one token spent first (hands swapped, P0 opens with a colour hint): the token comes back, both bits."""
    cfg = O.make_config("Hanabi-Full", 2)
    env = O.OracleEnv(cfg, 1, decks=np.array([deck_with_prefix([R1, R3, R5, Y1, Y1, R2, R4, Y2, Y2, Y3])], np.uint8))
    for k in range(5):
        out = env.step([5])
        assert (out["reward"][0], out["score"][0], out["terminal"][0]) == (1, k + 1, 0)
    o, st = out["obs"][0], env.export_state()[0]
    assert (st[0] >> 6) & 15 == 8 and o[192:200].sum() == 8
    assert (st[2] >> 18) & 3 == 1
    assert _ones(o, 167, 192) == [167 + 4]
    assert _ones(o, 253, 308) == [253 + 1, 255 + 0, 276 + 0, 281 + 4, 306]     # actor P0 at offset 1, play, slot 0, R5, scored
    assert out["legal"][0, 0:5].sum() == 0                                      # 8 tokens: still no discards

    env = O.OracleEnv(cfg, 1, decks=np.array([deck_with_prefix([R2, R4, Y2, Y2, Y3, R1, R3, R5, Y1, Y1])], np.uint8))
    out = env.step([10])                                                        # P0 reveals colour R (uid 2*5 + 0): 7 tokens
    assert out["obs"][0][192:200].sum() == 7
    for k in range(5):
        out = env.step([5])
        assert (out["reward"][0], out["score"][0]) == (1, k + 1)
        assert out["obs"][0][192:200].sum() == (8 if k == 4 else 7)
    o, st = out["obs"][0], env.export_state()[0]
    assert (st[0] >> 6) & 15 == 8 and (st[2] >> 18) & 3 == 3
    assert _ones(o, 253, 308) == [253 + 1, 255 + 0, 276 + 0, 281 + 4, 306, 307]
