"""Deep state rows of all twelve variants for the kernels that take an `hb_config` and state rows (helper module; DESIGN.md
section 6): the determinizer, the search layout and the rule playout.

`corpus(game, players)` is every state the open-handed driver of tests/deep_play.py visits on the CPU oracle, with masks that
name what a row is; `pick(game, players)` is a fixed few dozen of them, every category in every prefix;
`check_determinized` states what hb_belief_determinize promises about its output in numpy over the row layout (DESIGN.md section
3), without the restatement of tests/test_search_cpu.py: tests/test_deep_rows_cpu.py runs it on the restatement's output,
tests/test_determinize_deep_gpu.py on the kernel's. Nothing here touches the GPU or the library's kernels."""
import collections
import functools

import numpy as np

from deep_play import VARIANTS, fields, open_hand_moves   # noqa: F401  (VARIANTS: re-exported for the tests)
from oracle import oracle_py as O

N_GAMES, ENV_SEED, RNG_SEED, P_RAND = 48, 9, 4, 0.05
STEPS = {"Hanabi-Full": 90, "Hanabi-Small": 45, "Hanabi-Very-Small": 30}
# what pick() takes of each category, in the order it deals them out
TAKE = (("deck", 16), ("deck0", 12), ("short", 8), ("finished", 4), ("info0", 2), ("fresh", 1))
SHORT_ALL = 10   # a corpus with no more short-seat rows than this gives all of them (Full 2: 10, Small 2: 8)

Corpus = collections.namedtuple("Corpus", "rows running deck0 short finished info0")
Pick = collections.namedtuple("Pick", "rows short_seat category index")


def deck_size_of(cfg):
    return cfg.colors * sum(3 if r == 0 else 1 if r == cfg.ranks - 1 else 2 for r in range(cfg.ranks))


@functools.lru_cache(maxsize=None)
def corpus(game, players):
    """Every turn's export of 48 oracle games (seed 9, flags 0: a finished game stays finished) driven for 90 / 45 / 30 steps
    (Full / Small / Very-Small) by `open_hand_moves` with default_rng(4) and 5 % random moves, concatenated in turn order:
    rows [N, SW] uint32 and boolean masks over them: running; deck0 (running, nothing left to draw); short [P, N] (running, seat
    p holds fewer than hand_size cards); finished; info0 (running, no information token). Rows 0..47 are the fresh deals.
    Read only: shared."""
    cfg = O.make_config(game, players, 0)
    env = O.OracleEnv(cfg, N_GAMES, seed=ENV_SEED)
    legal, rng, turns = env.observe()["legal"], np.random.default_rng(RNG_SEED), []
    for _ in range(STEPS[game]):
        rows = np.asarray(env.export_state()).astype(np.uint32)
        turns.append(rows.copy())
        legal = env.step(open_hand_moves(cfg, rows, legal, rng, P_RAND))["legal"]
    assert env.illegal_count() == 0
    rows = np.concatenate(turns)
    f = fields(cfg, rows)
    running = ((rows[:, 0] >> 19) & 3) == 0
    c = Corpus(rows, running, running & (f["deck"] == 0), (running[:, None] & (f["hand_n"] < cfg.hand_size)).T.copy(), ~running,
               running & (f["info"] == 0))
    for a in c:
        a.setflags(write=False)
    return c


def counts(game, players):
    """The corpus' category counts, the columns of the table in tests/test_deep_rows_cpu.py."""
    c = corpus(game, players)
    return dict(deck=int((c.running & ~c.deck0).sum()), deck0=int(c.deck0.sum()), short=int(c.short.any(0).sum()),
                finished=int(c.finished.sum()), info0=int(c.info0.sum()))


def _spread(idx, k):
    """k of the indices `idx`, evenly spaced from the first to the last (all of them when there are no more than k)."""
    idx = np.asarray(idx)
    if len(idx) <= k:
        return list(idx)
    return list(idx[np.round(np.linspace(0, len(idx) - 1, k)).astype(np.int64)])


@functools.lru_cache(maxsize=None)
def pick(game, players):
    """A fixed selection of the corpus: 16 running rows with cards to draw (Very-Small 5 has none), 12 running rows with an empty
    deck and full hands where there are that many (else the empty-deck rows there are), 8 running rows in which some seat is
    short (all of them where the corpus has no more than 10), 4 finished rows, 2 running rows without an information token, and
    the fresh deal of game 0; each category spread evenly over its rows in turn order, the categories dealt out in turn so that
    every prefix mixes them. A total that is a multiple of 4 (a workgroup of the determinizer holds four output rows) loses its
    last row with cards to draw. Returns rows [m, SW] uint32, short_seat [m] (the lowest short seat of a short row, -1
    elsewhere), category [m] (names of TAKE) and index [m] (row of the corpus). Read only: shared."""
    c = corpus(game, players)
    any_short = c.short.any(0)
    short = np.flatnonzero(any_short)
    full0 = np.flatnonzero(c.deck0 & ~any_short)
    n0 = dict(TAKE)["deck0"]
    chosen, used = dict(fresh=[0]), {0}

    def take(name, idx, k):   # (no row twice: a category chooses among the rows the ones before it left)
        chosen[name] = _spread([i for i in idx if i not in used], k)
        used.update(chosen[name])

    take("short", short, len(short) if len(short) <= SHORT_ALL else dict(TAKE)["short"])
    take("info0", np.flatnonzero(c.info0), dict(TAKE)["info0"])
    take("finished", np.flatnonzero(c.finished), dict(TAKE)["finished"])
    take("deck0", full0 if len([i for i in full0 if i not in used]) >= n0 else np.flatnonzero(c.deck0), n0)
    take("deck", np.flatnonzero(c.running & ~c.deck0), dict(TAKE)["deck"])
    if sum(len(v) for v in chosen.values()) % 4 == 0:
        chosen["deck"] = chosen["deck"][:-1]
    order = []
    for k in range(max(len(v) for v in chosen.values())):
        order += [(name, chosen[name][k]) for name, _ in TAKE if k < len(chosen[name])]
    index = np.array([i for _, i in order], np.int64)
    seat = np.array([int(np.argmax(c.short[:, i])) if name == "short" else -1 for name, i in order], np.int64)
    p = Pick(np.ascontiguousarray(c.rows[index]), seat, np.array([name for name, _ in order]), index)
    assert len(index) % 4 != 0
    for a in p:
        a.setflags(write=False)
    return p


# ---- what the determinizer promises, from the rows alone -------------------------------------------------------------------------
def _view(cfg, rows, seat):
    """Per row, for the observing seat (`seat`, or the seat to act where it is -1): live (running and a seat of the game), the
    seat (0 where not live), its hand [n, H], hand size, knowledge [n, H] (12 bits a slot), the deck bytes [n, D] and the
    first undealt position."""
    r = np.ascontiguousarray(np.asarray(rows)).view(np.uint32).astype(np.int64)
    n, P, H, D = r.shape[0], cfg.players, cfg.hand_size, deck_size_of(cfg)
    g = np.arange(n)
    st = (r[:, 0] >> 13) & 7 if seat < 0 else np.full(n, seat, np.int64)
    live = (((r[:, 0] >> 19) & 3) == 0) & (st < P)
    st = np.where(live, st, 0)
    hand_w = r[g, 10 + st]
    hand = np.stack([(hand_w >> (5 * s)) & 31 for s in range(H)], axis=1)
    n_hand = np.minimum((r[:, 1] >> (15 + 3 * st)) & 7, H)
    kn64 = r[g, 10 + P + 2 * st] | (r[g, 10 + P + 2 * st + 1] << 32)
    know = np.stack([(kn64 >> (12 * s)) & 0xFFF for s in range(H)], axis=1)
    deck = np.ascontiguousarray(np.asarray(rows)[:, 10 + 3 * P:]).view(np.uint8).reshape(n, -1).astype(np.int64)
    return live, st, hand, n_hand, know, deck, D - np.minimum(r[:, 0] & 63, D)


def _plausible(cfg, know, card):
    """know, card: arrays of one shape -> the card is one of the game's and its colour and its rank are both plausible."""
    col, rk = card // cfg.ranks, card % cfg.ranks
    return (col < cfg.colors) & (((know >> np.minimum(col, 4)) & 1) == 1) & (((know >> (5 + rk)) & 1) == 1)


def _pool_counts(hand, n_hand, deck, deck_pos, D):
    """[n, 256]: how often each byte value is among the first n_hand slots and the deck positions deck_pos .. D - 1."""
    n = hand.shape[0]
    cnt = np.zeros((n, 256), np.int64)
    for s in range(hand.shape[1]):
        ok = s < n_hand
        np.add.at(cnt, (np.flatnonzero(ok), hand[ok, s]), 1)
    for q in range(D):
        ok = q >= deck_pos
        np.add.at(cnt, (np.flatnonzero(ok), deck[ok, q]), 1)
    return cnt


def can_change(cfg, rows, seat):
    """[n] bool: live rows with at least two arrangements the rule allows, by a sufficient condition that needs no walk: two
    different cards among the undealt ones (the hand as it is, the deck in two orders), or a slot whose card can change places
    with a different undealt card that is plausible for it, or with the card of another slot where each is plausible for the
    other's slot. Such a row has a pool of two or more."""
    live, _, hand, n_hand, know, deck, deck_pos = _view(cfg, rows, seat)
    n, H, D = hand.shape[0], cfg.hand_size, deck_size_of(cfg)
    q = np.arange(D)[None, :]
    undealt = q >= deck_pos[:, None]
    lo = np.where(undealt, deck[:, :D], 256).min(1)
    hi = np.where(undealt, deck[:, :D], -1).max(1)
    ok = undealt.any(1) & (lo != hi)
    for s in range(H):
        held = s < n_hand
        swap = undealt & (deck[:, :D] != hand[:, s:s + 1]) & _plausible(cfg, know[:, s:s + 1], deck[:, :D])
        ok |= held & swap.any(1)
        for t in range(s + 1, H):
            ok |= (t < n_hand) & (hand[:, s] != hand[:, t]) & _plausible(cfg, know[:, s], hand[:, t]) & _plausible(cfg, know[:, t], hand[:, s])
    return live & ok


def check_determinized(cfg, src, seat, replicas, out, weights):
    """The properties of hb_belief_determinize's output (include/hanabi_hip.h) on rows reached by play, asserted from the rows
    themselves: src [m, SW], out [m * replicas, SW], weights [m * replicas] (any integer type; the u32 values).
      - a row that is not live (finished, or the observing seat is no seat of the game) comes back unchanged with weight 0;
      - a live row's replicas all carry the same weight, and it is not 0 (states reached by play: the plausible sets of a hand
        are nested or disjoint, tests/test_search_cpu.crossed_states);
      - only the observing seat's hand word and the deck words differ from the source; deck bytes below the first undealt
        position, and the bytes behind the deck, are the source's; hand fields at or above the hand size are the source's, 31;
      - the cards of the hand and the undealt deck are the source's, card by card (the pool multiset);
      - every filled slot holds a card plausible under that slot's knowledge.
    Returns six counts of outputs: live; live and different from the source; of can_change rows; of those, different; of
    can_change rows whose pool is two cards; of those, different (see `assert_changes`)."""
    src = np.ascontiguousarray(np.asarray(src)).view(np.uint32)
    out = np.ascontiguousarray(np.asarray(out)).view(np.uint32)
    w = np.asarray(weights).astype(np.int64) & 0xFFFFFFFF
    m, R, P, H, D = src.shape[0], int(replicas), cfg.players, cfg.hand_size, deck_size_of(cfg)
    assert out.shape == (m * R, src.shape[1]) and w.shape == (m * R,)
    rep = np.repeat(src, R, axis=0)
    live, st, hand, n_hand, know, deck, deck_pos = _view(cfg, rep, seat)
    assert (w[~live] == 0).all(), "a row that is not live weighs something"
    assert np.array_equal(out[~live], rep[~live]), "a row that is not live was changed"
    assert (w[live] > 0).all(), "a dead replica of a state reached by play"
    wr = w.reshape(m, R)
    assert (wr == wr[:, :1]).all(), "the weights of a root's replicas differ"
    live2, st2, hand2, n_hand2, know2, deck2, deck_pos2 = _view(cfg, out, seat)
    assert np.array_equal(live2, live) and np.array_equal(st2, st) and np.array_equal(n_hand2, n_hand)
    assert np.array_equal(know2, know) and np.array_equal(deck_pos2, deck_pos)
    g = np.flatnonzero(live)
    same = np.ones(out.shape, bool)
    same[g, 10 + st[g]] = False
    same[:, 10 + 3 * P:] = False
    assert np.array_equal(out[same], rep[same]), "a word other than the seat's hand and the deck changed"
    q = np.arange(deck.shape[1])[None, :]
    fixed = (q < deck_pos[:, None]) | (q >= D)
    assert np.array_equal(deck2[fixed], deck[fixed]), "a dealt deck byte, or a byte behind the deck, changed"
    empty = np.arange(H)[None, :] >= n_hand[:, None]
    assert (hand[live][empty[live]] == 31).all() and (hand2[live][empty[live]] == 31).all(), "an empty slot does not hold 31"
    hw = out[g, 10 + st[g]].astype(np.int64)
    assert np.array_equal(hw >> (5 * H), rep[g, 10 + st[g]].astype(np.int64) >> (5 * H)), "bits above the hand's fields changed"
    assert np.array_equal(_pool_counts(hand2[live], n_hand[live], deck2[live], deck_pos[live], D),
                          _pool_counts(hand[live], n_hand[live], deck[live], deck_pos[live], D)), "the pool's cards are not conserved"
    assert (_plausible(cfg, know, hand2) | empty)[live].all(), "a slot holds a card its knowledge rules out"
    differs = (out != rep).any(1)
    movable = can_change(cfg, rep, seat)
    assert not (differs & ~live).any()
    two = movable & (n_hand + D - deck_pos == 2)
    return tuple(int(x.sum()) for x in (live, differs & live, movable, differs & movable, two, differs & two))


def assert_changes(counts):
    """The determinizer does change rows: `counts` is check_determinized's result, or the sum of several.
    Of the live outputs of rows that can change, more than half differ from their source, wherever some such row has a pool of
    three cards or more. A row whose pool is two cards (a hand of two behind an empty deck: every row of Very-Small 5) has
    exactly two arrangements, and the rule's uniform draw for slot 0 takes each with probability 1/2 whatever the seed: there
    "more than half" is a coin's toss, and what holds is that the changed outputs of those rows lie within six binomial
    standard deviations, 3 sqrt(n), of n / 2 (draws of different row ids are independent) -- which also fails a sampler that
    never, or always, swaps."""
    live, changed, movable, moved, two, two_moved = (int(x) for x in counts)
    assert movable > 0 and changed >= moved
    if movable > two:
        assert 2 * moved > movable, (moved, movable)
    assert (2 * two_moved - two) ** 2 <= 36 * two, (two_moved, two)
