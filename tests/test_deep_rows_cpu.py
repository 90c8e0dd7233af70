"""The deep-row corpus of tests/deep_rows.py, without a GPU: its floors (it cannot quietly stop reaching a state), the properties
of the determinizer's rule on `pick` of all twelve variants (asserted from the rows on the output of the restatement of
tests/test_search_cpu.py, by the checker tests/test_determinize_deep_gpu.py runs on the kernel's), and its teeth: five
deliberately wrong restatements, each told from the right one by `pick` in every variant where its mistake can show."""
import functools

import numpy as np
import pytest

import deep_rows as DR
from test_search_cpu import M32, deck_size_of, determinize_ref, determinize_row, philox_np

SEED, DRAW, REPLICAS = 7, 2, 6

# The corpus as first counted (deep_rows.counts): running with cards to draw, running on an empty deck, running with some seat
# short, finished, running without an information token.
RECORDED = {
    ("Hanabi-Full", 2): (2647, 58, 10, 1615, 163), ("Hanabi-Full", 3): (2121, 61, 24, 2138, 15),
    ("Hanabi-Full", 4): (2174, 90, 48, 2056, 36), ("Hanabi-Full", 5): (1861, 173, 111, 2286, 9),
    ("Hanabi-Small", 2): (1095, 43, 8, 1022, 250), ("Hanabi-Small", 3): (903, 77, 35, 1180, 130),
    ("Hanabi-Small", 4): (815, 141, 84, 1204, 106), ("Hanabi-Small", 5): (668, 204, 147, 1288, 77),
    ("Hanabi-Very-Small", 2): (439, 47, 17, 954, 73), ("Hanabi-Very-Small", 3): (283, 124, 68, 1033, 24),
    ("Hanabi-Very-Small", 4): (156, 183, 118, 1101, 11), ("Hanabi-Very-Small", 5): (0, 239, 151, 1201, 6),
}
NAMES = ("deck", "deck0", "short", "finished", "info0")


def _cfg(game, players):
    from oracle import oracle_py as O

    return O.make_config(game, players, 0)


def test_the_table_is_the_twelve_variants():
    assert set(RECORDED) == set(DR.VARIANTS) and len(DR.VARIANTS) == 12


@pytest.mark.parametrize("game,players", DR.VARIANTS)
def test_corpus_floors(game, players):
    """The floor of a category is what pick() takes of it (Very-Small 5 is dealt out completely: no row has cards to draw, then
    and now); RECORDED is what the corpus counted first, printed beside what it counts now."""
    c, p = DR.counts(game, players), DR.pick(game, players)
    recorded = dict(zip(NAMES, RECORDED[(game, players)]))
    print(game, players, "now", c, "recorded", recorded)
    need = dict(DR.TAKE)
    if recorded["deck"] == 0:
        need["deck"] = 0
        assert c["deck"] == 0
    for name in NAMES:
        assert c[name] >= need[name], (name, c[name])
        assert recorded[name] >= need[name]
    co = DR.corpus(game, players)
    assert co.rows.shape[0] == DR.N_GAMES * DR.STEPS[game] and co.rows.shape[1] == (48 if players >= 4 else 32)
    # the seat to act never holds a short hand: a short hand is reached through the determinizer's explicit seat only
    f = DR.fields(_cfg(game, players), co.rows)
    assert (f["own_n"][co.running] == _cfg(game, players).hand_size).all()
    # what pick() hands out
    taken = {name: int((p.category == name).sum()) for name, _ in DR.TAKE}
    short = c["short"] if c["short"] <= DR.SHORT_ALL else need["short"]
    assert taken["deck0"] == 12 and taken["short"] == short and taken["finished"] == 4 and taken["info0"] == 2 and taken["fresh"] == 1
    assert taken["deck"] in ((0,) if need["deck"] == 0 else (15, 16)) and len(p.rows) % 4 != 0
    assert len(set(p.index.tolist())) == len(p.index), "a row was picked twice"
    assert set(p.category[:6]) >= set(NAMES) - ({"deck"} if need["deck"] == 0 else set()), "a prefix of six rows mixes the categories"
    i = p.index
    assert co.deck0[i[p.category == "deck0"]].all() and co.finished[i[p.category == "finished"]].all()
    assert co.info0[i[p.category == "info0"]].all() and (co.running & ~co.deck0)[i[p.category == "deck"]].all()
    rows_short = np.flatnonzero(p.category == "short")
    assert co.short[p.short_seat[rows_short], i[rows_short]].all() and (p.short_seat[p.category != "short"] == -1).all()
    assert np.array_equal(p.rows[np.flatnonzero(p.category == "fresh")[0]], co.rows[0]) and (co.rows[0, 0] >> 21) & 255 == 0   # game 0, no move made


@pytest.mark.parametrize("game,players", DR.VARIANTS)
def test_restatement_properties_on_pick(game, players):
    """seat = -1 and every explicit seat, 6 replicas per row, checked by deep_rows.check_determinized; then seat = P (no such
    seat: unchanged copies of weight 0); then the change, over all the seats (deep_rows.assert_changes)."""
    cfg, p = _cfg(game, players), DR.pick(game, players)
    m, total = len(p.rows), np.zeros(6, np.int64)
    short_seen = 0
    for seat in range(-1, players + 1):
        out, w = determinize_ref(cfg, p.rows, seat, REPLICAS, SEED, DRAW, first_row_id=1000 * (seat + 1))
        got = DR.check_determinized(cfg, p.rows, seat, REPLICAS, out, w)
        if seat == players:
            assert got == (0,) * 6 and not w.any() and np.array_equal(out, np.repeat(p.rows, REPLICAS, 0))
        total += got
        short_seen += int((p.short_seat == seat).sum()) if seat >= 0 else 0
    live, changed, movable, moved, two, two_moved = (int(x) for x in total)
    print(f"{game} {players}: m = {m}, live outputs {live}, changed {changed}; of rows that can change {movable}, changed {moved}; "
          f"of those with a pool of two cards {two}, changed {two_moved}")
    assert short_seen == int((p.category == "short").sum())   # every short row met its short seat
    assert live >= REPLICAS * (players + 1) * 20
    DR.assert_changes(total)


# ---- teeth -----------------------------------------------------------------------------------------------------------------------
def _wrong_row(variant, cfg, row, seat, seed, draw, row_id):
    """tests/test_search_cpu.determinize_row with one deliberate mistake (variant None: none) -> (row_out, weight)."""
    row = np.asarray(row, np.uint32)
    P, H, D = cfg.players, cfg.hand_size, deck_size_of(cfg)
    w0, w1 = int(row[0]), int(row[1])
    st = (w0 >> 13) & 7 if seat < 0 or variant == "explicit_seat_ignored" else seat
    if (w0 >> 19) & 3 != 0 or st >= P:
        return row.copy(), 0
    w_deck = 10 + 3 * (2 if variant == "w_deck_of_two_players" else P)
    stride = 10 if variant == "knowledge_stride_10" else 12
    hand = int(row[10 + st])
    know = int(row[10 + P + 2 * st]) | int(row[10 + P + 2 * st + 1]) << 32
    n_hand = H if variant == "n_hand_is_hand_size" else min((w1 >> (15 + 3 * st)) & 7, H)
    deck_pos = 0 if variant == "deck_pos_is_zero" else D - min(w0 & 63, D)
    out = row.copy()
    deck_in, deck_out = row[w_deck:].view(np.uint8), out[w_deck:].view(np.uint8)
    pool = [(hand >> (5 * l)) & 31 for l in range(n_hand)] + [int(deck_in[q]) for q in range(deck_pos, D)]

    def plausible(s, card):
        kn = (know >> (stride * s)) & 0xFFF
        col, rk = divmod(card, cfg.ranks)
        return col < cfg.colors and bool((kn >> col) & 1) and bool((kn >> (5 + rk)) & 1)

    rid = int(row_id) & 0xFFFFFFFFFFFFFFFF
    rnd = philox_np(128 + np.arange(64), draw & M32, rid & M32, rid >> 32, seed & M32, ((seed >> 32) ^ (draw >> 32)) & M32)
    taken, weight, new_hand = set(), 1, hand
    for s in range(n_hand):
        cand = [l for l in range(len(pool)) if l not in taken and plausible(s, pool[l])]
        if not cand:
            return row.copy(), 0
        idx = cand[(int(rnd[0][s]) * len(cand)) >> 32]
        taken.add(idx)
        weight *= len(cand)
        new_hand = (new_hand & ~(31 << (5 * s))) | (pool[idx] << (5 * s))
    rest = [l for l in range(len(pool)) if l not in taken]
    rest.sort(key=lambda l: (int(rnd[1][l % 64]) & ~63) | l)
    for r, l in enumerate(rest):
        deck_out[deck_pos + r] = pool[l]
    out[10 + st] = new_hand
    return out, weight


# variant -> where its mistake can show: (game, players) -> bool
WRONG = {
    # an empty slot read as a card: through the explicit seat of a short hand, in every variant
    "n_hand_is_hand_size": lambda game, players: True,
    # the dealt cards taken for undealt ones: on every running row (no row has all of its deck undealt: the hands come off it)
    "deck_pos_is_zero": lambda game, players: True,
    # an explicit seat that is not the seat to act: in every variant
    "explicit_seat_ignored": lambda game, players: True,
    # slot 1 and later read another slot's bits: wherever a hand of two or more has been told something
    "knowledge_stride_10": lambda game, players: True,
    # the deck looked for at word 16: with three players or more, on rows with cards to draw (Very-Small 5 has none; a row
    # without them has no deck byte to read or write)
    "w_deck_of_two_players": lambda game, players: players > 2 and (game, players) != ("Hanabi-Very-Small", 5),
}


def _outputs(variant, game, players):
    """Every output (row, weight) of a variant of the rule over pick: seat = -1 and every explicit seat, 2 replicas."""
    cfg, p = _cfg(game, players), DR.pick(game, players)
    res = []
    for seat in range(-1, players):
        for o in range(2 * len(p.rows)):
            res.append((seat, o // 2) + _wrong_row(variant, cfg, p.rows[o // 2], seat, SEED, DRAW, o))
    return res


@functools.lru_cache(maxsize=None)
def _right(game, players):
    """The restatement's own outputs in _outputs' order (shared by the tests below; read only)."""
    cfg, p = _cfg(game, players), DR.pick(game, players)
    return [(seat, o // 2) + determinize_row(cfg, p.rows[o // 2], seat, SEED, DRAW, o)[:2]
            for seat in range(-1, players) for o in range(2 * len(p.rows))]


def _told_apart(variant, game, players):
    """(seat, row of pick) of the outputs at which the variant differs from the restatement, in the row or in the weight (a short
    hand of Small or Very-Small is one card behind an empty deck: its only arrangement is the source, so a wrong walk of it shows
    in the weight alone), and how many of them differ in the row."""
    hits, in_row = [], 0
    for (seat, i, row, w), (_, _, want, want_w) in zip(_outputs(variant, game, players), _right(game, players)):
        if w != want_w or not np.array_equal(row, want):
            hits.append((seat, i))
            in_row += not np.array_equal(row, want)
    return hits, in_row


@pytest.mark.parametrize("game,players", DR.VARIANTS)
def test_the_walk_without_a_mistake_is_the_restatement(game, players):
    assert _told_apart(None, game, players) == ([], 0)


@pytest.mark.parametrize("game,players", DR.VARIANTS)
@pytest.mark.parametrize("variant", sorted(WRONG))
def test_pick_catches_a_wrong_walk(variant, game, players):
    hits, in_row = _told_apart(variant, game, players)
    print(f"{variant} on {game} {players}: {len(hits)} outputs differ ({in_row} in the row), first {hits[:3]}")
    if WRONG[variant](game, players):
        assert hits, f"no row of pick notices {variant} on {game} {players}: pick is too weak"
    else:
        assert not hits, "the mistake shows where it was said it cannot"
