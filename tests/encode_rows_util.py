"""Helpers shared by tests/test_encode_rows_cpu.py and tests/test_encode_rows_gpu.py: the deep-play run of tests/deep_play.py
as a generator of (state rows, oracle outputs), and rows picked out of it at the depths an encoder goes wrong at."""
import functools

import numpy as np

import deep_play as D
from oracle import oracle_py as O

MAX_STEPS = 200
SNAPSHOTS = ("start", "mid", "empty_deck", "redealt", "round")


def steps(game, players):
    return min(D.steps_of(game, players), MAX_STEPS)


def deep_run(game, players, tally=None):
    """The deep-play corpus (deep_play's constants: 130 games, FLAGS, P_RAND, SEED) on the oracle, one item per state visited:
    (t, rows uint32 [130, SW], oracle outputs for those rows). Item 0 is the fresh deal; item t the state after t moves."""
    cfg = O.make_config(game, players, D.FLAGS)
    orc = O.OracleEnv(cfg, D.N_GAMES, seed=D.SEED, first_game_id=D.FIRST_GAME_ID)
    rng = np.random.default_rng(D.SEED)
    out, rows = orc.observe(), orc.export_state()
    if tally is not None:
        tally.state(rows)
    yield 0, rows, out
    for t in range(steps(game, players)):
        act = D.open_hand_moves(cfg, rows, out["legal"], rng, D.P_RAND)
        out = orc.step(act)
        after = orc.export_state()
        if tally is not None:
            tally.step(rows, act, out, after)
        rows = after
        yield t + 1, rows, out
    assert orc.illegal_count() == 0


@functools.lru_cache(maxsize=None)
def deep_rows(game, players):
    """Five snapshots [130, SW] uint32 of one deep run: the fresh deal, mid-game, the state with the most empty decks, the state
    with the most games past their first re-deal (deal counter, word 6, above 1), and "round": 26 games of each of five
    consecutive mid-game states (the games move in lock step, so only this one has every seat to act). Read only: shared."""
    snaps = list(deep_run(game, players))
    rows = [r for _, r, _ in snaps]
    empty = max(range(len(rows)), key=lambda i: int(((rows[i][:, 0] & 63) == 0).sum()))
    redealt = max(range(len(rows)), key=lambda i: (int((rows[i][:, 6] > 1).sum()), i))
    mid = len(rows) // 3
    picked = {"start": rows[0], "mid": rows[mid], "empty_deck": rows[empty], "redealt": rows[redealt],
              "round": np.concatenate([rows[mid + 1 + k][26 * k:26 * (k + 1)] for k in range(5)])}
    assert ((picked["empty_deck"][:, 0] & 63) == 0).any() and (picked["redealt"][:, 6] > 1).any()
    for r in picked.values():
        r.setflags(write=False)
    return picked


def mixed_rows(game, players, n):
    """n rows cycling through the five snapshots (every depth in every batch size), uint32 [n, SW], read only."""
    snaps = deep_rows(game, players)
    pool = np.concatenate([snaps[k] for k in SNAPSHOTS])
    # stride through the pool so that small n still sees every depth
    idx = (np.arange(n) * (len(pool) // len(SNAPSHOTS) + 1)) % len(pool)
    out = np.ascontiguousarray(pool[idx])
    out.setflags(write=False)
    return out


def with_seat(rows, seat):
    """The rows with word 0's seat-to-act field (bits 13-15) set to `seat`."""
    r = np.array(rows, dtype=np.uint32)
    r[:, 0] = (r[:, 0] & ~np.uint32(7 << 13)) | np.uint32(seat << 13)
    return r


def pack_bits(obs):
    """int8 0/1 rows [n, L] -> the packed form [n, ceil(L / 32)] uint32 (bit i of the row = bit i & 31 of word i >> 5)."""
    obs = np.asarray(obs)
    n, L = obs.shape
    pad = np.zeros((n, (-L) % 32), np.uint8)
    return np.packbits(np.concatenate([obs.astype(np.uint8), pad], axis=1), axis=1, bitorder="little").view(np.uint32)
