"""hb_belief_determinize and hb_search_layout (csrc/belief.hip) on the deep rows of tests/deep_rows.py, all twelve variants: empty
decks, short hands through the explicit seat, finished rows, 4-player rows (hands of four, 48-word rows, the deck at word 22),
Very-Small with 5 players (no deck from the deal on). The kernel against the restatement of tests/test_search_cpu.py bit for bit,
against the properties tests/test_deep_rows_cpu.py holds the restatement to (the same checker, on the kernel's output: an error
the two share does not pass), against the encoder as every seat's eyes, and between guard bands."""
import numpy as np
import pytest

import deep_rows as DR
from guard_util import GuardSet
from search_util import _u32

pytestmark = pytest.mark.gpu

SEED, DRAW = 77, 5


def _setup(game, players):
    """(library config, oracle config, pick, its rows on the device)."""
    import torch

    import hanabi_hip
    from oracle import oracle_py as O

    p = DR.pick(game, players)
    rows = torch.from_numpy(np.array(p.rows).view(np.int32)).cuda()   # (a copy: pick's rows are read only)
    cfg, ocfg = hanabi_hip.make_config(game, players), O.make_config(game, players, 0)
    assert rows.shape[1] == (48 if players >= 4 else 32)
    assert (cfg.players, cfg.colors, cfg.ranks, cfg.hand_size) == (ocfg.players, ocfg.colors, ocfg.ranks, ocfg.hand_size)
    return cfg, ocfg, p, rows


@pytest.mark.parametrize("game,players", DR.VARIANTS)
def test_kernel_equals_the_restatement(game, players):
    """seat in (-1, 0 .. P - 1) x replicas in (1, 9): rows and weights bit for bit; once with row ids that cross 2^32; once split in
    two calls at m // 3."""
    import torch
    from test_search_cpu import determinize_ref

    from hanabi_hip import Determinizer

    cfg, ocfg, p, rows = _setup(game, players)
    m = len(p.rows)
    det = Determinizer(config=cfg)
    for seat in range(-1, players):
        for replicas in (1, 9):
            out, w = det.sample(rows, seat=seat, replicas=replicas, seed=SEED, draw=DRAW, first_row_id=1000)
            want, want_w = determinize_ref(ocfg, p.rows, seat, replicas, SEED, DRAW, first_row_id=1000)
            bad = np.flatnonzero((_u32(out) != want).any(1) | (w.cpu().numpy() != want_w.astype(np.int64)))
            assert not len(bad), (seat, replicas, "first differing output", int(bad[0]), "row of pick", int(bad[0]) // replicas,
                                  p.category[bad[0] // replicas])
    big = 2 ** 32 - 5
    out, w = det.sample(rows, seat=players - 1, replicas=9, seed=SEED, draw=DRAW, first_row_id=big)
    want, want_w = determinize_ref(ocfg, p.rows, players - 1, 9, SEED, DRAW, first_row_id=big)
    assert np.array_equal(_u32(out), want) and np.array_equal(w.cpu().numpy(), want_w.astype(np.int64))
    k = m // 3
    o1, w1 = det.sample(rows[:k], seat=players - 1, replicas=9, seed=SEED, draw=DRAW, first_row_id=big)
    o2, w2 = det.sample(rows[k:], seat=players - 1, replicas=9, seed=SEED, draw=DRAW, first_row_id=big + 9 * k)
    assert torch.equal(torch.cat([o1, o2]), out) and torch.equal(torch.cat([w1, w2]), w)


@pytest.mark.parametrize("game,players", DR.VARIANTS)
def test_kernel_output_has_the_properties(game, players):
    """deep_rows.check_determinized and assert_changes on the kernel's output, the restatement not asked: 6 replicas for seat
    -1 and for every explicit seat (a short row meets its short seat among them)."""
    from hanabi_hip import Determinizer

    cfg, ocfg, p, rows = _setup(game, players)
    det = Determinizer(config=cfg)
    total = np.zeros(6, np.int64)
    for seat in range(-1, players):
        out, w = det.sample(rows, seat=seat, replicas=6, seed=SEED + 1, draw=DRAW, first_row_id=10 ** 6 * (seat + 1))
        total += DR.check_determinized(ocfg, p.rows, seat, 6, _u32(out), w.cpu().numpy())
    print(f"{game} {players}: live outputs {total[0]}, changed {total[1]}; of rows that can change {total[2]}, changed {total[3]}; "
          f"of those with a pool of two cards {total[4]}, changed {total[5]}")
    assert total[0] >= 6 * (players + 1) * 20
    DR.assert_changes(total)


@pytest.mark.parametrize("game,players", [("Hanabi-Full", 2), ("Hanabi-Full", 4), ("Hanabi-Very-Small", 3)])
def test_a_seat_field_that_names_no_seat(game, players):
    """seat = -1 on running rows whose seat-to-act field was overwritten with P and with 7: unchanged copies of weight 0, as the
    restatement has it (the wrapper refuses an explicit seat >= P before the kernel sees it)."""
    import torch
    from encode_rows_util import with_seat
    from test_search_cpu import determinize_ref

    from hanabi_hip import Determinizer

    cfg, ocfg, p, _ = _setup(game, players)
    src = np.concatenate([with_seat(p.rows[p.category == "deck"][:5], players), with_seat(p.rows[p.category == "deck0"][:5], 7),
                          p.rows[:3]])
    rows = torch.from_numpy(src.view(np.int32)).cuda()
    out, w = Determinizer(config=cfg).sample(rows, seat=-1, replicas=3, seed=SEED, draw=DRAW)
    want, want_w = determinize_ref(ocfg, src, -1, 3, SEED, DRAW)
    assert np.array_equal(_u32(out), want) and np.array_equal(w.cpu().numpy(), want_w.astype(np.int64))
    assert not w[:30].any() and np.array_equal(_u32(out)[:30], np.repeat(src[:10], 3, 0)) and bool(w[30:].any())
    DR.check_determinized(ocfg, src, -1, 3, _u32(out), w.cpu().numpy())


@pytest.mark.parametrize("game,players", DR.VARIANTS)
def test_no_seat_can_tell(game, players):
    """The rows determinized for seat o (and, seat = -1, for each row's seat to act) look to seat o exactly like their source:
    hb_encode_rows' observation bits and legal mask of the live replicas (tests/test_encode_rows_gpu.py pins the encoder to the
    oracle on all twelve variants)."""
    import torch

    from hanabi_hip import Determinizer, encode_rows

    cfg, _, p, rows = _setup(game, players)
    R = 6
    src = rows.repeat_interleave(R, 0).contiguous()
    det = Determinizer(config=cfg)
    changed = 0
    for seat in range(-1, players):
        out, w = det.sample(rows, seat=seat, replicas=R, seed=4, draw=2, first_row_id=7 * (seat + 1))
        eye = None if seat < 0 else seat
        obs, legal = encode_rows(cfg, out, seat=eye)
        obs0, legal0 = encode_rows(cfg, src, seat=eye)
        live = w > 0
        assert int(live.sum()) > len(p.rows)
        assert torch.equal(obs[live], obs0[live]) and torch.equal(legal[live], legal0[live]), seat
        assert torch.equal(out[~live], src[~live])
        changed += int((out[live] != src[live]).any(1).sum())
    assert changed > 0


@pytest.mark.parametrize("game,players", [("Hanabi-Very-Small", 5), ("Hanabi-Full", 4), ("Hanabi-Small", 3)])
@pytest.mark.parametrize("replicas", [1, 3])
def test_guard_bands(game, players, replicas):
    """Rows and weights in guarded buffers (a workgroup's four rows behind the rows), the source registered as an input: the two
    48-word variants no test had launched, and a 32-word one with three players. m * replicas is no multiple of 4."""
    import torch
    from test_search_cpu import determinize_ref

    from hanabi_hip import Determinizer

    cfg, ocfg, p, rows = _setup(game, players)
    m, SW = rows.shape
    assert (m * replicas) % 4 != 0
    det = Determinizer(config=cfg)
    for seat in (-1, players - 1):
        gs = GuardSet("hb_belief_determinize")
        gs.inp("src_rows", rows)
        out = gs.out("rows_out", (m * replicas, SW), torch.int32, 4 * SW)
        w = gs.out("weights", (m * replicas,), torch.int32, 64)
        det.sample(rows, seat=seat, replicas=replicas, seed=SEED, draw=DRAW, first_row_id=3, out=(out, w))
        torch.cuda.synchronize()
        gs.check(f"{game} {players} seat={seat} replicas={replicas}")
        assert not gs.untouched()
        want, want_w = determinize_ref(ocfg, p.rows, seat, replicas, SEED, DRAW, first_row_id=3)
        assert np.array_equal(_u32(out), want) and np.array_equal(_u32(w), want_w)


@pytest.mark.parametrize("game,players", [("Hanabi-Full", 4), ("Hanabi-Very-Small", 5)])
def test_layout_of_deep_rows(game, players):
    """hb_search_layout on the determinized deep rows (48-word rows; finished roots whose replicas weigh nothing) against
    the numpy gather of tests/test_search_confirm_gpu.py: R = 3, candidate lists of 1 and 3 slots with -1 among them."""
    import torch
    from test_search_confirm_gpu import layout_by_gather

    from hanabi_hip import Determinizer
    from hanabi_hip.search import search_layout

    cfg, _, p, rows = _setup(game, players)
    m, SW = rows.shape
    R, A = 3, 2 * cfg.hand_size + (players - 1) * (cfg.colors + cfg.ranks)
    det_rows, w = Determinizer(config=cfg).sample(rows, seat=players - 1, replicas=R, seed=5, draw=2, out=(
        torch.empty((m * R, SW), dtype=torch.int32, device="cuda"), torch.empty(m * R, dtype=torch.int32, device="cuda")))
    dn, wn = det_rows.cpu().numpy(), _u32(w)
    finished = np.flatnonzero(p.category == "finished")
    assert (wn.reshape(m, R)[finished] == 0).all() and (wn > 0).any()
    rng = np.random.default_rng(7)
    for Cn in (1, 3):
        cand = rng.integers(0, A, (m, Cn)).astype(np.int32)
        cand[0] = -1              # a row of all -1
        cand[1, 0] = -1           # -1 in slot 0 only
        cand[2:, Cn - 1][::3] = -1   # -1 in the last slot of every third root
        filler = rng.integers(0, A, m).astype(np.int32)
        got = search_layout(cfg, det_rows, w, torch.as_tensor(cand).cuda(), torch.as_tensor(filler).cuda(), R)
        want = layout_by_gather(dn, wn, cand, filler, R)
        for name, g, e in zip(("rows", "forced", "done", "n_played"), got, want):
            assert np.array_equal(g.cpu().numpy(), e), (name, Cn)
        assert got[3][0] == 0 and int(got[3].sum()) > 0
