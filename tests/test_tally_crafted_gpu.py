"""GPU: hb_eval_tally, hb_eval_tally_grouped, hb_train_tally and hb_train_tally_init (csrc/eval.hip, csrc/eval_tally.hpp,
csrc/train_tally.hip) against the per-game models of tests/tally_cases.py on its crafted steps, after every call, every comparison
exact. Played games never choose what sits in a wavefront and uniform-random play ends every game at score 0; here every lane is
chosen: 64 lanes on one score, as many scores as bins, a lone lane 0 or 63, a ragged last wave, the top bin, counters across 2^32,
lengths at the int16 limit, 64 members, a second pass of the grid-stride loop. The last leg plays an auto-reset env with the
open-handed driver, so hb_train_tally also sees an env's own outputs with real points in them."""
import ctypes as C

import numpy as np
import pytest

import deep_play as D
import tally_cases as T

pytestmark = pytest.mark.gpu

NEAR = (1 << 32) - 3                    # counters so far: the first adds carry into the high word
STEP_KEYS = ("actions", "reward", "terminal", "score")


def _setup(game, players, flags=0):
    import hanabi_hip

    L = hanabi_hip.lib()
    cfg = hanabi_hip.make_config(game, players, flags)
    d = T.dims_of(cfg)
    assert d.A == L.hb_num_actions(C.byref(cfg)) and d.deck == L.hb_deck_size(C.byref(cfg))
    assert T.eval_counters(d) == L.hb_eval_counters(C.byref(cfg)) and T.train_counters(d) == L.hb_train_counters(C.byref(cfg))
    return L, cfg, d


def _cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ins(step):
    return [_cuda(step[k]) for k in STEP_KEYS]


def _eval_call(L, cfg, n, seat, turn, ins, done, final, length, counters):
    from hanabi_hip import _capi as K

    K.check(L.hb_eval_tally(C.byref(cfg), n, seat, turn, *(K.dptr(x) for x in ins), K.dptr(done), K.dptr(final), K.dptr(length),
                            K.dptr(counters), K.current_stream()))


def _train_call(L, cfg, n, seat, ins, tm, n_members, lost, length, counters):
    from hanabi_hip import _capi as K

    K.check(L.hb_train_tally(C.byref(cfg), n, seat, *(K.dptr(x) for x in ins), K.dptr(tm), n_members, K.dptr(lost), K.dptr(length),
                             K.dptr(counters), K.current_stream()))


# ---- hb_eval_tally -----------------------------------------------------------------------------------------------------------------

def _check_eval(game, players, n, turns=6, turn0=0, base=0):
    import torch

    L, cfg, d = _setup(game, players)
    cr = T.crafted_steps(d, n, turns, seed=1000 * players + n)
    c0 = [int((cr.done0 & 0x80 == 0).sum())] + [base] * (T.eval_counters(d) - 1)
    g_done, g_final, g_len = _cuda(cr.done0), _cuda(np.full(n, -1, np.int8)), _cuda(np.full(n, -1, np.int16))
    g_c = torch.tensor(c0, dtype=torch.int64, device="cuda")
    for (t, done, final, length, c), step in zip(T.eval_run(d, cr, turn0, c0), cr.steps):
        ins = _ins(step)
        _eval_call(L, cfg, n, (turn0 + t) % d.P, turn0 + t, ins, g_done, g_final, g_len, g_c)
        assert g_c.cpu().tolist() == c, t
        assert np.array_equal(g_done.cpu().numpy(), done), t
        assert np.array_equal(g_final.cpu().numpy(), final), t
        assert np.array_equal(g_len.cpu().numpy(), length), t
        for x, k in zip(ins, STEP_KEYS):
            assert np.array_equal(x.cpu().numpy(), step[k]), k                    # read only
    never = g_done.cpu().numpy() & 0x80 == 0
    never |= cr.done0 & 0x80 != 0
    assert (g_final.cpu().numpy()[never] == -1).all() and (g_len.cpu().numpy()[never] == -1).all()
    assert g_c[0].item() == int((g_done.cpu().numpy() & 0x80 == 0).sum())
    return c


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257, 300])
@pytest.mark.parametrize("game,players", T.VARIANTS)
def test_eval_tally_equals_the_model_after_every_turn(game, players, n):
    """n = 1: a lone lane; 63 / 64 / 65: a wavefront boundary; 255 / 257: a workgroup boundary; 300: two workgroups and a ragged
    last wave in which games end. Six consecutive turns, seat = turn mod P."""
    c = _check_eval(game, players, n)
    if n >= 255:
        assert all(x > 0 for x in c[1:])             # every bin (the top one too), bomb-outs, every (seat, kind), every seat's misplays


@pytest.mark.parametrize("game,players", T.VARIANTS)
def test_eval_tally_at_the_last_turns_int16_holds(game, players):
    """Turns 32 761 .. 32 766: the lengths written are 32 762 .. 32 767."""
    _check_eval(game, players, 300, turn0=32761)


@pytest.mark.parametrize("game,players", T.VARIANTS)
def test_eval_tally_counters_cross_2_pow_32(game, players):
    """Every counter but the live count starts at 2^32 - 3: adding is adding, whatever is there."""
    c = _check_eval(game, players, 300, base=NEAR)
    assert max(c) > 1 << 32


def test_eval_tally_grid_stride_second_pass():
    """128 workgroups of 256 lanes cover 32 768 games: 70 more take the loop round again in one workgroup."""
    _check_eval("Hanabi-Full", 5, 128 * 256 + 70, turns=1)


def _one_game(game, players, uid, reward, terminal, score, done=0):
    import torch

    L, cfg, d = _setup(game, players)
    ins = [torch.tensor([uid], dtype=torch.int32), torch.tensor([reward], dtype=torch.float32),
           torch.tensor([terminal], dtype=torch.int8), torch.tensor([score], dtype=torch.int8)]
    return L, cfg, d, [x.cuda() for x in ins]


@pytest.mark.parametrize("uid_off", [-1, 0])          # uid -1 and uid A
@pytest.mark.parametrize("terminal", [0, 1])
def test_a_uid_outside_the_range_is_no_move(uid_off, terminal):
    """include/hanabi_hip.h: no kind, no misplay (reward 0 would make a play one); the step counts towards the length and a
    terminal still ends the game. Both tallies, one game (hb_train_tally: one tile, the game in its lane 0)."""
    import torch

    L, cfg, d, ins = _one_game("Hanabi-Small", 3, 0, 0.0, terminal, 4)
    ins[0][0] = -1 if uid_off else d.A
    B = d.B
    done = torch.zeros(1, dtype=torch.uint8, device="cuda")
    final, length = torch.full((1,), -1, dtype=torch.int8, device="cuda"), torch.full((1,), -1, dtype=torch.int16, device="cuda")
    c = torch.zeros(T.eval_counters(d), dtype=torch.int64, device="cuda")
    c[0] = 1
    _eval_call(L, cfg, 1, 1, 6, ins, done, final, length, c)
    want = [0] * T.eval_counters(d)
    want[0], want[1 + 4] = 1 - terminal, terminal
    assert c.tolist() == want
    assert (done.item(), final.item(), length.item()) == ((0x80, 4, 7) if terminal else (0, -1, -1))
    tile = [torch.cat([x, torch.zeros(127, dtype=x.dtype, device="cuda")]) for x in ins]
    tile[0][1:] = 0                                    # the other 127 games discard slot 0 and go on
    lost = torch.zeros(128, dtype=torch.uint8, device="cuda")
    length = torch.full((128,), 9, dtype=torch.int16, device="cuda")
    c = torch.zeros(1, T.train_counters(d), dtype=torch.int64, device="cuda")
    _train_call(L, cfg, 128, 1, tile, torch.zeros(1, dtype=torch.int32, device="cuda"), 1, lost, length, c)
    want = [0] * T.train_counters(d)
    want[6 + B + 4 * 1 + 0] = 127
    if terminal:
        want[0], want[1], want[2], want[3 + 4], want[4 + B], want[5 + B] = 1, 4, 16, 1, 10, 1
    assert c[0].tolist() == want and not lost.any()
    assert length.tolist() == [0 if terminal else 10] + [10] * 127


@pytest.mark.parametrize("score,bin_", [(-3, 0), (127, 10), (11, 10)])
def test_a_score_outside_the_bins_counts_in_the_nearest_end_bin(score, bin_):
    """include/hanabi_hip.h: hb_eval_tally stores the raw value in final_score; hb_train_tally adds the clamped one to its sums."""
    import torch

    L, cfg, d, ins = _one_game("Hanabi-Small", 3, 1, 0.0, 1, score)
    B = d.B
    done, final, length = (torch.zeros(1, dtype=t, device="cuda") for t in (torch.uint8, torch.int8, torch.int16))
    c = torch.zeros(T.eval_counters(d), dtype=torch.int64, device="cuda")
    c[0] = 1
    _eval_call(L, cfg, 1, 0, 0, ins, done, final, length, c)
    want = [0] * T.eval_counters(d)
    want[1 + bin_], want[2 + B + 0] = 1, 1
    assert c.tolist() == want and (done.item(), final.item(), length.item()) == (0x80, score, 1)
    tile = [torch.cat([x, torch.zeros(127, dtype=x.dtype, device="cuda")]) for x in ins]
    lost = torch.zeros(128, dtype=torch.uint8, device="cuda")
    length = torch.zeros(128, dtype=torch.int16, device="cuda")
    c = torch.zeros(1, T.train_counters(d), dtype=torch.int64, device="cuda")
    _train_call(L, cfg, 128, 0, tile, torch.zeros(1, dtype=torch.int32, device="cuda"), 1, lost, length, c)
    want = [0] * T.train_counters(d)
    want[0], want[1], want[2], want[3 + bin_], want[4 + B], want[5 + B], want[6 + B + 0] = 1, bin_, bin_ * bin_, 1, 1, 1, 128
    assert c[0].tolist() == want


# ---- hb_eval_tally_grouped ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("game,players", [("Hanabi-Full", 2), ("Hanabi-Small", 3)])
def test_eval_tally_grouped_equals_the_model_on_every_slice(game, players):
    """3 blocks of 70 games (block offsets 70 and 140: no multiple of 64), two turns; every game of block 1 was finished before, and
    its counters, status, scores and lengths stay as they were."""
    import torch

    from hanabi_hip import _capi as K

    L, cfg, d = _setup(game, players)
    nb, bg, nc = 3, 70, T.eval_counters(d)
    cr = T.crafted_steps(d, nb * bg, 2, seed=31 + players)
    cr.done0[bg:2 * bg] |= 0x80
    cr.done0[0] = cr.done0[2 * bg] = 0
    blocks = [T.Crafted([{k: s[k][b * bg:(b + 1) * bg] for k in STEP_KEYS} for s in cr.steps], cr.done0[b * bg:(b + 1) * bg], None, None, None)
              for b in range(nb)]
    c0 = [[int((blk.done0 & 0x80 == 0).sum())] + [5 + b] * (nc - 1) for b, blk in enumerate(blocks)]
    assert c0[1][0] == 0
    g_done, g_final, g_len = _cuda(cr.done0), _cuda(np.full(nb * bg, -1, np.int8)), _cuda(np.full(nb * bg, -1, np.int16))
    g_c = torch.tensor(c0, dtype=torch.int64, device="cuda")
    runs = [T.eval_run(d, blk, 3, c0[b]) for b, blk in enumerate(blocks)]
    for t, step in enumerate(cr.steps):
        ins = _ins(step)
        K.check(L.hb_eval_tally_grouped(C.byref(cfg), nb, bg, (3 + t) % d.P, 3 + t, *(K.dptr(x) for x in ins), K.dptr(g_done),
                                        K.dptr(g_final), K.dptr(g_len), K.dptr(g_c), K.current_stream()))
        for b, run in enumerate(runs):
            _, done, final, length, c = next(run)
            sl = slice(b * bg, (b + 1) * bg)
            assert g_c[b].cpu().tolist() == c, (t, b)
            assert np.array_equal(g_done.cpu().numpy()[sl], done) and np.array_equal(g_final.cpu().numpy()[sl], final), (t, b)
            assert np.array_equal(g_len.cpu().numpy()[sl], length), (t, b)
    assert g_c[1].tolist() == c0[1] and g_c[0].tolist() != c0[0] and g_c[2].tolist() != c0[2]
    assert np.array_equal(g_done.cpu().numpy()[bg:2 * bg], cr.done0[bg:2 * bg])
    assert (g_final[bg:2 * bg] == -1).all() and (g_len[bg:2 * bg] == -1).all()


# ---- hb_train_tally ------------------------------------------------------------------------------------------------------------------

def _tiles(n_tiles, n_members):
    """The member of every tile. 5 tiles (n = 640): the last member owns tiles 0 and 2 (not adjacent), and shares the first
    256-lane workgroup with member 0; tile 3 is nobody's (-1) and tile 4 names a member that is not there."""
    last = n_members - 1
    return np.array({1: [last], 2: [last, 0] if n_members > 1 else [0, -1], 3: [last, n_members, last],
                     5: [last, 0, last, -1, n_members]}[n_tiles], np.int32)


def _check_train(game, players, n, n_members, tile_member, turns=6, base=0):
    import torch

    L, cfg, d = _setup(game, players)
    cr = T.crafted_steps(d, n, turns, seed=77 * players + n + n_members, p_end=0.3)
    nc = T.train_counters(d)
    c0 = [[base] * nc for _ in range(n_members)]
    g_lost, g_len, g_tm = _cuda(cr.lost0), _cuda(cr.length0), _cuda(tile_member)
    g_c = torch.tensor(c0, dtype=torch.int64, device="cuda")
    for (t, lost, length, c), step in zip(T.train_run(d, cr, tile_member, n_members, seat0=1, counters0=c0), cr.steps):
        ins = _ins(step)
        _train_call(L, cfg, n, (1 + t) % d.P, ins, g_tm, n_members, g_lost, g_len, g_c)
        assert g_c.cpu().tolist() == c, t
        assert np.array_equal(g_lost.cpu().numpy(), lost), t
        assert np.array_equal(g_len.cpu().numpy(), length), t
        for x, k in zip(ins, STEP_KEYS):
            assert np.array_equal(x.cpu().numpy(), step[k]), k                    # read only
    owned = np.repeat((tile_member >= 0) & (tile_member < n_members), T.TILE)
    assert np.array_equal(g_lost.cpu().numpy()[~owned], cr.lost0[~owned]) and np.array_equal(g_len.cpu().numpy()[~owned], cr.length0[~owned])
    for m in range(n_members):
        if m not in tile_member.tolist():
            assert g_c[m].tolist() == c0[m], m                                    # a member without a tile: its row is untouched
    return c


@pytest.mark.parametrize("n_members", [1, 3, 64])
@pytest.mark.parametrize("n", [128, 256, 384, 640])
@pytest.mark.parametrize("game,players", T.VARIANTS)
def test_train_tally_equals_the_model_after_every_step(game, players, n, n_members):
    """One tile; one workgroup of two tiles; a second workgroup of one tile; three workgroups, the last half empty. 1, 3 and
    HB_TRAIN_MAX_MEMBERS members (the LDS rows of all of them are zeroed and flushed). Six steps, seat = (1 + t) mod P."""
    tm = _tiles(n // T.TILE, n_members)
    c = _check_train(game, players, n, n_members, tm)
    B = T.dims_of(_setup(game, players)[1]).B
    row = c[n_members - 1]
    assert row[2] > row[1] > row[0] > 0 and row[3 + B] > 0 and row[5 + B] > row[3 + B] and row[4 + B] > 32767


@pytest.mark.parametrize("game,players", T.VARIANTS)
def test_train_tally_counters_cross_2_pow_32(game, players):
    """Every counter starts at 2^32 - 3. Members 2 and 0 own tiles; member 1 owns none and keeps its row."""
    c = _check_train(game, players, 640, 3, _tiles(5, 3), base=NEAR)
    assert max(c[2]) > 1 << 32 and max(c[0]) > 1 << 32 and c[1] == [NEAR] * len(c[1])


def test_train_tally_grid_stride_second_pass():
    """128 workgroups of 256 lanes cover 32 768 games: one more tile takes the loop round again, in the workgroup that has tiles 0
    and 1. 257 tiles over 64 members, some of nobody (-1) and some of a member that is not there (64); two steps."""
    n = 128 * 256 + 128
    tm = (np.arange(n // T.TILE, dtype=np.int32) * 5) % 66 - 1
    assert tm.min() == -1 and tm.max() == 64 and tm[0] != tm[256]
    _check_train("Hanabi-Full", 5, n, 64, tm, turns=2)


# ---- hb_train_tally_init ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pre", [0, 3])
@pytest.mark.parametrize("game,players", T.VARIANTS)
def test_train_tally_init_equals_the_model_on_exported_rows(game, players, pre):
    import torch

    import hanabi_hip
    from hanabi_hip import _capi as K

    L, cfg, d = _setup(game, players, D.FLAGS)
    n = 300
    env = hanabi_hip.HanabiEnv(config=cfg, n_games=n, seed=players + pre)
    for t in range(pre):
        env.step(env.random_legal_actions(seed=2, draw=100 + t))
    rows = env.export_state()
    assert rows.shape == (n, env.state_words)
    lost = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    length = torch.full((n,), 7, dtype=torch.int16, device="cuda")
    K.check(L.hb_train_tally_init(C.byref(cfg), K.dptr(rows), n, K.dptr(lost), K.dptr(length), K.current_stream()))
    want_lost, want_len = T.train_tally_init_model(d, rows.cpu().numpy())
    assert np.array_equal(lost.cpu().numpy(), want_lost) and np.array_equal(length.cpu().numpy(), want_len)
    assert not want_lost.any() if pre == 0 else (want_lost == 0x80).any()


# ---- played, with real points ----------------------------------------------------------------------------------------------------------

# What the CPU oracle gives for the same driver, seeds and 256 games (episodes; endings above score 0, at the maximum score, with
# lives left), measured when this test was written; the floors are at most half of it.
PLAYED = {
    ("Hanabi-Small", 3): dict(steps=80, measured=(889, 704, 428, 704), floors=(350, 210, 350)),
    ("Hanabi-Full", 2): dict(steps=200, measured=(787, 737, 426, 737), floors=(360, 210, 360)),
}


@pytest.mark.parametrize("game,players", list(PLAYED))
def test_train_tally_on_played_games_with_real_points(game, players):
    """An auto-reset env of 256 games, tile members [0, 1], driven by deep_play.open_hand_moves on its exported rows with 5 % random
    moves; hb_train_tally after every step. The counters equal the model fed with the env's own outputs, and the members' episodes
    and score sums add up to the env's episode statistics."""
    import torch

    import hanabi_hip
    from hanabi_hip import _capi as K

    L, cfg, d = _setup(game, players, D.FLAGS)
    n, case = 256, PLAYED[(game, players)]
    env = hanabi_hip.HanabiEnv(config=cfg, n_games=n, seed=D.SEED, first_game_id=D.FIRST_GAME_ID)
    rng = np.random.default_rng(D.SEED)
    tm = np.array([0, 1], np.int32)
    g_tm = _cuda(tm)
    g_lost = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    g_len = torch.full((n,), 7, dtype=torch.int16, device="cuda")
    g_c = torch.zeros(2, T.train_counters(d), dtype=torch.int64, device="cuda")
    rows = env.export_state()
    K.check(L.hb_train_tally_init(C.byref(cfg), K.dptr(rows), n, K.dptr(g_lost), K.dptr(g_len), K.current_stream()))
    lost, length = T.train_tally_init_model(d, rows.cpu().numpy())
    assert not lost.any() and np.array_equal(g_lost.cpu().numpy(), lost)
    c = [[0] * T.train_counters(d) for _ in range(2)]
    for t in range(case["steps"]):
        act = D.open_hand_moves(cfg, env.export_state().cpu().numpy(), env.legal.cpu().numpy(), rng, D.P_RAND)
        g_act = _cuda(act)
        env.step(g_act)
        _train_call(L, cfg, n, t % players, [g_act, env.reward, env.terminal, env.score], g_tm, 2, g_lost, g_len, g_c)
        lost, length, c = T.train_tally_model(d, t % players, act, env.reward.cpu().numpy(), env.terminal.cpu().numpy(),
                                              env.score.cpu().numpy(), tm, 2, lost, length, c)
        assert g_c.cpu().tolist() == c, t
        assert np.array_equal(g_lost.cpu().numpy(), lost) and np.array_equal(g_len.cpu().numpy(), length), t
    B = d.B
    episodes, score_sum = env.stats()
    assert env.illegal_count() == 0
    assert c[0][0] + c[1][0] == episodes and c[0][1] + c[1][1] == score_sum
    got = (episodes - c[0][3] - c[1][3], c[0][3 + B - 1] + c[1][3 + B - 1], sum(r[5 + B] - r[3 + B] for r in c))
    print(f"{game} {players}: episodes {episodes}; endings above 0, at the maximum, with lives left {got}; measured on the oracle "
          f"{case['measured']}")
    assert all(2 * f <= m for f, m in zip(case["floors"], case["measured"][1:]))
    assert all(g >= f for g, f in zip(got, case["floors"])), got
    assert all(r[2] > r[1] > 0 for r in c)
