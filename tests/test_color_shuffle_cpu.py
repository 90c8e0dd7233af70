"""Colour-permuted frames without a GPU: the host helpers of hanabi_hip.symmetry (permutation order, round trips, composition,
colour-free sections untouched) and the argument checks of the new entry points."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

VARIANTS = [(g, p) for g in ("Hanabi-Full", "Hanabi-Small", "Hanabi-Very-Small") for p in (2, 3, 4, 5)]


def _cfg(game, players):
    import hanabi_hip

    return hanabi_hip.make_config(game, players)


def _random_perms(rng, n, P, C):
    return np.stack([np.stack([rng.permutation(C) for _ in range(P)]) for _ in range(n)]).astype(np.uint8)


def _pack(bits):
    n, L = bits.shape
    w = (L + 31) // 32
    pad = np.zeros((n, w * 32), np.uint64)
    pad[:, :L] = bits
    return (pad.reshape(n, w, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32).view(np.int32)


@pytest.mark.parametrize("C_", [1, 2, 3, 4, 5])
def test_permutation_lists_all_in_lexicographic_order(C_):
    from hanabi_hip import symmetry as S

    got = [tuple(S.permutation(i, C_)) for i in range(math.factorial(C_))]
    assert got == list(itertools.permutations(range(C_)))
    assert tuple(S.permutation(0, C_)) == tuple(range(C_))
    with pytest.raises(ValueError):
        S.permutation(math.factorial(C_), C_)
    assert S.perm_index(0, C_) == 0 and S.perm_index(2 ** 32 - 1, C_) == math.factorial(C_) - 1


def test_layout_matches_the_library():
    import hanabi_hip
    from hanabi_hip import symmetry as S

    L = hanabi_hip.lib()
    for game, players in VARIANTS:
        cfg = _cfg(game, players)
        lay = S.layout(cfg)
        assert lay["OBS_LEN"] == L.hb_obs_len(C.byref(cfg))
        assert lay["A"] == L.hb_num_actions(C.byref(cfg))
        assert lay["D"] == L.hb_deck_size(C.byref(cfg))


@pytest.mark.parametrize("game,players", VARIANTS)
def test_obs_round_trip_and_composition(game, players):
    from hanabi_hip import symmetry as S

    cfg = _cfg(game, players)
    lay = S.layout(cfg)
    rng = np.random.default_rng(players * 7 + cfg.colors)
    n = 64
    obs = (rng.random((n, lay["OBS_LEN"])) < 0.3).astype(np.int8)
    seat = rng.integers(0, players, n)
    sig = _random_perms(rng, n, players, cfg.colors)
    tau = _random_perms(rng, n, players, cfg.colors)
    y = S.permute_obs(obs, sig, seat, cfg)
    assert y.dtype == np.int8 and y.shape == obs.shape and (y.sum(axis=1) == obs.sum(axis=1)).all()
    assert np.array_equal(S.permute_obs(y, S.invert(sig), seat, cfg), obs)
    # sigma o tau: tau first, then sigma
    assert np.array_equal(S.permute_obs(S.permute_obs(obs, tau, seat, cfg), sig, seat, cfg),
                          S.permute_obs(obs, S.compose(sig, tau), seat, cfg))
    # packed rows take the same map
    assert np.array_equal(S.permute_obs(_pack(obs), sig, seat, cfg), _pack(y))
    # identity permutations change nothing
    ident = np.broadcast_to(np.arange(cfg.colors, dtype=np.uint8), sig.shape)
    assert np.array_equal(S.permute_obs(obs, ident, seat, cfg), obs)


def _colour_free_positions(cfg):
    """Every observation position outside the colour-carrying fields, from the section sizes alone."""
    P, Cc, R, H = cfg.players, cfg.colors, cfg.ranks, cfg.hand_size
    bits = Cc * R
    D = Cc * sum(3 if r == 0 else (1 if r == R - 1 else 2) for r in range(R))
    pos, free = 0, []
    pos += (P - 1) * H * bits                          # other hands: colour
    free += range(pos, pos + P + D - P * H)            # hand-short flags, deck thermometer
    pos += P + D - P * H
    pos += bits                                        # fireworks: colour
    free += range(pos, pos + cfg.max_info + cfg.max_life)
    pos += cfg.max_info + cfg.max_life
    pos += D                                           # discards: colour
    free += range(pos, pos + P + 4 + P)                # last move: actor, type, target
    pos += P + 4 + P
    pos += Cc                                          # revealed colour
    free += range(pos, pos + R + H + H)                # revealed rank, revealed slots, card slot
    pos += R + H + H
    pos += bits                                        # card played / discarded
    free += range(pos, pos + 2)                        # scored, information token
    pos += 2
    for _ in range(P * H):
        pos += bits + Cc                               # plausible identities, revealed colour
        free += range(pos, pos + R)                    # revealed rank
        pos += R
    return np.array(free, dtype=np.int64), pos


@pytest.mark.parametrize("game,players", VARIANTS)
def test_colour_free_sections_untouched(game, players):
    from hanabi_hip import symmetry as S

    cfg = _cfg(game, players)
    free, L = _colour_free_positions(cfg)
    assert L == S.layout(cfg)["OBS_LEN"]
    rng = np.random.default_rng(11)
    n = 128
    obs = (rng.random((n, L)) < 0.5).astype(np.int8)
    sig = _random_perms(rng, n, players, cfg.colors)
    y = S.permute_obs(obs, sig, 0, cfg)
    assert np.array_equal(y[:, free], obs[:, free])
    if cfg.colors > 1:   # and something colour-carrying did move
        assert not np.array_equal(y, obs)


def test_known_fields_move_by_colour_block():
    """Full 2-player: the partner's card (c, r), firework c and the discard block of c land at colour sigma(c)."""
    from hanabi_hip import symmetry as S

    cfg = _cfg("Hanabi-Full", 2)
    lay = S.layout(cfg)
    sig = np.array([[[3, 0, 4, 1, 2], [0, 1, 2, 3, 4]]], np.uint8)
    obs = np.zeros((1, lay["OBS_LEN"]), np.int8)
    obs[0, 1 * 5 + 2] = 1                               # slot 0 of the partner: colour 1, rank 2
    obs[0, lay["FW_OFF"] + 4 * 5 + 0] = 1               # firework of colour 4 at 1
    obs[0, lay["DISC_OFF"] + 2 * lay["CPC"] + 1] = 1    # a discarded card of colour 2
    obs[0, lay["O4"] + 0] = 1                           # the last move revealed colour 0
    y = S.permute_obs(obs, sig, 0, cfg)[0]
    assert y[0 * 5 + 2] == 1 and y[lay["FW_OFF"] + 2 * 5] == 1 and y[lay["DISC_OFF"] + 4 * lay["CPC"] + 1] == 1 and y[lay["O4"] + 3] == 1
    assert y.sum() == 4
    assert np.array_equal(S.permute_obs(obs, sig, 1, cfg), obs)   # seat 1 keeps the identity


@pytest.mark.parametrize("game,players", VARIANTS)
def test_actions_and_legal(game, players):
    from hanabi_hip import symmetry as S

    cfg = _cfg(game, players)
    lay = S.layout(cfg)
    rng = np.random.default_rng(5)
    A, H, Cc = lay["A"], cfg.hand_size, cfg.colors
    n = A * 4
    acts = np.tile(np.arange(A, dtype=np.int32), 4)
    seat = rng.integers(0, players, n)
    sig = _random_perms(rng, n, players, Cc)
    fwd = S.permute_actions(acts, sig, seat, cfg)
    assert fwd.dtype == np.int32
    assert np.array_equal(S.unpermute_actions(fwd, sig, seat, cfg), acts)
    rc = (acts >= 2 * H) & (acts < 2 * H + (players - 1) * Cc)
    assert np.array_equal(fwd[~rc], acts[~rc])
    s = sig[np.arange(n), seat].astype(np.int64)
    xc = acts[rc] - 2 * H
    assert np.array_equal(fwd[rc], 2 * H + (xc // Cc) * Cc + s[rc][np.arange(rc.sum()), xc % Cc])
    legal = (rng.random((n, A)) < 0.5).astype(np.int8)
    pl = S.permute_legal(legal, sig, seat, cfg)
    assert np.array_equal(pl[np.arange(n), fwd], legal[np.arange(n), acts])   # move u legal <=> its image is legal
    assert np.array_equal(S.permute_legal(pl, S.invert(sig), seat, cfg), legal)


def test_torch_tensors_come_back_as_tensors():
    import torch

    from hanabi_hip import symmetry as S

    cfg = _cfg("Hanabi-Small", 3)
    lay = S.layout(cfg)
    obs = torch.randint(0, 2, (8, lay["OBS_LEN"]), dtype=torch.int8)
    perms = torch.tensor(np.array([[[1, 0]] * 3] * 8), dtype=torch.uint8)
    y = S.permute_obs(obs, perms, torch.zeros(8, dtype=torch.int64), cfg)
    assert isinstance(y, torch.Tensor) and y.dtype == torch.int8
    assert torch.equal(S.permute_obs(y, perms, 0, cfg), obs)


def test_seat_mask():
    from hanabi_hip import symmetry as S

    assert S.seat_mask(True, 3) == 7 and S.seat_mask(False, 3) == 0 and S.seat_mask(None, 5) == 0
    assert S.seat_mask((0, 2), 3) == 5 and S.seat_mask(2, 2) == 2
    for bad in ((3,), (-1,), 8, -1):
        with pytest.raises(ValueError):
            S.seat_mask(bad, 3)


def test_entry_points_reject_null_env_and_bad_masks():
    import hanabi_hip

    L = hanabi_hip.lib()
    assert L.hb_env_set_color_shuffle(None, None, 1, None) != 0 and b"null env" in L.hb_last_error()
    assert L.hb_env_set_color_shuffle(None, None, 0x40, None) != 0 and b"seat" in L.hb_last_error()
    assert L.hb_env_set_color_shuffle(None, C.c_void_p(16), 1, None) != 0 and b"not both" in L.hb_last_error()
    assert L.hb_env_color_perms(None, C.c_void_p(16), None) != 0 and b"null env" in L.hb_last_error()
    assert L.hb_env_set_color_perms(None, C.c_void_p(16), None) != 0 and b"null env" in L.hb_last_error()
    assert L.hb_env_color_shuffled(None) == 0
    assert L.hb_actor_fused_step_supported(None) == 0
