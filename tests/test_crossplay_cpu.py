"""Cross-play (hanabi_hip.crossplay, the grouped kernels of csrc/actor_fused.hip, rule_agent.hip and eval.hip), the parts that need
no GPU: team enumeration and validation, the block / chunk arithmetic, construction, and the new entry points' argument checks."""
import ctypes as C

import pytest


def test_default_teams_two_and_five_players():
    from hanabi_hip.crossplay import default_teams

    t2 = default_teams(3, 2)
    assert t2 == [(i, j) for i in range(3) for j in range(3)]
    t5 = default_teams(4, 5)
    assert len(t5) == 16 and t5[0] == (0, 0, 0, 0, 0) and t5[1] == (0, 1, 1, 1, 1) and t5[-1] == (3, 3, 3, 3, 3)
    assert all(t[1:] == (t[1],) * 4 for t in t5)
    assert sorted({(t[0], t[1]) for t in t5}) == [(i, j) for i in range(4) for j in range(4)]
    assert default_teams(1, 2) == [(0, 0)]
    with pytest.raises(ValueError):
        default_teams(0, 2)


def test_explicit_team_validation():
    from hanabi_hip.crossplay import check_teams

    assert check_teams([(0, 3), [3, 0]], 4, 2) == [(0, 3), (3, 0)]
    with pytest.raises(ValueError, match="one pool index per seat"):
        check_teams([(0, 1, 2)], 4, 2)
    with pytest.raises(ValueError, match="pool indices"):
        check_teams([(0, 4)], 4, 2)
    with pytest.raises(ValueError, match="pool indices"):
        check_teams([(-1, 0)], 4, 2)
    with pytest.raises(ValueError, match="no teams"):
        check_teams([], 4, 2)


@pytest.mark.parametrize("n,n_pad", [(1, 128), (127, 128), (128, 128), (129, 256), (1000, 1024), (4096, 4096)])
def test_padded_games(n, n_pad):
    from hanabi_hip.crossplay import padded_games

    assert padded_games(n) == n_pad
    with pytest.raises(ValueError):
        padded_games(0)


@pytest.mark.parametrize("n", [1, 1000, 4096])
@pytest.mark.parametrize("max_rows", [100, 4096, 262144])
def test_chunks_and_block_offsets(n, max_rows):
    from hanabi_hip.crossplay import padded_games, plan_chunks

    n_pad = padded_games(n)
    teams = 64
    plan = plan_chunks(teams, n_pad, max_rows)
    # every team exactly once, in order, chunks within max_rows unless one team alone is larger
    covered = [first + i for first, cnt in plan for i in range(cnt)]
    assert covered == list(range(teams))
    for first, cnt in plan:
        assert cnt >= 1 and (cnt * n_pad <= max_rows or cnt == 1)
    per = max(1, max_rows // n_pad)
    assert len(plan) == -(-teams // per)
    # team k's rows in its chunk: [(k - first) * n_pad, + n) real games, then n_pad - n padding rows, all in whole 128-row tiles
    for first, cnt in plan:
        offs = [(k - first) * n_pad for k in range(first, first + cnt)]
        assert all(o % 128 == 0 for o in offs) and offs == sorted(offs)
        assert offs[-1] + n_pad == cnt * n_pad
    if max_rows < n_pad:
        assert plan == [(k, 1) for k in range(teams)]


def test_crossplay_construction_without_gpu():
    import hanabi_hip
    from hanabi_hip import CrossPlay, CrossPlayResult, EvalResult

    cp = CrossPlay("Hanabi-Full", players=5, n_games=1000, seed=7, first_game_id=3, max_rows=4096, record_actions=True)
    assert (cp.n, cp.n_pad, cp.players, cp.max_turns) == (1000, 1024, 5, hanabi_hip.evaluate.max_turns(hanabi_hip.make_config("Hanabi-Full", 5)))
    assert cp._deals is None and not cp._chunks   # nothing touches the device before run()
    assert cp.chunks(16) == [(0, 4), (4, 4), (8, 4), (12, 4)]
    with pytest.raises(ValueError):
        CrossPlay(n_games=0)
    with pytest.raises(ValueError):
        CrossPlay(max_rows=0)
    with pytest.raises(ValueError):
        CrossPlay(config=hanabi_hip.HbConfig(6, 5, 5, 5, 8, 3, 0))
    # the result's matrices from the default team order
    k = 3
    teams = [(i, j) for i in range(k) for j in range(k)]
    res = [EvalResult([i * 3 + j, i * 3 + j + 2], [10, 12], 25) for i, j in teams]
    r = CrossPlayResult(teams, res, k, 2, default=True)
    m = r.mean_matrix()
    assert m.shape == (3, 3) and m[1, 2].item() == 6.0 and m[2, 0].item() == 7.0
    assert r.stderr_matrix()[0, 0].item() == pytest.approx(1.0)
    import json

    d = r.as_dict()
    json.dumps(d)
    assert d["mean_matrix"][1][2] == 6.0 and len(d["results"]) == 9
    with pytest.raises(ValueError):
        CrossPlayResult(teams[:2], res[:2], k, 2, default=False).mean_matrix()


def test_crossplay_rejects_bad_pools_before_the_device():
    from hanabi_hip import CrossPlay

    class NoMoves:
        pass

    cp = CrossPlay("Hanabi-Full", players=2, n_games=8)
    with pytest.raises(TypeError):
        cp.run([NoMoves()])
    with pytest.raises(ValueError):
        cp.run([NoMoves()], teams=[(0, 1)])
    assert cp._deals is None


def test_grouped_entry_points_reject_bad_arguments():
    import hanabi_hip

    L = hanabi_hip.lib()
    one = C.c_void_p(16)
    # hb_actor_fused_act_grouped(tiles, n_rows, obs, legal, obs_len, hidden, A, atoms, q, eps, seed, draw, actions, dtype, stream)
    act = lambda tiles=one, n=256, obs=one, legal=one, obs_len=658, hidden=512, A=20, atoms=51, q=one, acts=one, dt=1: \
        L.hb_actor_fused_act_grouped(tiles, n, obs, legal, obs_len, hidden, A, atoms, q, 0.0, 1, 1, acts, dt, None)
    for kw in (dict(tiles=None), dict(obs=None), dict(legal=None), dict(q=None), dict(acts=None)):
        assert act(**kw) == -1 and b"null" in L.hb_last_error(), kw
    assert act(n=200) == -1 and b"multiple of 128" in L.hb_last_error()
    assert act(n=-128) == -1
    assert act(A=65) == -1 and b"64" in L.hb_last_error()
    assert act(hidden=256) == -1 and b"shape" in L.hb_last_error()
    assert act(atoms=21) == -1
    assert act(dt=3) == -1 and b"dtype" in L.hb_last_error()
    assert act(n=0) == 0   # no rows: nothing to launch

    cfg = hanabi_hip.make_config()
    # hb_rule_act_grouped(cfg, rows, n_blocks, block_rows, first_gid, set_of_block, rules, n_rules, n_sets, seed, draw, actions, fired, s)
    rule = lambda rows=one, nb=2, br=128, sob=one, rules=one, nr=one, ns=1, acts=one, c=C.byref(cfg): \
        L.hb_rule_act_grouped(c, rows, nb, br, 0, sob, rules, nr, ns, 1, 1, acts, None, None)
    for kw in (dict(rows=None), dict(sob=None), dict(rules=None), dict(nr=None), dict(acts=None), dict(c=None)):
        assert rule(**kw) == -1 and b"null" in L.hb_last_error(), kw
    assert rule(ns=0) == -1 and b"n_sets" in L.hb_last_error()
    assert rule(nb=-1) == -1 and rule(nb=70000) == -1
    assert rule(br=-5) == -1
    assert rule(c=C.byref(hanabi_hip.HbConfig(6, 5, 5, 5, 8, 3, 0))) < 0
    assert rule(nb=0) == 0 and rule(br=0) == 0

    # hb_eval_tally_grouped(cfg, n_blocks, block_games, seat, turn, actions, reward, terminal, score, done, final, length, counters, s)
    tally = lambda nb=2, n=4, seat=0, turn=0, ptr=one: \
        L.hb_eval_tally_grouped(C.byref(cfg), nb, n, seat, turn, ptr, one, one, one, one, one, one, one, None)
    assert tally(seat=2) == -1 and b"seat" in L.hb_last_error()
    assert tally(turn=-1) == -1 and tally(turn=40000) == -1
    assert tally(n=-1) == -1 and tally(nb=-1) == -1 and tally(nb=70000) == -1
    assert tally(ptr=None) == -1 and b"null" in L.hb_last_error()
    assert tally(nb=0) == 0 and tally(n=0) == 0


def test_grouped_tally_without_device():
    import torch

    import hanabi_hip

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    cfg = hanabi_hip.make_config()
    one = C.c_void_p(16)
    assert hanabi_hip.lib().hb_eval_tally_grouped(C.byref(cfg), 2, 4, 0, 0, one, one, one, one, one, one, one, one, None) == -2


def test_new_symbols_exported_and_bound():
    import hanabi_hip
    from hanabi_hip import _capi

    L = hanabi_hip.lib()
    for name in ("hb_actor_fused_act_grouped", "hb_rule_act_grouped", "hb_eval_tally_grouped"):
        assert name in _capi.SIGNATURES and getattr(L, name).argtypes == _capi.SIGNATURES[name][1]
    assert "CrossPlay" in hanabi_hip.__all__ and "CrossPlayResult" in hanabi_hip.__all__
    # hb_fused_tile: five pointers, the int64 game id, active, pad
    assert C.sizeof(_capi.HbFusedTile) == 5 * 8 + 8 + 4 + 4
    assert _capi.HbFusedTile.first_game_id.offset == 40 and _capi.HbFusedTile.active.offset == 48
    from hanabi_agents.rlax_dqn import DQNAgent

    assert callable(DQNAgent.eval_operands)
