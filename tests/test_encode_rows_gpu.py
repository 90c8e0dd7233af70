"""hb_encode_rows on the GPU (csrc/encode_rows.hip, hanabi_hip.encode; DESIGN.md section 4, "The stateless encoder"):

* the kernel against `encode_rows_ref` bit for bit on rows of the oracle-driven deep play (fresh deals, mid-game, empty decks,
  re-dealt games, every seat to act), every output form, guard words around every buffer, the rows untouched;
* the kernel against the env it replaces, with no numpy in between: import_state + observe on a HanabiEnv;
* the slabs of a [K, m, SW] buffer in one call;
* ConditionedDeterminizer and OffBeliefSession with stateless on and off: the same bits, and no import into the scratch env.
"""
import functools
import json
import os

import numpy as np
import pytest

import deep_play as D
import encode_rows_util as U
from search_util import _conditioned_games, _dqn, _mid_game_env, _u32

pytestmark = pytest.mark.gpu

GUARD = 64                       # sentinel elements before and after every buffer (a multiple of 16 bytes for every dtype used)
SIZES = (1, 7, 8, 9, 63, 64, 65, 257)


def _guarded(shape, dtype, fill):
    import torch

    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(shape)


def _cuda(rows_np):
    """uint32 rows (possibly read only) -> an int32 tensor on the GPU."""
    import torch

    return torch.as_tensor(np.array(np.asarray(rows_np).view(np.int32))).cuda()


def _guards_intact(buf, fill):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all())


@functools.lru_cache(maxsize=None)
def _reference(game, players, n, seat):
    """(rows uint32 [n, SW], obs int8, packed obs uint32, legal int8) of the numpy reference: computed once, read only."""
    import hanabi_hip

    cfg = hanabi_hip.make_config(game, players, D.FLAGS)
    rows = U.mixed_rows(game, players, n)
    obs, legal = hanabi_hip.encode_rows_ref(cfg, rows, seat=seat)
    bits = U.pack_bits(obs)
    for a in (obs, bits, legal):
        a.setflags(write=False)
    return rows, obs, bits, legal


def _check_all_forms(game, players, n, seat):
    import torch

    import hanabi_hip
    from hanabi_hip import _capi as K
    import ctypes as C

    cfg = hanabi_hip.make_config(game, players, D.FLAGS)
    rows_np, want_obs, want_bits, want_legal = _reference(game, players, n, seat)
    L = hanabi_hip.lib()
    NW, OL, A = want_bits.shape[1], want_obs.shape[1], want_legal.shape[1]
    assert (NW, OL, A) == (L.hb_obs_words(C.byref(cfg)), L.hb_obs_len(C.byref(cfg)), L.hb_num_actions(C.byref(cfg)))
    rbuf, rows = _guarded(rows_np.shape, torch.int32, 0x5A5A5A5A)
    rows.copy_(_cuda(rows_np))
    s = -1 if seat is None else seat
    # (packed, int8, legal): packed only, int8 only, both, and each without the legal mask
    for use_bits, use_obs, use_legal in ((1, 0, 1), (0, 1, 1), (1, 1, 1), (1, 0, 0), (0, 1, 0)):
        bbuf, bits = _guarded((n, NW), torch.int32, -0x21524111)
        obuf, obs = _guarded((n, OL), torch.int8, 0x77)
        lbuf, legal = _guarded((n, A), torch.int8, 0x77)
        K.check(L.hb_encode_rows(C.byref(cfg), K.dptr(rows), n, s, K.dptr(bits) if use_bits else None, K.dptr(obs) if use_obs else None,
                                 K.dptr(legal) if use_legal else None, K.current_stream()))
        torch.cuda.synchronize()
        form = (use_bits, use_obs, use_legal)
        if use_bits:
            got = _u32(bits)
            assert np.array_equal(got, want_bits), form
            if OL % 32:
                assert not (got[:, -1] >> np.uint32(OL % 32)).any(), "pad bits of the last packed word"
        else:
            assert bool((bits == -0x21524111).all()), form
        if use_obs:
            assert np.array_equal(obs.cpu().numpy(), want_obs), form
        else:
            assert bool((obs == 0x77).all()), form
        if use_legal:
            assert np.array_equal(legal.cpu().numpy(), want_legal), form
        else:
            assert bool((legal == 0x77).all()), form
        assert _guards_intact(bbuf, -0x21524111) and _guards_intact(obuf, 0x77) and _guards_intact(lbuf, 0x77), form
    assert np.array_equal(_u32(rows), rows_np) and _guards_intact(rbuf, 0x5A5A5A5A), "the rows were written"
    # and through the Python wrapper, both forms
    for int8, want in ((False, want_bits), (True, want_obs)):
        obs, legal = hanabi_hip.encode_rows(cfg, rows, seat=seat, int8=int8)
        assert obs.dtype == (torch.int8 if int8 else torch.int32) and legal.dtype == torch.int8
        assert np.array_equal(_u32(obs) if not int8 else obs.cpu().numpy(), want) and np.array_equal(legal.cpu().numpy(), want_legal)


@pytest.mark.parametrize("game,players", D.VARIANTS)
def test_kernel_equals_the_reference_on_every_variant(game, players):
    _check_all_forms(game, players, D.N_GAMES, None)
    _check_all_forms(game, players, D.N_GAMES, players - 1)


@pytest.mark.parametrize("players", [2, 5])
@pytest.mark.parametrize("n", SIZES)
def test_kernel_equals_the_reference_at_every_size(players, n):
    """Full 2p: 32-word rows, 21 observation words, 20 actions. Full 5p: 48-word rows, 40 words, 48 actions (the legal bits
    cross into the second word). One row, a partial wave, exactly 16 / 64 rows and one more, more than one workgroup."""
    _check_all_forms("Hanabi-Full", players, n, None)
    _check_all_forms("Hanabi-Full", players, n, 0)


def test_large_batch_takes_the_wide_kernel():
    """32 768 rows and more with packed output alone run 32 rows per wavefront: the same bits."""
    import torch

    import hanabi_hip

    cfg = hanabi_hip.make_config("Hanabi-Full", 2, D.FLAGS)
    rows_np, _, want_bits, want_legal = _reference("Hanabi-Full", 2, 257, None)
    n = 32768 + 257
    idx = np.arange(n) % 257
    rows = _cuda(rows_np[idx])
    obs, legal = hanabi_hip.encode_rows(cfg, rows)
    assert np.array_equal(_u32(obs), want_bits[idx]) and np.array_equal(legal.cpu().numpy(), want_legal[idx])


def test_wrapper_checks_out_buffers():
    import torch

    import hanabi_hip

    cfg = hanabi_hip.make_config()
    rows = _cuda(_reference("Hanabi-Full", 2, 9, None)[0])
    good = (torch.empty((9, 21), dtype=torch.int32, device="cuda"), torch.empty((9, 20), dtype=torch.int8, device="cuda"))
    o, l = hanabi_hip.encode_rows(cfg, rows, out=good)
    assert o is good[0] and l is good[1]
    for bad in ((good[0][:8], good[1]), (good[0].to(torch.int64), good[1]), (good[0], good[1].cpu()),
                (torch.empty((9, 42), dtype=torch.int32, device="cuda")[:, ::2], good[1]), (good[0], good[1].to(torch.uint8))):
        with pytest.raises(ValueError):
            hanabi_hip.encode_rows(cfg, rows, out=bad)
    o, l = hanabi_hip.encode_rows(cfg, rows[:0])                 # no rows: empty outputs, no error
    assert o.shape == (0, 21) and o.dtype == torch.int32 and l.shape == (0, 20) and l.dtype == torch.int8
    assert hanabi_hip.encode_rows(cfg, rows[:0], int8=True)[0].shape == (0, 658)
    with pytest.raises(ValueError):
        hanabi_hip.encode_rows(cfg, rows[:, :31])
    with pytest.raises(ValueError):
        hanabi_hip.encode_rows(cfg, rows.long())
    with pytest.raises(hanabi_hip.HbError):
        hanabi_hip.encode_rows(cfg, rows.cpu())


# ---- against the env it replaces -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("game,players", [("Hanabi-Full", 2), ("Hanabi-Small", 2), ("Hanabi-Full", 3), ("Hanabi-Full", 5)])
def test_kernel_equals_import_and_observe(game, players):
    import torch

    import hanabi_hip

    cfg = hanabi_hip.make_config(game, players, D.FLAGS)
    deep = _cuda(U.mixed_rows(game, players, D.N_GAMES))
    # an env without auto-reset, played on until some games are over: finished rows
    ended = _mid_game_env(game, players, D.N_GAMES, 40)
    done = ((ended.export_state()[:, 0] >> 19) & 3) != 0
    assert bool(done.any())
    for rows in (deep, ended.export_state()):
        n = rows.shape[0]
        packed = hanabi_hip.HanabiEnv(game, players, n_games=n, seed=3, packed=True)
        plain = hanabi_hip.HanabiEnv(game, players, n_games=n, seed=3, packed=False)
        for seat in [None] + list(range(players)):
            src = rows if seat is None else _cuda(U.with_seat(_u32(rows), seat))
            packed.import_state(src)
            want_bits, want_legal = packed.observe()
            plain.import_state(src)
            want_obs, _ = plain.observe()
            bits, legal = hanabi_hip.encode_rows(cfg, rows, seat=seat)
            obs, legal8 = hanabi_hip.encode_rows(cfg, rows, seat=seat, int8=True)
            assert torch.equal(bits, want_bits) and torch.equal(obs, want_obs) and torch.equal(legal, legal8), seat
            if seat is None:
                assert torch.equal(legal, want_legal)
            else:   # the env's mask is the rewritten row's; the encoder's is the real row's, for its real seat to act only
                mine = ((rows[:, 0] >> 13) & 7) == seat
                assert torch.equal(legal[mine], want_legal[mine]) and not bool(legal[~mine].any()), seat


def test_slabs_in_one_call():
    import torch

    import hanabi_hip

    cfg = hanabi_hip.make_config("Hanabi-Full", 3, D.FLAGS)
    rows = _cuda(U.mixed_rows("Hanabi-Full", 3, 3 * 65)).view(3, 65, -1)
    obs, legal = hanabi_hip.encode_rows(cfg, rows.view(3 * 65, -1))
    obs8, _ = hanabi_hip.encode_rows(cfg, rows.view(3 * 65, -1), int8=True)
    for k in range(3):
        o, l = hanabi_hip.encode_rows(cfg, rows[k])
        o8, _ = hanabi_hip.encode_rows(cfg, rows[k], int8=True)
        assert torch.equal(obs.view(3, 65, -1)[k], o) and torch.equal(legal.view(3, 65, -1)[k], l)
        assert torch.equal(obs8.view(3, 65, -1)[k], o8)


# ---- ConditionedDeterminizer -------------------------------------------------------------------------------------------------------------
def _game(team, m, turns, seat, depth, seed=7):
    """m games of `team` on Full 2p, turn by turn as Evaluator.run keys it, seat `seat` keeping a PartnerHistory as SearchPlayer
    does. -> (env, history, rows, the state the partner last moved from)."""
    import torch

    import hanabi_hip
    from hanabi_hip import PartnerHistory, last_move_uid

    env = hanabi_hip.HanabiEnv("Hanabi-Full", 2, n_games=m, seed=seed, auto_reset=False, packed=True)
    hist = PartnerHistory(env.cfg, m, depth, "cuda", partner_seed=seed, first_game_id=0)
    act = torch.empty(m, dtype=torch.int32, device="cuda")
    states, mine, scratch = [env.export_state()], None, [{}, {}]
    for t in range(turns + 1):
        rows = states[-1]
        if t % 2 == seat and t >= 1:
            if mine is not None:
                hist.own_move(mine)
            hist.push(states[-2], last_move_uid(env.cfg, rows), t, torch.ones(m, dtype=torch.uint8), seat=seat)
        if t == turns:
            break
        a = team[t % 2]
        if a.requires_vectorized_observation():
            a.eval_moves((env, (env.net_obs, env.legal)), seed, t + 1, act, scratch=scratch[t % 2])
        else:
            a.eval_moves(env, seed, t + 1, act)
        if t % 2 == seat:
            mine = act.clone()
        env.step(act)
        states.append(env.export_state())
    assert turns % 2 == seat
    return env, hist, states[-1], states[-2]


def _both_settings(team, m, expect_stateless, turns=8):
    """sample (replicas 2, oversample 4) and sample_history (depth 2, oversample 4) with stateless on and off -> the two result
    tuples of each; with stateless on, whether the scratch env was left alone."""
    import torch

    from hanabi_hip import ConditionedDeterminizer

    seed, seat, partner = 7, 0, 1
    env, hist, rows, prev = _game(team, m, turns, seat, 2, seed)
    assert bool((((rows[:, 0] >> 19) & 3) == 0).all()) and hist.filled == 2
    out = {}
    for stateless in (True, False):
        cd = ConditionedDeterminizer("Hanabi-Full", 2, stateless=stateless)
        assert cd.stateless is stateless
        cd._setup(m, 8, rows.device)                               # the scratch env exists before the first call
        scratch_env = cd._sized[(m, 8)]["env"]
        before = scratch_env.export_state().clone()
        one = cd.sample(rows, prev, team[partner], seat, 2, 4, seed=5, draw=turns + 1, partner_seed=seed, partner_draw=turns,
                        first_game_id=0, first_row_id=100)
        more = cd.sample_history(rows, hist, team[partner], seat, 2, 4, seed=5, draw=turns + 1, partner_seed=seed, first_game_id=0,
                                 first_row_id=100)
        torch.cuda.synchronize()
        assert cd._sized[(m, 8)]["env"] is scratch_env
        untouched = torch.equal(scratch_env.export_state(), before)
        if stateless:
            assert untouched == expect_stateless, "the scratch env and the stateless path"
        else:
            assert not untouched
        out[stateless] = [t.clone() for t in (one.rows, one.weights, one.n_surv[0], one.fallback,
                                              more.rows, more.weights, more.n_surv, more.depth_used, more.fallback)]
    assert len(out[True]) == 4 + 5
    for a, b in zip(out[True], out[False]):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    n_surv = out[True][2]
    print("n_surv", n_surv.tolist(), "depth_used", out[True][7].tolist())
    return out


@pytest.mark.parametrize("m", [8, 6])
def test_conditioned_determinizer_stateless_equals_the_scratch_env(m):
    """A DQN partner (bf16, bit-packed rows): one encode call over all slabs (m = 8) or, where a slab of m rows is no multiple
    of 16 bytes (m = 6), one per padded slab; no import, no observe: the scratch env's state stays what it was. The game is
    Piers (seat 0, the observer) with the DQN agent in seat 1: four turns in, the untrained agent has moved twice, so no game can
    have lost its three lives, and the history holds both of its moves."""
    from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR

    shape = _mid_game_env("Hanabi-Full", 2, 1, 0)
    team = [RulebasedAgent(PR.piers_rules, seed=11), _dqn(shape, seed=6)]
    assert type(team[1]).obs_only_eval is True
    out = _both_settings(team, m, expect_stateless=True, turns=4)
    assert bool((out[True][2] < 8).any()) or bool((out[True][6] < 8).any())   # the filter rejected something: the moves mattered


def test_conditioned_determinizer_piers_partner_keeps_the_scratch_env():
    """A rule-based partner reads state rows, not observations: no obs_only_eval, both settings take the scratch env."""
    from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR

    team = [RulebasedAgent(PR.piers_rules, seed=11), RulebasedAgent(PR.piers_rules, seed=12)]
    assert not getattr(team[1], "obs_only_eval", False)
    _both_settings(team, 8, expect_stateless=False)


def test_recorded_conditioned_games_with_stateless_off(monkeypatch):
    """search_util._conditioned_games (Piers partners, SearchPlayer(condition=True)) with every ConditionedDeterminizer built
    stateless=False equals the recorded games, which tests/test_search_belief_gpu.py holds the default (True) to."""
    from hanabi_hip import search

    init = search.ConditionedDeterminizer.__init__
    built = []

    def off(self, *a, **kw):
        kw["stateless"] = False
        init(self, *a, **kw)
        built.append(self)

    monkeypatch.setattr(search.ConditionedDeterminizer, "__init__", off)
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "search_belief_lastmove.json")) as f:
        want = json.load(f)
    got = _conditioned_games()
    assert built and not any(cd.stateless for cd in built)
    assert got == want


# ---- OffBeliefSession --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [200, 256])
def test_off_belief_level_2_stateless_equals_the_scratch_env(n):
    """200 games of Small 2p: a slab of 200 legal rows (11 bytes each) is no multiple of 16 bytes, so the slabs are padded apart
    and encoded one call each; 256 games: one call over all slabs."""
    import torch
    from test_obl_level_gpu import _dqn as _obl_dqn

    import hanabi_hip
    from hanabi_hip import OffBeliefSession
    from hanabi_hip.obl import frozen_copy

    steps = 20

    def run(stateless):
        env = hanabi_hip.HanabiEnv("Hanabi-Small", 2, n_games=n, seed=11, packed=True)
        agents = [_obl_dqn(env, seed=s, experience_buffer_size=4096) for s in (1, 2)]
        frozen = [frozen_copy(a) for a in agents]
        sess = OffBeliefSession(env, agents, belief_seed=5, belief_policy=frozen, depth=2, oversample=4)
        assert sess.cdet.stateless is True
        sess.cdet.stateless = stateless
        sess.run(steps)
        torch.cuda.synchronize()
        rings = []
        for a in agents:
            b = a.experience
            rings.append((b.size, b.oldest_entry, [getattr(b, f).clone() for f in ("_obs_tm1_buf", "_act_tm1_buf", "_obs_t_buf", "_lms_t_buf",
                                                                                   "_rew_t_buf", "_terminal_t_buf")]))
        counters = {k: getattr(sess, k) for k in ("env_steps", "grad_steps", "branch_steps", "dead_rows", "belief_forwards") +
                    OffBeliefSession.LEVEL_COUNTERS}
        return rings, counters, env.export_state().clone()

    on, off = run(True), run(False)
    print(on[1])
    assert on[1] == off[1] and on[1]["belief_forwards"] > 0 and on[1]["conditioned_rows"] > 0
    assert torch.equal(on[2], off[2])
    for (size_a, old_a, bufs_a), (size_b, old_b, bufs_b) in zip(on[0], off[0]):
        assert (size_a, old_a) == (size_b, old_b) and size_a == n * steps // 2
        for x, y in zip(bufs_a, bufs_b):
            assert torch.equal(x, y)
