"""hb_rule_playout without a GPU: where the entry point is declared, its argument checks, `playout_supported`, the wrappers'
shape and dtype errors, and the CPU expectation (tests/playout_util.py) against itself."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import playout_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rule_team(P=2):
    from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR

    return [RulebasedAgent(PR.piers_rules, seed=11 + p) for p in range(P)]


def test_entry_point_is_exported_and_declared_in_its_own_header():
    import hanabi_hip
    from hanabi_hip import _capi

    assert hasattr(hanabi_hip.lib(), "hb_rule_playout")
    own = open(os.path.join(ROOT, "include", "hanabi_hip_playout.h")).read()
    assert re.search(r"\bint\s+hb_rule_playout\s*\(", own) and '#include "hanabi_hip.h"' in own
    main = open(os.path.join(ROOT, "include", "hanabi_hip.h")).read()
    assert "hb_rule_playout" not in main
    assert "hb_rule_playout" not in _capi.SIGNATURES
    assert hanabi_hip.lib().hb_abi_version() == 1
    for name in ("rule_playout", "playout_supported"):
        assert name in hanabi_hip.__all__ and callable(getattr(hanabi_hip, name))


def test_argument_validation_needs_no_gpu():
    import torch

    import hanabi_hip
    from hanabi_hip import _capi as K, evaluate, playout

    L, f = hanabi_hip.lib(), playout._fn()
    cfg = hanabi_hip.make_config()
    bound = evaluate.max_turns(cfg)
    assert bound == 95
    one = C.c_void_p(16)   # a non-null, 16-byte aligned fake pointer: validation must reject the call before using it
    tab = (K.HbRule * 16)()
    tab[0].kind = K.RULE_PLAY_SAFE_CARD

    def call(rows=one, n=4, tabs=(tab, tab), lens=(1, 1), first_seat=0, max_turns=bound, counters=one):
        rules = (C.POINTER(K.HbRule) * 2)(*[C.cast(t, C.POINTER(K.HbRule)) for t in tabs])
        n_rules = (C.c_int32 * 2)(*lens)
        return f(C.byref(cfg), rows, n, 0, rules, n_rules, 1, first_seat, None, max_turns, one, one, one, counters, None, one, one, None)

    assert call(rows=None) == -1 and b"rows" in L.hb_last_error()
    assert call(counters=None) == -1 and b"counters" in L.hb_last_error()
    bad = (K.HbRule * 16)()
    bad[0].kind = 99
    assert call(tabs=(tab, bad)) == -1 and b"unknown kind 99" in L.hb_last_error()
    assert call(lens=(17, 1)) == -1 and b"n_rules" in L.hb_last_error()
    for seat in (-1, 2):
        assert call(first_seat=seat) == -1 and b"first_seat" in L.hb_last_error()
    assert call(max_turns=0) == -1 and b"max_turns" in L.hb_last_error()
    assert call(max_turns=bound + 1) == -1 and b"max_turns" in L.hb_last_error()
    assert call(rows=C.c_void_p(8)) == -4 and b"aligned" in L.hb_last_error()
    assert call(n=-1) == -1
    assert call(n=0) == 0                                   # no games: a no-op
    if not torch.cuda.is_available():
        assert call() == -2 and b"no HIP device" in L.hb_last_error()   # a valid call: HB_ERR_NO_DEVICE, nothing computed


def test_playout_supported():
    from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR
    from hanabi_hip import PartnerPool, SearchPlayer, playout_supported

    team = _rule_team()
    assert playout_supported(team) is True
    assert playout_supported(_rule_team(5)) is True
    assert playout_supported([RulebasedAgent([]), RulebasedAgent(PR.flawed_rules)]) is True

    class Dqn:   # a seat that is asked for its moves turn by turn, on observations
        def eval_moves(self, *a, **k):
            raise AssertionError

        def requires_vectorized_observation(self):
            return True

    assert playout_supported([team[0], Dqn()]) is False
    assert playout_supported([SearchPlayer(team, 0), team[1]]) is False
    assert playout_supported([team[0], PartnerPool([team[1]])]) is False
    assert playout_supported([]) is False
    for opt in (dict(responses=True), dict(color_shuffle=True), dict(horizon=4), dict(something_else=True)):
        assert playout_supported(team, **opt) is False, opt
    assert playout_supported(team, responses=False, color_shuffle=False, horizon=None) is True


def test_switches_construct_without_a_gpu_and_wrappers_check_their_tensors():
    import torch

    import hanabi_hip
    from hanabi_hip import Evaluator, RolloutSearch, SearchPlayer, rule_playout

    team = _rule_team()
    ev = Evaluator(n_games=8, playout=True)
    assert ev.playout is True and ev.last_path is None and Evaluator(n_games=8).playout is False
    rs = RolloutSearch(replicas=4, playout=True)
    assert rs.playout is True and RolloutSearch(replicas=4).playout is False
    assert SearchPlayer(team, 0, playout=True).playout is True
    for cls, kw in ((Evaluator, dict(n_games=8)), (RolloutSearch, {})):
        with pytest.raises(TypeError):
            cls(playout=1, **kw)

    cfg = hanabi_hip.make_config()
    rows = torch.zeros((4, 32), dtype=torch.int32)
    with pytest.raises(ValueError, match="rows"):
        rule_playout(cfg, torch.zeros((4, 31), dtype=torch.int32), team, 1)
    with pytest.raises(ValueError, match="rows"):
        rule_playout(cfg, rows.long(), team, 1)
    with pytest.raises(ValueError, match="one agent per seat"):
        rule_playout(cfg, rows, team[:1], 1)
    with pytest.raises(TypeError, match="RulebasedAgent"):
        rule_playout(cfg, rows, [team[0], object()], 1)
    with pytest.raises(ValueError, match="max_turns"):
        rule_playout(cfg, rows, team, 1, max_turns=96)
    with pytest.raises(ValueError, match="first_seat"):
        rule_playout(cfg, rows, team, 1, first_seat=2)
    with pytest.raises(ValueError, match="first_moves"):
        rule_playout(cfg, rows, team, 1, first_moves=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="done"):
        rule_playout(cfg, rows, team, 1, done=torch.zeros(4, dtype=torch.int8))
    with pytest.raises(ValueError, match="counters"):
        rule_playout(cfg, rows, team, 1, out=(torch.zeros(4, dtype=torch.int8), torch.zeros(4, dtype=torch.int16),
                                              torch.zeros(3, dtype=torch.int64)))
    with pytest.raises(hanabi_hip.HbError, match="GPU"):   # everything right but the device: there is no CPU path
        rule_playout(cfg, rows, team, 1)


def test_oracle_playout_is_consistent_with_itself():
    e = U.expected("Hanabi-Very-Small", 2, 64, "mixed")   # [Piers, IGGI]
    n, B = 64, e["bins"]
    by_status = np.bincount(e["status"], minlength=4)
    assert by_status.tolist() == [0, 10, 4, 50]            # every ending: out of lives, perfect, out of cards
    assert e["counters"][0] == 0 and e["illegal"] == 0
    assert e["counters"][1:1 + B].sum() == n
    assert e["counters"][1 + B] == (e["status"] == 1).sum()
    assert ((e["done"] & 0x80) != 0).all()
    # length = the turn of the terminal step: the last logged move is at length - 1, and the row counts as many moves
    acts = e["actions"]
    for g in range(n):
        ln = int(e["length"][g])
        assert (acts[:ln, g] >= 0).all() and (acts[ln:, g] == -1).all()
    assert np.array_equal((e["rows"][:, 0] >> 21) & 255, e["length"].astype(np.int64))
    assert np.array_equal(np.bincount(e["final_score"], minlength=B), e["counters"][1:1 + B])
    assert e["counters"][2 + B:2 + B + 8].sum() == e["length"].astype(np.int64).sum()   # one counted move per turn played
    assert e["max_len"] == e["length"].max() <= 95

    c = U.expected("Hanabi-Very-Small", 2, 64, "mixed", max_turns=5)
    longer = e["length"] > 5
    assert 0 < longer.sum() < n
    assert c["counters"][0] == longer.sum()
    assert np.array_equal((c["done"] & 0x80) == 0, longer)
    assert np.array_equal(c["length"][~longer], e["length"][~longer]) and (c["length"][longer] == 0).all()
    assert np.array_equal(c["actions"], e["actions"][:5])


def test_flawed_teams_bomb_out_early():
    for game, P, n in (("Hanabi-Small", 2, 193), ("Hanabi-Full", 2, 63), ("Hanabi-Full", 5, 65)):
        e = U.expected(game, P, n, "flawed")
        assert (e["status"] == 1).sum() + (e["status"] == 2).sum() == n and e["length"].max() <= 22 and e["illegal"] == 0
    assert U.expected("Hanabi-Small", 2, 193, "flawed")["length"].min() == 1
