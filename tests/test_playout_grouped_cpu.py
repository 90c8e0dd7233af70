"""hb_rule_playout_grouped without a GPU: where the entry point is declared, its argument checks, the wrapper's shape and dtype
errors, the cross-play support predicate and the switch, and RuleSearch on an injected score."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rule_team(P=2):
    from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR

    return [RulebasedAgent(PR.piers_rules, seed=11 + p) for p in range(P)]


class _Dqn:   # an agent that is asked for its moves turn by turn, on observations
    def eval_moves(self, *a, **k):
        raise AssertionError

    def requires_vectorized_observation(self):
        return True


def test_entry_point_is_exported_and_declared_in_the_playout_header():
    import hanabi_hip
    from hanabi_hip import _capi

    assert hasattr(hanabi_hip.lib(), "hb_rule_playout_grouped")
    own = open(os.path.join(ROOT, "include", "hanabi_hip_playout.h")).read()
    assert re.search(r"\bint\s+hb_rule_playout_grouped\s*\(", own) and re.search(r"\bint\s+hb_rule_playout\s*\(", own)
    main = open(os.path.join(ROOT, "include", "hanabi_hip.h")).read()
    assert "hb_rule_playout_grouped" not in main
    assert "hb_rule_playout_grouped" not in _capi.SIGNATURES
    assert hanabi_hip.lib().hb_abi_version() == 1
    for name in ("rule_playout_grouped", "crossplay_playout_supported", "GroupedPlayoutResult", "RuleSearch"):
        assert name in hanabi_hip.__all__ and getattr(hanabi_hip, name) is not None


def test_argument_validation_needs_no_gpu():
    import torch

    import hanabi_hip
    from hanabi_hip import evaluate, playout

    L, f = hanabi_hip.lib(), playout._fn_grouped()
    cfg = hanabi_hip.make_config()
    bound = evaluate.max_turns(cfg)
    one = C.c_void_p(16)   # a non-null, 16-byte aligned fake pointer: validation must reject the call before using it

    def call(cfg=cfg, rows=one, n_blocks=3, block_games=5, id_stride=0, team=one, rules=one, n_rules=one, n_sets=2, first_seat=0,
             max_turns=bound, done=one, fs=one, ln=one, counters=one, illegal=one, max_len=one):
        return f(C.byref(cfg) if cfg is not None else None, rows, n_blocks, block_games, 0, id_stride, team, rules, n_rules, n_sets, 1,
                 first_seat, None, max_turns, done, fs, ln, counters, None, illegal, max_len, None)

    def rejected(code=-1, word=None, **kw):
        rc = call(**kw)
        msg = L.hb_last_error()
        assert rc == code, (kw, rc, msg)
        for name in ([word] if word else list(kw)):
            assert name.encode() in msg, (kw, msg)

    # hb_rule_playout's checks
    rejected(cfg=None, word="config")
    rejected(cfg=hanabi_hip.HbConfig(2, 5, 5, 3, 8, 3, 0), word="no compiled kernel")
    rejected(rows=None)
    rejected(counters=None)
    rejected(done=None)
    rejected(fs=None, word="final_score")
    rejected(ln=None, word="length")
    rejected(illegal=None)
    rejected(max_len=None)
    for seat in (-1, 2):
        rejected(first_seat=seat)
    rejected(max_turns=0)
    rejected(max_turns=bound + 1)
    rejected(code=-4, rows=C.c_void_p(8), word="aligned")
    # the grouped form's own
    rejected(team=None, word="team_of_block_dev")
    rejected(rules=None, word="rules_dev")
    rejected(n_rules=None, word="n_rules_dev")
    rejected(n_sets=0)
    rejected(n_sets=-3)
    rejected(n_blocks=-1)
    rejected(block_games=0)
    rejected(block_games=-7)
    rejected(id_stride=1)
    rejected(id_stride=-5, block_games=5)
    rejected(n_blocks=2 ** 16, block_games=2 ** 15, word="2^31")             # exactly 2^31 games
    rejected(n_blocks=2 ** 40, block_games=2 ** 40, word="2^31")             # (the product does not fit 64 bits)
    assert call(id_stride=5, n_blocks=0) == 0 and call(n_blocks=0) == 0      # no blocks: a no-op
    assert call(n_blocks=0, rows=None) == -1                                 # ... after the checks
    if not torch.cuda.is_available():
        for stride in (0, 5):   # a valid call: HB_ERR_NO_DEVICE, nothing computed
            assert call(id_stride=stride) == -2 and b"no HIP device" in L.hb_last_error()
        assert call(n_blocks=2 ** 16 - 1, block_games=2 ** 15) == -2           # just below 2^31 games


def test_wrapper_checks_its_arguments():
    import torch

    import hanabi_hip
    from hanabi_hip import rule_playout_grouped

    team = tuple(_rule_team())
    cfg = hanabi_hip.make_config()
    rows = torch.zeros((12, 32), dtype=torch.int32)
    teams = [team, None, team]
    with pytest.raises(ValueError, match="rows"):
        rule_playout_grouped(cfg, torch.zeros((12, 31), dtype=torch.int32), teams, 1, block_games=4)
    with pytest.raises(ValueError, match="rows"):
        rule_playout_grouped(cfg, rows, teams, 1, block_games=5)            # 3 blocks of 5 games are 15 rows
    with pytest.raises(ValueError, match="rows"):
        rule_playout_grouped(cfg, rows.long(), teams, 1, block_games=4)
    with pytest.raises(ValueError, match="block_games"):
        rule_playout_grouped(cfg, rows, teams, 1, block_games=0)
    with pytest.raises(ValueError, match="id_stride"):
        rule_playout_grouped(cfg, rows, teams, 1, block_games=4, id_stride=3)
    with pytest.raises(ValueError, match="block 2: one agent per seat"):
        rule_playout_grouped(cfg, rows, [team, None, team[:1]], 1, block_games=4)
    with pytest.raises(TypeError, match="block 0.*RulebasedAgent"):
        rule_playout_grouped(cfg, rows, [(team[0], _Dqn()), None, team], 1, block_games=4)
    with pytest.raises(ValueError, match="max_turns"):
        rule_playout_grouped(cfg, rows, teams, 1, block_games=4, max_turns=96)
    with pytest.raises(ValueError, match="first_seat"):
        rule_playout_grouped(cfg, rows, teams, 1, block_games=4, first_seat=2)
    with pytest.raises(ValueError, match="first_moves"):
        rule_playout_grouped(cfg, rows, teams, 1, block_games=4, first_moves=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="done"):
        rule_playout_grouped(cfg, rows, teams, 1, block_games=4, done=torch.zeros(12, dtype=torch.int8))
    with pytest.raises(ValueError, match="counters"):   # one counter row per block
        rule_playout_grouped(cfg, rows, teams, 1, block_games=4, out=(torch.zeros(12, dtype=torch.int8), torch.zeros(12, dtype=torch.int16),
                                                                      torch.zeros(47, dtype=torch.int64)))
    with pytest.raises(hanabi_hip.HbError, match="GPU"):   # everything right but the device: there is no CPU path
        rule_playout_grouped(cfg, rows, teams, 1, block_games=4, id_stride=4)


def test_crossplay_support_predicate_and_switch():
    from hanabi_hip import CrossPlay, crossplay_playout_supported as ok
    from hanabi_hip.crossplay import default_teams

    pool = _rule_team(4)
    assert ok(pool, default_teams(4, 2)) is True
    assert ok(pool, [(0, 1, 2), (3, 3, 3)]) is True
    mixed = pool[:2] + [_Dqn()]
    assert ok(mixed, default_teams(3, 2)) is False              # a DQN-style agent in a team that is played
    assert ok(mixed, [(0, 1), (1, 1), (1, 0)]) is True          # the same agent in a pool slot no team uses
    assert ok(mixed, [(0, 1), (2, 0)]) is False
    for opt in (dict(responses=True), dict(color_shuffle=True), dict(something_else=True)):
        assert ok(pool, default_teams(4, 2), **opt) is False, opt
    assert ok(pool, default_teams(4, 2), responses=False, color_shuffle=False) is True
    assert ok(pool, []) is False and ok(pool, [(0, 7)]) is False

    cp = CrossPlay(n_games=8, playout=True)                     # construction needs no GPU
    assert cp.playout is True and cp.last_path is None and CrossPlay(n_games=8).playout is False
    with pytest.raises(TypeError):
        CrossPlay(n_games=8, playout=1)


def _kind_sum(lists):
    return [float(sum(r.kind for r in rules)) for rules in lists]


def test_rule_search_on_an_injected_score():
    from hanabi_agents.rule_based import Ruleset, predefined_rules as PR
    from hanabi_hip import RuleSearch
    from hanabi_hip import _capi as K
    from hanabi_hip.rule_search import MUTATIONS, default_catalogue

    seen = []

    def score(lists):
        seen.extend(lists)
        return _kind_sum(lists)

    def search():
        return RuleSearch("Hanabi-Small", 2, n_games=64, seed=1, population=24, elite=4, score=score)

    first = [PR.piers_rules, [Ruleset.legal_random]]
    rs = search()
    a = rs.run(first, generations=12, rng_seed=5)
    assert set(rs.mutation_counts) == set(MUTATIONS) and all(rs.mutation_counts[m] > 0 for m in MUTATIONS)
    assert sum(rs.mutation_counts.values()) == 22 + 12 * 20         # the first fill, then population - elite per generation
    assert len(seen) == 13 * 24 and all(1 <= len(x) <= K.MAX_RULES == 16 for x in seen)
    assert len(a.history) == 13 and all(y >= x for x, y in zip(a.history, a.history[1:]))   # the elite survive
    assert a.history[-1] > a.history[0] >= _kind_sum([PR.piers_rules])[0]
    assert a.mean == a.history[-1] == _kind_sum([a.best])[0] == max(_kind_sum(seen[-24:])) and a.best in seen[-24:]
    b = search().run(first, generations=12, rng_seed=5)              # the same rng_seed: the same run
    assert b == a
    n_seen = len(seen)
    search().run(first, generations=12, rng_seed=6)
    assert seen[n_seen:] != seen[:13 * 24]                          # another rng_seed: other mutants
    # lengths stay in 1..16 at both ends: a score that rewards long lists, and one that rewards short ones
    for sign in (1, -1):
        lengths = []

        def by_length(ls, s=sign):
            lengths.extend(len(x) for x in ls)
            return [s * len(x) for x in ls]

        r = RuleSearch("Hanabi-Small", 2, 64, 1, population=16, elite=2, score=by_length)
        out = r.run([[Ruleset.play_safe_card] * 8], generations=40, rng_seed=1)
        assert len(out.best) == (16 if sign > 0 else 1) and min(lengths) >= 1 and max(lengths) <= 16
        assert lengths.count(16 if sign > 0 else 1) > 100            # many mutants of a list at the bound: none leaves it
    assert len(default_catalogue()) > 16 and all(0 <= r.kind < 16 for r in default_catalogue())
    with pytest.raises(ValueError, match="elite"):
        RuleSearch(population=4, elite=5)
    with pytest.raises(ValueError, match="initial"):
        search().run([], 1)
    with pytest.raises(ValueError, match="1..16"):
        search().run([[]], 1)
