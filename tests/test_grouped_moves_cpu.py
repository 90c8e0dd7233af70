"""The move table cross-play and the partner pool share (hanabi_hip.grouped), on the host: agent classification, the tile
descriptors and rule tables of both callers' layouts field by field, and EvalResult.from_counters. Operand dicts are fakes with
integer "addresses"; nothing touches a device."""
import pytest

OBS_LEN, N_ACTIONS = 658, 20


class _Tile:
    """An agent of vectorised observations whose eval_operands() is the given dict (None: off the one-kernel actor)."""

    def __init__(self, ops):
        self.ops, self.asked = ops, 0

    def requires_vectorized_observation(self):
        return True

    def eval_operands(self):
        self.asked += 1
        return self.ops


def _ops(tag, dtype, first_game_id=0, obs_len=OBS_LEN, n_actions=N_ACTIONS):
    return dict(w1f=tag + 1, b1f=tag + 2, w2f=tag + 3, b2f=tag + 4, support=tag + 5, support_t=f"support of {tag}", dtype=dtype,
                obs_len=obs_len, hidden=512, n_actions=n_actions, n_atoms=51, first_game_id=first_game_id)


def _rule(name):
    from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR

    return RulebasedAgent(getattr(PR, f"{name}_rules"))


def _fields(d):
    return (d.w1f, d.b1f, d.w2f, d.b2f, d.support, d.first_game_id, d.active)


def _held(o, gid):
    return (o["w1f"], o["b1f"], o["w2f"], o["b2f"], o["support"], gid, 1)


EMPTY = (None, None, None, None, None, 0, 0)


def test_crossplay_layout():
    """Two blocks of 3 tiles, seat agents [tile agent of dtype 1, rule agent]: block 0's descriptors carry the operands and
    the agent's own game ids, block 1's stay all-zero; block 1 walks rule set 0."""
    from hanabi_hip.grouped import TILE, MoveTable, RuleSets, classify

    base = 4096
    dqn, piers = _Tile(_ops(1000, 1, first_game_id=base)), _rule("piers")
    kinds = [classify(a, OBS_LEN, N_ACTIONS) for a in (dqn, piers)]
    assert kinds[0] == ("tile", dqn.ops) and kinds[1] == ("rule", piers)
    tab = MoveTable(6, (2, 3 * TILE, 0), RuleSets([piers]))
    tab.set_tiles([(0, 3, kinds[0][1], kinds[0][1]["first_game_id"])])
    tab.walk(1, piers)
    assert tab.geometry == (2, 384, 0)
    assert [key for key, _ in tab.groups] == [(1, 512, 51)]
    (_, tiles), = tab.groups
    assert len(tiles) == 6
    assert [_fields(d) for d in tiles[:3]] == [_held(dqn.ops, base + g) for g in (0, 128, 256)]
    assert [_fields(d) for d in tiles[3:]] == [EMPTY] * 3
    assert tab.set_of_block == [-1, 0]
    assert tab.generic == [] and tab.keep == ["support of 1000"]
    assert tab.groups_dev is None and tab.sets_dev is None   # host objects until upload()


def test_pool_layout():
    """Five tiles, members [rule, tile dtype 1, tile dtype 2] with 2 / 2 / 1 tiles: a group per dtype in sorted key order, each
    active on its member's tiles only and keyed by the env's global game ids; the rule member walks blocks 0 and 1."""
    from hanabi_hip.grouped import TILE, MoveTable, RuleSets, classify

    env_first = 1000
    members = [_rule("iggi"), _Tile(_ops(2000, 1)), _Tile(_ops(3000, 2))]
    layout = [(0, 2), (2, 2), (4, 1)]
    kinds = [classify(m, OBS_LEN, N_ACTIONS, prefix=f"member {k}: ") for k, m in enumerate(members)]
    tab = MoveTable(5, (5, TILE, TILE), RuleSets(members[:1]))
    for b in range(2):
        tab.walk(b, members[0])
    # (handed over in reverse: the groups come out in key order, not in member order)
    tab.set_tiles([(first, count, o, env_first + TILE * first) for (first, count), (kind, o) in reversed(list(zip(layout, kinds)))
                   if kind == "tile"])
    assert tab.geometry == (5, 128, 128)
    assert [key for key, _ in tab.groups] == [(1, 512, 51), (2, 512, 51)]
    (_, bf16), (_, f16) = tab.groups
    assert [_fields(d) for d in bf16] == [EMPTY, EMPTY, _held(members[1].ops, env_first + 256), _held(members[1].ops, env_first + 384), EMPTY]
    assert [_fields(d) for d in f16] == [EMPTY] * 4 + [_held(members[2].ops, env_first + 512)]
    assert tab.set_of_block == [0, 0, -1, -1, -1]
    assert sorted(tab.keep) == ["support of 2000", "support of 3000"]
    # a refill replaces every earlier descriptor (the pool: a member's operand addresses changed)
    tab.set_tiles([(2, 2, members[1].ops, env_first + 256)])
    assert [key for key, _ in tab.groups] == [(1, 512, 51)] and tab.set_of_block == [0, 0, -1, -1, -1]
    with pytest.raises(ValueError, match="id_stride"):
        MoveTable(5, (5, TILE, 64), RuleSets([]))


def test_rule_table():
    from hanabi_hip import _capi as K
    from hanabi_hip.grouped import RuleSets

    agents = [_rule(x) for x in ("piers", "flawed", "outer")]
    rs = RuleSets(agents)
    assert len(rs) == 3 and len(rs.table) == 3 * K.MAX_RULES
    assert rs.n_rules == [len(a.rules) for a in agents] and len(set(rs.n_rules)) > 1
    for s, a in enumerate(agents):
        assert rs.index(a) == s
        for q in range(K.MAX_RULES):
            got = rs.table[s * K.MAX_RULES + q]
            want = a._tab[q] if q < len(a.rules) else K.HbRule()
            assert (got.kind, got.arg, got.threshold) == (want.kind, want.arg, want.threshold), (s, q)
    assert rs.table_dev is None and rs.n_rules_dev is None


def test_classification_and_its_errors():
    from hanabi_hip.grouped import classify

    off = _Tile(None)
    assert classify(off, OBS_LEN, N_ACTIONS) == ("generic", None) and off.asked == 1
    on = _Tile(_ops(1, 1))
    assert classify(on, OBS_LEN, N_ACTIONS, fused=False) == ("generic", None) and on.asked == 0   # (operands not even asked for)

    class NoOperands:
        def requires_vectorized_observation(self):
            return True

    assert classify(NoOperands(), OBS_LEN, N_ACTIONS) == ("generic", None)
    with pytest.raises(ValueError, match=r"^agent of obs_len 100 / 20 actions in a game of 658 / 20$"):
        classify(_Tile(_ops(1, 1, obs_len=100)), OBS_LEN, N_ACTIONS)
    with pytest.raises(ValueError, match=r"^member 3: agent of obs_len 658 / 11 actions in a game of 658 / 20$"):
        classify(_Tile(_ops(1, 1, n_actions=11)), OBS_LEN, N_ACTIONS, prefix="member 3: ")

    class Scalar:
        def requires_vectorized_observation(self):
            return False

    with pytest.raises(TypeError, match="vectorised observations"):
        classify(Scalar(), OBS_LEN, N_ACTIONS)


@pytest.mark.parametrize("P", [2, 3])
def test_eval_result_from_counters(P):
    """A hand-made hb_eval_tally counter row against the explicit slices of its layout (include/hanabi_hip.h)."""
    import torch

    from hanabi_hip import EvalResult

    max_score, B = 25, 26
    row = torch.arange(100, 100 + 2 + B + 5 * P, dtype=torch.int64)
    scores, lengths = [3, 0, 25], [40, 12, 61]
    got = EvalResult.from_counters(scores, lengths, max_score, row, P, turns=64)
    want = EvalResult(scores, lengths, max_score, histogram=row[1:1 + B], bombouts=int(row[1 + B]),
                      moves=row[2 + B:2 + B + 4 * P].view(P, 4), misplays=row[2 + B + 4 * P:2 + B + 5 * P], turns=64)
    assert got.histogram.tolist() == list(range(101, 101 + B)) and got.bombouts == 101 + B
    assert got.moves.shape == (P, 4) and got.moves[0].tolist() == list(range(102 + B, 106 + B))
    assert got.misplays.tolist() == list(range(102 + B + 4 * P, 102 + B + 5 * P))
    for name in ("scores", "lengths", "histogram", "moves", "misplays"):
        assert torch.equal(getattr(got, name), getattr(want, name)), name
    assert (got.bombouts, got.turns, got.max_score) == (want.bombouts, want.turns, want.max_score)
    # a longer row (the playout's counters with its two tail words) reads the same
    longer = EvalResult.from_counters(scores, lengths, max_score, torch.cat([row, torch.tensor([7, 9])]), P, turns=64)
    assert torch.equal(longer.moves, want.moves) and torch.equal(longer.misplays, want.misplays)
