"""Training against a partner pool (hanabi_hip.partner_pool, csrc/train_tally.hip, hb_rule_act_blocks), the parts that need no
GPU: the tile layout, every construction and seating error, checkpoint validation and the new entry points' argument checks."""
import ctypes as C

import pytest


def _rules(name="piers"):
    from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR

    return RulebasedAgent(getattr(PR, f"{name}_rules"))


def test_layout_largest_remainder_contiguous_deterministic():
    from hanabi_hip.partner_pool import pool_layout

    assert pool_layout(1024, [1, 1, 1]) == [(0, 3), (3, 3), (6, 2)]            # 8 tiles: 2.67 each, ties to the earlier member
    assert pool_layout(4096, [3, 1, 2, 1, 1]) == [(0, 12), (12, 4), (16, 8), (24, 4), (28, 4)]
    assert pool_layout(128 * 10, [0.5, 0.3, 0.2]) == [(0, 5), (5, 3), (8, 2)]
    # 7 tiles over weights 1, 1, 1, 1: quotas 1.75 each -> 2, 2, 2, 1
    assert pool_layout(7 * 128, [1, 1, 1, 1]) == [(0, 2), (2, 2), (4, 2), (6, 1)]
    # 10 tiles, weights 1, 2, 4: quotas 1.43, 2.86, 5.71 -> floors 1, 2, 5 and the remainder to the largest fractions (.86, .71)
    assert pool_layout(1280, [1, 2, 4]) == [(0, 1), (1, 3), (4, 6)]
    for n, w in ((32768, [1] * 6), (4096, [5, 1, 1, 3]), (640, [1, 1, 1, 1, 1])):
        lay = pool_layout(n, w)
        assert lay == pool_layout(n, list(w))   # a pure function of (n, weights)
        assert sum(c for _, c in lay) == n // 128 and all(c > 0 for _, c in lay)
        assert all(lay[k + 1][0] == lay[k][0] + lay[k][1] for k in range(len(lay) - 1)) and lay[0][0] == 0


@pytest.mark.parametrize("n,w,match", [(1000, [1, 1], "multiple of 128"), (0, [1], "multiple of 128"), (256, [1, 1, 1], "only 2 tiles"),
                                       (1024, [1, 100], "no tile")])
def test_layout_errors(n, w, match):
    from hanabi_hip.partner_pool import pool_layout

    with pytest.raises(ValueError, match=match):
        pool_layout(n, w)


def test_construction_errors():
    from hanabi_hip import PartnerPool

    piers = _rules()
    with pytest.raises(ValueError, match="at least one"):
        PartnerPool([])
    with pytest.raises(ValueError, match="neither"):
        PartnerPool([piers, object()])
    with pytest.raises(ValueError, match="twice"):
        PartnerPool([piers, piers])
    with pytest.raises(ValueError, match="weights"):
        PartnerPool([piers], weights=[1, 2])
    with pytest.raises(ValueError, match="positive"):
        PartnerPool([piers, _rules("iggi")], weights=[1, 0])
    pool = PartnerPool([piers])
    with pytest.raises(ValueError, match="another pool"):
        PartnerPool([pool])
    assert pool.layout(256) == [(0, 2)] and pool.seed == 4321 and pool._draws == 0
    assert not pool.requires_vectorized_observation() and not hasattr(pool, "experience")
    assert pool.add_experience_first(None, None) is None and pool.update() is None
    with pytest.raises(ValueError, match="not in a session"):
        pool.stats()


def test_session_seating_errors():
    from hanabi_hip import PartnerPool
    from hanabi_hip.selfplay import check_pool_seats

    piers, iggi, trainee = _rules(), _rules("iggi"), object()
    pool = PartnerPool([piers, iggi])
    assert check_pool_seats([trainee, piers], {0}) is None
    assert check_pool_seats([trainee, pool], {0}) is pool
    assert check_pool_seats([trainee, pool, pool], {0}) is pool   # one pool, several seats
    with pytest.raises(ValueError, match="train_seats"):
        check_pool_seats([trainee, pool], {0, 1})
    with pytest.raises(ValueError, match="also one of the session's agents"):
        check_pool_seats([iggi, pool], {0})
    with pytest.raises(ValueError, match="at most one partner pool"):
        check_pool_seats([trainee, pool, PartnerPool([_rules("outer")])], {0})


def test_shuffle_mask_of_an_unbound_pool():
    from hanabi_hip import PartnerPool

    pool = PartnerPool([_rules(), _rules("iggi"), _rules("outer")], weights=[1, 1, 2])
    with pytest.raises(ValueError, match="pool_seats"):
        pool.shuffle_mask((0, 1))
    # (an unbound pool's mask stays on the host; a pool of only rule members shuffles only the trainee's seat 0)
    m = pool.shuffle_mask((0, 1), n=1024, pool_seats=(1,))
    assert m.shape == (1024,) and m.tolist() == [1] * 1024


def test_checkpoint_validation():
    from hanabi_hip import PartnerPool

    pool = PartnerPool([_rules(), _rules("iggi")], weights=[1, 3])
    with pytest.raises(ValueError, match="not a partner-pool"):
        pool.load_checkpoint_state({"format": "hanabi-agents_amd/rule_agent/1"})
    with pytest.raises(ValueError, match="not a partner-pool"):
        pool.load_checkpoint_state(None)
    good = dict(format="hanabi-agents_amd/partner_pool/1", n=1024, tiles=[[0, 2], [2, 6]], weights=[1.0, 3.0], seed=1, draws=3,
                members=[("rule", [(r.kind, r.arg, float(r.threshold)) for r in m.rules]) for m in pool.members])
    pool.load_checkpoint_state(dict(good))   # an unbound pool keeps it for its session
    assert pool._restore is not None
    other = PartnerPool([_rules(), _rules("outer")], weights=[1, 3])
    with pytest.raises(ValueError, match="different members"):
        other.load_checkpoint_state(dict(good))
    with pytest.raises(ValueError, match="layout"):
        PartnerPool([_rules(), _rules("iggi")]).load_checkpoint_state(dict(good))


def test_new_entry_points_exported_and_reject_bad_arguments():
    import torch

    import hanabi_hip
    from hanabi_hip import _capi

    L = hanabi_hip.lib()
    for name in ("hb_rule_act_blocks", "hb_train_counters", "hb_train_tally_init", "hb_train_tally"):
        assert hasattr(L, name) and name in _capi.SIGNATURES
    assert L.hb_abi_version() == 1
    cfg = hanabi_hip.make_config("Hanabi-Full", 2)
    assert L.hb_train_counters(C.byref(cfg)) == 6 + 26 + 10
    assert L.hb_train_counters(C.byref(hanabi_hip.make_config("Hanabi-Small", 5))) == 6 + 11 + 25
    assert L.hb_train_counters(None) == -1
    one = C.c_void_p(16)
    # hb_rule_act_blocks(cfg, rows, n_blocks, block_rows, first_gid, set_of_block, rules, n_rules, n_sets, seed, draw, actions, fired, s)
    rule = lambda rows=one, nb=2, br=128, sob=one, rules=one, nr=one, ns=1, acts=one, c=C.byref(cfg): \
        L.hb_rule_act_blocks(c, rows, nb, br, 0, sob, rules, nr, ns, 1, 1, acts, None, None)
    for kw in (dict(rows=None), dict(sob=None), dict(rules=None), dict(nr=None), dict(acts=None), dict(c=None)):
        assert rule(**kw) == -1 and b"null" in L.hb_last_error(), kw
    assert rule(ns=0) == -1 and b"n_sets" in L.hb_last_error()
    assert rule(nb=-1) == -1 and rule(nb=70000) == -1 and rule(br=-5) == -1
    assert rule(c=C.byref(hanabi_hip.HbConfig(6, 5, 5, 5, 8, 3, 0))) < 0
    assert rule(nb=0) == 0 and rule(br=0) == 0
    # hb_train_tally(cfg, n, seat, actions, reward, terminal, score, tile_member, n_members, lost, length, counters, s)
    tally = lambda n=256, seat=0, members=2, ptr=one: \
        L.hb_train_tally(C.byref(cfg), n, seat, ptr, one, one, one, one, members, one, one, one, None)
    assert tally(n=200) == -1 and b"multiple of 128" in L.hb_last_error()
    assert tally(n=-128) == -1
    assert tally(seat=2) == -1 and b"seat" in L.hb_last_error()
    assert tally(members=0) == -1 and tally(members=65) == -1 and b"n_members" in L.hb_last_error()
    assert tally(ptr=None) == -1 and b"null" in L.hb_last_error()
    assert tally(n=0) == 0
    assert L.hb_train_tally_init(C.byref(cfg), None, 128, one, one, None) == -1
    assert L.hb_train_tally_init(C.byref(cfg), one, -1, one, one, None) == -1
    assert L.hb_train_tally_init(C.byref(cfg), one, 0, one, one, None) == 0
    if not torch.cuda.is_available():   # arguments are checked first, then the device
        assert tally() == -2 and L.hb_train_tally_init(C.byref(cfg), one, 128, one, one, None) == -2
