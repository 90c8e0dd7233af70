"""The one result and the one-entry history of conditioned sampling, the parts that need no GPU (hanabi_hip.search): `LastMove`
and `_history` refuse what the tuple history was refused for, with the same messages, and present a `PartnerHistory`'s
attributes; `BeliefSample.survivors()` against the gather written out root by root; the numpy restatements are importable from
hanabi_hip.belief_ref and from the package."""
import pytest


def test_last_move_and_history_refuse_the_same_things():
    import torch

    from hanabi_hip import LastMove
    from hanabi_hip.search import _history

    rows = torch.zeros((4, 32), dtype=torch.int32)
    make = lambda prev, *rest: LastMove(prev, 7, 3, 100, *rest, m=4, words=32, device="cpu")
    for bad in (rows, (rows, 7, 3), (rows, 7, 3, 100, None, None), None, "history"):
        with pytest.raises(ValueError, match=r"history is \(prev_rows, partner_seed, partner_draw, first_game_id\[, valid\]\)"):
            _history(bad, 4, 32, "cpu")
    for bad_rows, shape in ((rows[:3], "(3, 32)"), (rows[:, :31], "(4, 31)"), (rows[0], "(32,)")):
        for call in (lambda: _history((bad_rows, 7, 3, 100), 4, 32, "cpu"), lambda: make(bad_rows)):
            with pytest.raises(ValueError) as e:
                call()
            assert str(e.value) == f"history's previous rows have shape (4, 32), got {shape}"
    for call in (lambda: _history((rows, 7, 3, 100, [1, 0, 1]), 4, 32, "cpu"), lambda: make(rows, [1, 0, 1])):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == "history's valid mask has shape (4,), got (3,)"
    for call in (lambda: _history((rows, "x", 3, 100), 4, 32, "cpu"), lambda: LastMove(rows, 7, None, 100, m=4, words=32, device="cpu")):
        with pytest.raises((ValueError, TypeError)):   # (int() of the keys, as before)
            call()


def test_last_move_presents_a_history_of_one_entry():
    import torch

    from hanabi_hip import LastMove
    from hanabi_hip.search import _history

    rows = torch.arange(4 * 32, dtype=torch.int64).view(4, 32)   # (any integer type: moved to int32)
    h = _history((rows, 7, 3, 100, [2, 0, 1, 1]), 4, 32, "cpu")
    assert isinstance(h, LastMove) and (h.depth, h.filled, h.draws, h.alive, h.moves) == (1, 1, [3], None, None)
    assert (h.m, h.state_words, h.partner_seed, h.partner_draw, h.first_game_id) == (4, 32, 7, 3, 100)
    assert h.prev_rows.shape == (1, 4, 32) and h.prev_rows.dtype == torch.int32 and h.prev_rows.is_contiguous()
    assert torch.equal(h.prev_rows[0], rows.int())
    assert h.valid.shape == (1, 4) and h.valid.dtype == torch.uint8 and h.valid.tolist() == [[1, 0, 1, 1]]
    # it unpacks as the tuple it was made from
    prev, seed, draw, gid, valid = h
    assert torch.equal(prev, rows.int()) and (seed, draw, gid) == (7, 3, 100) and valid.tolist() == [1, 0, 1, 1]
    assert h[1] == 7 and h[4].tolist() == [1, 0, 1, 1]
    for none in (_history((rows, 7, 3, 100), 4, 32, "cpu"), _history((rows, 7, 3, 100, None), 4, 32, "cpu")):
        assert none.valid is None and none[4] is None


def test_survivors_is_n_surv_at_the_depth_used():
    import torch

    from hanabi_hip import BeliefSample

    n_surv = torch.tensor([[9, 8, 7, 0, 5], [6, 8, 0, 0, 4], [3, 0, 0, 0, 4]], dtype=torch.int32)
    used = torch.tensor([3, 2, 1, 0, 0], dtype=torch.int32)
    s = BeliefSample(None, None, n_surv, used, torch.tensor([0, 0, 0, 1, 2], dtype=torch.uint8), None)
    assert len(s) == 6 and s._fields == ("rows", "weights", "n_surv", "depth_used", "fallback", "ess")
    got = s.survivors()
    assert got.dtype == torch.int32 and got.tolist() == [3, 8, 7, 0, 0]   # (root 4: survivors at depth 1, but no depth used)
    one = BeliefSample(None, None, n_surv[:1], (used > 0).int(), None, None)
    assert one.survivors().tolist() == [9, 8, 7, 0, 0]


def test_the_restatements_moved_out_of_the_search_module():
    import hanabi_hip
    from hanabi_hip import belief_ref, search

    for name in ("belief_select_soft_ref", "belief_carry_ref", "belief_score_ref"):
        assert getattr(hanabi_hip, name) is getattr(belief_ref, name) and name in hanabi_hip.__all__
        assert not hasattr(search, name)
    for name in ("BeliefSample", "LastMove"):
        assert getattr(hanabi_hip, name) is getattr(search, name) and name in hanabi_hip.__all__
