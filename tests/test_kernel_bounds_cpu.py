"""No GPU: the guard-band sweep's table covers the whole C-ABI, and the guard helper itself bites.

1. Every symbol of hanabi_hip._capi.SIGNATURES (one entry per prototype of include/hanabi_hip.h, tests/test_capi_symbols.py)
   is a key of kernel_bounds_cases.CASES or of its EXEMPT dict, never both, and neither dict has a stale key: a new entry
   point cannot be added without someone deciding where its bounds are checked.
2. guard_util.GuardSet on torch CPU tensors: an element written into the front guard, into the tail guard, and a flipped byte
   of a registered input are each reported with the buffer's name and the damaged offset. No kernel is altered for this."""
import re

import pytest

import kernel_bounds_cases as KB
from guard_util import FILL, FRONT, GuardSet, PlainSet, guarded, same_bits


def _signatures():
    from hanabi_hip import _capi

    return set(_capi.SIGNATURES)


def test_every_entry_point_has_a_case_or_an_exemption():
    names = _signatures()
    cases, exempt = set(KB.CASES), set(KB.EXEMPT)
    missing = sorted(names - cases - exempt)
    assert not missing, f"entry points with neither a bounds case nor an exemption: {missing}"
    assert not sorted(cases & exempt), f"both a case and an exemption: {sorted(cases & exempt)}"
    assert not sorted(cases - names), f"stale keys in CASES: {sorted(cases - names)}"
    assert not sorted(exempt - names), f"stale keys in EXEMPT: {sorted(exempt - names)}"
    for name, reason in KB.EXEMPT.items():
        assert isinstance(reason, str) and len(reason) > 10, name


def test_exemptions_are_of_the_three_kinds():
    """host-only, library-owned memory, or one of the three entry points whose own test file guards every output."""
    own = {"hb_encode_rows": "tests/test_encode_rows_gpu.py", "hb_belief_score": "tests/test_belief_score_gpu.py",
           "hb_belief_carry": "tests/test_belief_carry_gpu.py"}
    import os

    for name, reason in KB.EXEMPT.items():
        if name in own:
            assert own[name] in reason
            path = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.path.basename(own[name]))
            assert "_guarded" in open(path).read(), path
        else:
            assert reason.startswith("host-only") or reason.startswith("writes only memory the library owns"), (name, reason)


def test_the_header_declares_what_the_table_names():
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "hanabi_hip.h")).read()
    protos = set(re.findall(r"^(?:const\s+)?[A-Za-z_][\w\s\*]*?\b(hb_\w+)\s*\(", text, re.M))
    assert set(KB.CASES) <= protos, sorted(set(KB.CASES) - protos)


def test_the_table_is_well_formed():
    ids = set()
    for entry, fn, p in KB.flat_cases():
        assert callable(fn) and isinstance(p, tuple)
        i = KB.case_id(entry, p)
        assert i not in ids, f"duplicate case {i}"
        ids.add(i)
    assert KB.edge_sizes(128) == [1, 127, 129] and KB.edge_sizes(16, 64) == [1, 15, 17, 65] and KB.edge_sizes(1, 4) == [1, 2, 5]
    assert KB.tail(4, 1) == FRONT and KB.tail(128, 20) == 2560


def test_cases_name_rows_of_the_shared_tables_that_exist():
    """The replay cases are picked by name / index out of tests/replay_cases.py: a renamed row there must fail here, on the host."""
    import replay_cases as RC

    insert = {c.name for c in RC.INSERT_CASES} | set(KB.INSERT_EDGES)
    for _, (name,) in KB.CASES["hb_replay_insert"]:
        assert name in insert, name
    assert {c.name for c in RC.INSERT_CASES} <= {p[0] for _, p in KB.CASES["hb_replay_insert"]}
    for entry in ("hb_replay_gather", "hb_replay_gather_packed"):
        for _, (name, state, n_step) in KB.CASES[entry]:
            rc = RC.BY_NAME[name]
            assert state in rc.states and n_step in RC.N_STEPS and rc.packed == entry.endswith("packed"), (entry, name)
    assert {i for _, (i,) in KB.CASES["hb_per_sample_gather"]} == set(range(len(RC.PSG_CASES)))
    assert any(RC.BY_NAME[RC.PSG_CASES[i].case].x_ld > RC.BY_NAME[RC.PSG_CASES[i].case].L for _, (i,) in KB.CASES["hb_per_sample_gather"])


def test_removing_a_case_is_noticed(monkeypatch):
    cases = dict(KB.CASES)
    del cases["hb_env_step_packed"]
    monkeypatch.setattr(KB, "CASES", cases)
    with pytest.raises(AssertionError, match="hb_env_step_packed"):
        test_every_entry_point_has_a_case_or_an_exemption()


# ---- the helper, on the host ---------------------------------------------------------------------------------------------------
def test_guarded_layout():
    import torch

    for dtype in (torch.int8, torch.uint8, torch.int16, torch.bfloat16, torch.float16, torch.int32, torch.float32, torch.int64,
                  torch.float64):
        buf, view = guarded((3, 7), dtype, FILL, 100, device="cpu")
        item = buf.element_size()
        assert buf.numel() == FRONT + 21 + 100 and view.shape == (3, 7) and view.is_contiguous()
        assert view.data_ptr() - buf.data_ptr() == FRONT * item and (FRONT * item) % 16 == 0
        assert bool((buf.view(torch.uint8) == FILL).all())
    with pytest.raises(ValueError):
        guarded((4,), torch.int8, FILL, FRONT - 1, device="cpu")
    with pytest.raises(ValueError):
        guarded((4,), torch.int8, 0, FRONT, device="cpu")
    with pytest.raises(ValueError):
        guarded((4,), torch.int8, 0xFF, FRONT, device="cpu")


def test_guardset_reports_front_tail_and_input_damage():
    import torch

    gs = GuardSet("hb_fake_entry", device="cpu")
    a = gs.out("q", (5, 4), torch.float32, 80)
    b = gs.out("actions", (5,), torch.int32, 64, init=torch.arange(5, dtype=torch.int32))
    x = gs.inp("legal", torch.arange(40, dtype=torch.int8).reshape(5, 8))
    assert b.tolist() == [0, 1, 2, 3, 4]
    assert gs.untouched() == ["q"]    # (an in/out argument is never reported: its payload was written by `init`)
    a.fill_(1.0)                      # writing the whole payload is what a kernel does
    assert gs.untouched() == []
    b.add_(1)
    gs.check("clean")
    assert gs.problems() == []

    # a deliberately oversized view of q's buffer: element -1 is the last front-guard element, element 20 the first of the tail
    buf_q = gs.outs["q"][0]
    wide = buf_q[FRONT - 8:FRONT + 20 + 8]
    wide[7] = 3.0                     # payload offset -1
    with pytest.raises(AssertionError) as e:
        gs.check("front")
    msg = str(e.value)
    assert msg.startswith("front: ") and "output 'q'" in msg and "front guard" in msg and "element -1 " in msg, msg
    assert "actions" not in msg and "legal" not in msg
    wide[7] = torch.tensor([FILL] * 4, dtype=torch.uint8).view(torch.float32)[0]
    gs.check("repaired")

    wide[8 + 20 + 2] = 0.0            # payload offset 22: two elements past the end
    with pytest.raises(AssertionError) as e:
        gs.check()
    msg = str(e.value)
    assert msg.startswith("hb_fake_entry: ") and "output 'q'" in msg and "tail guard" in msg and "element 22 " in msg, msg
    wide[8 + 20 + 2] = torch.tensor([FILL] * 4, dtype=torch.uint8).view(torch.float32)[0]

    # the last byte of the last tail element of the other output
    buf_a = gs.outs["actions"][0]
    buf_a.view(torch.uint8)[-1] ^= 0x01
    with pytest.raises(AssertionError) as e:
        gs.check("tail end")
    msg = str(e.value)
    assert "output 'actions'" in msg and "tail guard" in msg and f"element {5 + 64 - 1} " in msg and "byte 3" in msg, msg
    assert "'q'" not in msg
    buf_a.view(torch.uint8)[-1] ^= 0x01
    gs.check("repaired again")

    x.view(torch.uint8).reshape(-1)[13] ^= 0x40      # one byte of a registered input
    with pytest.raises(AssertionError) as e:
        gs.check("input")
    msg = str(e.value)
    assert "input 'legal'" in msg and "element 13 " in msg and "output" not in msg, msg


def test_guardset_input_offsets_count_elements_and_names_are_unique():
    import torch

    gs = GuardSet("e", device="cpu")
    x = gs.inp("prios", torch.zeros(6, dtype=torch.float64))
    x.view(torch.uint8)[8 * 4 + 5] = 1
    (msg,) = gs.problems()
    assert "input 'prios'" in msg and "element 4 " in msg and "byte 5" in msg
    with pytest.raises(KeyError):
        gs.out("prios", (1,), torch.int8, 64)
    with pytest.raises(KeyError):
        gs.inp("prios", x)


def test_plainset_matches_guardset_payloads():
    import torch

    g, p = GuardSet("e", device="cpu"), PlainSet("e", device="cpu")
    for s in (g, p):
        s.out("a", (2, 3), torch.int16, 64)
        s.out("b", (4,), torch.float32, 64, init=torch.ones(4))
        s.out("empty", (0, 5), torch.int8, 64)
        t = torch.zeros(3)
        assert s.inp("x", t) is t
    assert g.payloads().keys() == p.payloads().keys()
    for k in g.payloads():
        assert same_bits(g.payloads()[k], p.payloads()[k]) == -1
        assert p.payloads()[k].is_contiguous()
    p.payloads()["a"][1, 2] = 7
    assert same_bits(g.payloads()["a"], p.payloads()["a"]) == 5
    assert bool((g.payloads()["a"].view(torch.uint8) == FILL).all())
