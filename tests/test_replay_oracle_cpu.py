"""CPU: the trajectory oracle (oracle/replay_oracle.py) and the torch fallback of the replay ring pinned to each other over
the whole case table (tests/replay_cases.py), the table's teeth (every wrong variant of the ring walk is caught by some case),
and the hb_per_sample_gather cases' sampled indices. The GPU tests (tests/test_replay_kernels_oracle.py) hold the kernels to
the same oracle answers."""
import numpy as np
import pytest

import replay_cases as RC
from oracle.replay_oracle import ReplayOracle

RING = (("_obs_tm1_buf", "obs_tm1"), ("_obs_t_buf", "obs_t"), ("_act_tm1_buf", "act"), ("_lms_t_buf", "lms"),
        ("_rew_t_buf", "rew"), ("_terminal_t_buf", "term"))


def test_oracle_hand_worked_example():
    """Two games, capacity 3: the third row of the stream overwrites nothing, the fourth replaces slot 0."""
    o = ReplayOracle(3, np.array([[10], [20]], np.int8))
    o.insert(np.array([[11], [21]], np.int8), np.ones((2, 2), np.int8), [0, 1], np.float32([0.5, -1.0]), [1, 1])
    assert (o.size, o.write_pointer, o.holder) == (2, 2, [(0, 0), (0, 1), None])
    o.insert(np.array([[12], [22]], np.int8), np.ones((2, 2), np.int8), [1, 0], np.float32([2.0, 4.0]), [2, 1])
    assert (o.size, o.write_pointer, o.holder) == (3, 1, [(1, 1), (0, 1), (1, 0)])
    r = o.expected_ring()
    assert r["obs_tm1"][:, 0].tolist() == [21, 20, 11] and r["obs_t"][:, 0].tolist() == [22, 21, 12]
    assert r["rew"][:, 0].tolist() == [4.0, -1.0, 2.0] and r["term"][:, 0].tolist() == [False, False, True]
    assert r["last_obs"][:, 0].tolist() == [12, 22]
    g = float(np.float32(0.9))
    a = o.nstep(1, 3, 0.9)      # game 1 from its first transition: -1 + g * 4, then nothing further has happened
    assert (a["m"], a["terminal"], int(a["obs_t"][0]), int(a["obs_tm1"][0])) == (2, False, 22, 20)
    assert a["R"] == -1.0 + g * 4.0 and a["S"] == 1.0 + g * 4.0 and a["disc"] == g * g
    b = o.nstep(2, 3, 0.9)      # game 0's terminal transition: one step
    assert (b["m"], b["terminal"], b["R"], b["disc"]) == (1, True, 2.0, g)
    assert o.nstep(1, 1, 0.9)["m"] == 1 and o.nstep(0, 5, 0.9)["m"] == 1


def test_table_covers_what_it_promises():
    Ls, As, rings = {c.L for c in RC.CASES}, {c.A for c in RC.CASES}, {(c.cap, c.n_ins) for c in RC.CASES}
    assert Ls == {1, 31, 32, 33, 171, 658} and As == {11, 20, 48}
    assert rings == {(40, 8), (37, 5), (8, 8), (16, 8), (2000, 48)}
    assert {c.gamma for c in RC.CASES} == {0.99, 0.9, 1.0} and {c.B for c in RC.CASES} == {1, 5, 64}
    assert {d for c in RC.CASES for d in c.dtypes} == {"f32", "bf16", "f16"}
    assert [c.x_ld for c in RC.CASES if c.x_ld != c.L] == [704] and sum(c.arbitrary for c in RC.CASES) == 1
    assert {p.B for p in RC.PSG_CASES} == {1, 2, 5, 64} and {p.n_step for p in RC.PSG_CASES} == {1, 3}
    kinds = set()
    for c in RC.CASES:
        for state, s in RC.scenario(c.name).items():
            size, wp = s["ring"]["size"], s["ring"]["write_pointer"]
            kinds.add("partial" if size < c.cap else "full_wp0" if wp == 0 and state * c.n_ins == c.cap else
                      "laps" if state * c.n_ins > 2 * c.cap else "wrapped_mid" if wp else "laps_wp0")
            assert (s["ring"]["rew"][:size] != np.round(s["ring"]["rew"][:size])).any()   # rewards are not all integers
    assert kinds >= {"partial", "full_wp0", "wrapped_mid", "laps"}, kinds
    # the hand-placed terminals: at the sampled transition, at the last step of a chain, twice in a row, in the newest insert
    s = RC.scenario("m40_i8_L658_pad")[7]
    t3 = s["nstep"][3]
    assert any(t and m == 1 for t, m in zip(t3["term"], t3["m"])) and any(t and m == 3 for t, m in zip(t3["term"], t3["m"]))
    assert any(k == 6 and t for (k, g), t in zip(t3["last"], t3["term"]))
    games = {}
    for slot, (k, g) in enumerate(s["holder"]):
        games.setdefault(g, {})[k] = bool(s["ring"]["term"][slot, 0])
    assert any(games[1].get(k) and games[1].get(k + 1) for k in range(7))


@pytest.mark.parametrize("name", [c.name for c in RC.CASES])
def test_oracle_equals_torch_fallback(name):
    """Ring contents after every insert, and gather_nstep_dev at every slot in range(size), n_step 1 / 2 / 3 / 5, at every
    state of the case: ExperienceBuffer(device="cpu") against the trajectory oracle."""
    import torch

    from hanabi_agents.rlax_dqn.experience_buffer import ExperienceBuffer

    case = RC.BY_NAME[name]
    first, inserts = RC.case_inputs(case)
    scen = RC.scenario(name)
    buf = ExperienceBuffer(case.L, case.A, 1, case.cap, device="cpu", packed=case.packed)
    orc, last = ReplayOracle(case.cap, first), first
    form = (lambda a: RC.pack_rows(a, case.L)) if case.packed else (lambda a: a)
    worst = [0.0, 0.0]
    for k, (obs, legal, action, reward, st) in enumerate(inserts):
        buf.add_transitions(last, action.reshape(-1, 1), reward.reshape(-1, 1), obs, legal, (st == 2).reshape(-1, 1))
        orc.insert(obs, legal, action, reward, st)
        last = obs
        ring = orc.expected_ring()
        assert (buf.size, buf.oldest_entry, buf.rows_per_insert) == (ring["size"], ring["write_pointer"], case.n_ins)
        for attr, key in RING:
            want = form(ring[key]) if key.startswith("obs") else ring[key]
            assert np.array_equal(getattr(buf, attr).numpy(), want), (k, key)
        if k + 1 not in scen:
            continue
        size, idx = ring["size"], torch.arange(ring["size"])
        for n in RC.N_STEPS:
            exp, where = scen[k + 1]["nstep"][n], (name, k + 1, n)
            tr, disc = buf.gather_nstep_dev(idx, n, case.gamma)
            assert np.array_equal(tr.observation_tm1.numpy(), exp["obs_tm1"]), where
            assert np.array_equal(tr.observation_t.numpy(), exp["obs_t"]), where
            assert np.array_equal(tr.legal_moves_t.numpy(), exp["legal"]), where
            assert np.array_equal(tr.action_tm1.numpy()[:, 0], exp["act"]), where
            assert np.array_equal(tr.terminal_t.numpy()[:, 0], exp["term"]), where
            d, r = RC.check_rew_disc(tr.reward_t.numpy()[:, 0], disc.numpy(), exp, np.arange(size), n, case.gamma, ring["rew"], where)
            worst = [max(worst[0], d), max(worst[1], r)]
    print(f"{name}: worst error / bound: disc {worst[0]:.3f}, rew {worst[1]:.3f}")


# ---- the table has teeth ----------------------------------------------------------------------------------------------------
def _walk(variant, rew, term, holder, n_ins, cap, size, wp, i, n):
    """The ring walk of the kernels and the fallback, with one deliberate mistake (variant None: none). Works on slot numbers
    only and returns what can be compared discretely: (the (insert, game) its last step landed on, steps, terminal flag).
    A slot past the ring's end reads as empty."""
    def t(j):
        return bool(term[j, 0]) if j < cap else False

    ahead = (wp - 1 - i) % cap if size >= cap else size - 1 - i
    if variant == "bound_from_capacity_when_partly_filled":
        ahead = (wp - 1 - i) % cap if size >= cap else cap - 1 - i
    stride = n_ins + 1 if variant == "stride_plus_one" else n_ins
    j, m = i, 1
    while m < n and (variant == "ignores_terminal" or not t(j)) and (
            m * n_ins < ahead if variant == "lt_for_le" else m * n_ins <= ahead):
        j = j + stride if variant == "successor_not_wrapped" else (j + stride) % cap
        m += 1
    last = i if variant == "obs_t_and_terminal_from_first_step" else j
    return (holder[last] if last < cap else None), m, t(last)


VARIANTS = ("lt_for_le", "stride_plus_one", "successor_not_wrapped", "ignores_terminal",
            "bound_from_capacity_when_partly_filled", "obs_t_and_terminal_from_first_step")


def _mismatches(variant):
    """Names of the (case, state, n_step) at which the variant's walk differs from the oracle at some slot."""
    hits = []
    for case in RC.CASES:
        if case.cap > 100:   # the small rings must do it alone
            continue
        for state, s in RC.scenario(case.name).items():
            ring = s["ring"]
            for n in RC.N_STEPS:
                exp = s["nstep"][n]
                for i in range(ring["size"]):
                    got = _walk(variant, ring["rew"], ring["term"], s["holder"], case.n_ins, case.cap, ring["size"],
                                ring["write_pointer"], i, n)
                    if got != (exp["last"][i], int(exp["m"][i]), bool(exp["term"][i])):
                        hits.append((case.name, state, n))
                        break
    return hits


def test_the_correct_walk_matches_the_oracle_everywhere():
    assert _mismatches(None) == []


@pytest.mark.parametrize("variant", VARIANTS)
def test_table_catches_wrong_walk(variant):
    hits = _mismatches(variant)
    print(f"{variant}: caught by {len(hits)} (case, state, n_step) rows, first {hits[:3]}")
    assert hits, f"no case of the table notices the walk variant {variant}: the table is too weak"


# ---- hb_per_sample_gather cases: every sampled index is a written slot -------------------------------------------------------------
@pytest.mark.parametrize("pc", RC.PSG_CASES, ids=lambda p: f"{p.case}-s{p.state}-B{p.B}")
def test_sampled_indices_stay_inside_the_ring(pc):
    size = RC.scenario(pc.case)[pc.state]["ring"]["size"]
    tree = RC.psg_oracle_tree(pc, size)
    assert (tree.leaves()[:size] > 0).all() and not tree.leaves()[size:].any()
    for counter in RC.PSG_COUNTERS:
        u = RC.philox_uniforms(pc.seed, counter, pc.B)
        assert (u >= 0).all() and (u < 1.0 / pc.B).all()
        idx, prob = tree.per_sample(u)
        assert (idx >= 0).all() and (idx < size).all() and (prob > 0).all(), (counter, idx)
