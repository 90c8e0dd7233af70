"""CPU-side checks of the drop-in boundary: the C-ABI library builds/loads and exports every
symbol include/hanabi_hip.h declares; pure-host size functions agree with the oracle; the
product refuses to run without a GPU instead of falling back to anything on the CPU."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    text = open(os.path.join(ROOT, "include", "hanabi_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(hb_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    import hanabi_hip

    L = hanabi_hip.lib()
    names = header_functions()
    assert len(names) >= 30
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/hanabi_hip.h but not exported"
    from hanabi_hip import _capi

    assert sorted(_capi.SIGNATURES) == names, "ctypes table and header disagree"
    assert L.hb_abi_version() == 1


def test_host_size_functions_match_oracle():
    import hanabi_hip
    from oracle import oracle_py as O

    L, OL = hanabi_hip.lib(), O.lib()
    for game in ("Hanabi-Full", "Hanabi-Small", "Hanabi-Very-Small"):
        for players in (2, 3, 4, 5):
            cfg = hanabi_hip.make_config(game, players)
            ocfg = O.make_config(game, players)
            assert L.hb_config_validate(C.byref(cfg)) == 0
            assert L.hb_obs_len(C.byref(cfg)) == OL.orc_obs_len(C.byref(ocfg))
            assert L.hb_num_actions(C.byref(cfg)) == OL.orc_num_actions(C.byref(ocfg))
            assert L.hb_deck_size(C.byref(cfg)) == OL.orc_deck_size(C.byref(ocfg))
            assert L.hb_state_words(C.byref(cfg)) == OL.orc_state_words(C.byref(ocfg))
    cfg = hanabi_hip.make_config()
    assert (L.hb_obs_len(C.byref(cfg)), L.hb_num_actions(C.byref(cfg))) == (658, 20)
    bad = hanabi_hip.HbConfig(6, 5, 5, 5, 8, 3, 0)
    assert L.hb_config_validate(C.byref(bad)) != 0 and b"players" in L.hb_last_error()


def test_no_cpu_fallback():
    import torch

    import hanabi_hip

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(hanabi_hip.HbError):
        hanabi_hip.HanabiEnv(n_games=2)
    with pytest.raises(hanabi_hip.HbError):
        hanabi_hip.SumTree(8)
    # and the C-ABI itself reports "no device" rather than computing anything
    h = C.c_void_p()
    cfg = hanabi_hip.make_config()
    assert hanabi_hip.lib().hb_env_create(C.byref(cfg), 4, 1, 0, C.byref(h)) == -2
    assert hanabi_hip.lib().hb_tree_create(8, C.byref(h)) == -2


def test_product_never_touches_the_oracle():
    """Only tests/, bench.py's cpu_baseline leg and __graft_entry__.smoke() may use oracle/."""
    pkg = os.path.join(ROOT, "hanabi-agents_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h", ".cpp")):
                text = open(os.path.join(dirpath, f)).read()
                for needle in ("oracle_py", "liboracle", "from oracle", "import oracle", "orc_"):
                    assert needle not in text, f"{f} references the oracle ({needle})"


def test_argument_validation_needs_no_gpu():
    """Every entry point checks its arguments before it touches the device: bad calls come back with a negative code and a
    message, never a crash — also on a machine without a GPU (nothing here launches anything)."""
    import hanabi_hip
    from hanabi_hip import _capi as K

    L = hanabi_hip.lib()
    cfg = hanabi_hip.make_config()
    one = C.c_void_p(16)      # a non-null, 16-byte aligned fake pointer: validation must reject the call before using it
    assert L.hb_actor_hidden(None, 10, 658, one, 704, one, 512, one, None) < 0 and b"null" in L.hb_last_error()
    assert L.hb_actor_hidden(one, 10, 658, one, 700, one, 512, one, None) < 0 and b"multiple of 64" in L.hb_last_error()
    assert L.hb_actor_hidden(one, 10, 658, one, 704, one, 500, one, None) < 0 and b"multiple of 256" in L.hb_last_error()
    assert L.hb_actor_hidden(one, 0, 658, one, 704, one, 512, one, None) == 0            # empty batch: no-op
    assert L.hb_actor_q(one, 10, 500, one, one, one, 20, 51, one, None) < 0
    assert L.hb_actor_q(one, 10, 512, one, one, one, 20, 300, one, None) < 0 and b"n_atoms" in L.hb_last_error()
    assert L.hb_actor_q(one, 0, 512, one, one, one, 20, 51, one, None) == 0
    assert L.hb_policy_select(one, one, 5, 65, 0.1, 1, 1, 0, one, None) < 0
    assert L.hb_policy_select(one, one, 0, 20, 0.1, 1, 1, 0, one, None) == 0
    jobs = (K.HbPackJob * 1)()
    assert L.hb_actor_pack_weights(jobs, 1, None) < 0 and b"null pointer in job 0" in L.hb_last_error()
    assert L.hb_actor_pack_weights(jobs, 5, None) < 0
    rules = (K.HbRule * 1)()
    rules[0].kind = 99
    assert L.hb_rule_act(C.byref(cfg), one, 4, 0, rules, 1, 1, 1, one, None, None) < 0 and b"unknown kind" in L.hb_last_error()
    assert L.hb_rule_act(C.byref(cfg), one, 4, 0, rules, 17, 1, 1, one, None, None) < 0
    assert L.hb_rule_act(C.byref(cfg), one, 0, 0, rules, 0, 1, 1, one, None, None) == 0
    assert L.hb_relu_bwd_colsum(one, one, 4, 1, 8, 8, one, None) < 0 and b"act_ld" in L.hb_last_error()
    assert L.hb_colsum(None, 1, 8, 8, one, None) < 0
    tab = (K.HbAdamTensor * 1)()
    assert L.hb_noisy_adam_multi(tab, 1, one, 1.0, 1, 1e-3, 0.9, 0.999, 1e-5, None) < 0 and b"tensor 0" in L.hb_last_error()
    assert L.hb_noisy_adam_multi(tab, 9, one, 1.0, 1, 1e-3, 0.9, 0.999, 1e-5, None) < 0
    # round 3: the packing Adam, the one-kernel actor's entry points and the chain
    packs = (K.HbAdamPack * 1)()
    assert L.hb_noisy_adam_multi_pack(tab, packs, 1, one, 1.0, 1, 1e-3, 0.9, 0.999, 1e-5, None) < 0 and b"tensor 0" in L.hb_last_error()
    assert L.hb_noisy_adam_multi_pack(tab, packs, 5, one, 1.0, 1, 1e-3, 0.9, 0.999, 1e-5, None) < 0
    assert L.hb_noisy_adam_multi_pack(tab, packs, 1, one, 1.0, 0, 1e-3, 0.9, 0.999, 1e-5, None) < 0 and b"16-bit" in L.hb_last_error()
    cols = (C.c_int32 * (20 * 51))()
    assert L.hb_actor_fused_columns(20, cols) == 0 and sorted(cols) == sorted(set(cols)) and max(cols) < 1024 and min(cols) >= 0
    assert L.hb_actor_fused_columns(81, cols) < 0
    assert L.hb_actor_fused_supported(658, 512, 20, 51) == 1 and L.hb_actor_fused_supported(658, 512, 81, 51) == 0
    assert L.hb_actor_fused_q_dt(one, 10, 658, one, one, one, one, one, 512, 20, 51, one, 3, None) < 0 and b"dtype" in L.hb_last_error()
    assert L.hb_actor_fused_act_dt(one, None, 10, 658, one, one, one, one, one, 512, 20, 51, one, 0.1, 1, 1, 0, one, 1, None) < 0
    assert L.hb_actor_fused_pack_thin(one, 512, one, one, 1024, one, 658, 512, 20, 51, one, one, one, one, one, 100, None, 0, 1, None) < 0
    assert b"w1t" in L.hb_last_error()
    assert L.hb_thin_gemm(one, one, None, one, 32, 16, 32, 32, 32, 16, 1, 0, 0, 0, 8, None) < 0 and b"relu" in L.hb_last_error()
    cmds = (K.HbCmd * 1)()
    cmds[0].op, cmds[0].var, cmds[0].fvar, cmds[0].cond = 99, -1, -1, -1
    assert L.hb_chain_run(cmds, 1, None, None) < 0 and b"unknown op" in L.hb_last_error()
    assert L.hb_chain_run(cmds, 0, None, None) == 0
    assert L.hb_per_sample_philox(None, 1, one, 4, one, one, None) < 0
    assert L.hb_tree_import_nodes(None, one, None) < 0
    assert L.hb_tree_set_ring(None, 8) < 0 and b"null tree" in L.hb_last_error()   # (its range check needs a tree: tests/test_per_ring_gpu.py)
    assert L.hb_env_state(None) is None
