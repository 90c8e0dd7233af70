"""hanabi_hip — thin Python host layer over the C-ABI of include/hanabi_hip.h.

PyTorch is used only for device memory and streams: every call hands raw device pointers
(`tensor.data_ptr()`) and the current HIP stream to `libhanabi_hip.so` through ctypes.
There is no CPU path: constructing an env or a tree without the compiled library or
without a GPU raises.

Public names: `HanabiEnv`, `SumTree`, `Evaluator`, `EvalResult`, `CrossPlay`, `CrossPlayResult`, `PartnerPool`, `PartnerStats`, `Determinizer`, `ConditionedDeterminizer`, `RolloutSearch`, `SearchPlayer`, `SearchResult`, `BeliefSample`, `LastMove`, `belief_splice`, `belief_select`, `belief_splice_alive`, `belief_select_depth`, `belief_select_soft`, `belief_select_soft_ref`, `soft_table`, `PartnerHistory`, `last_move_uid`, `search_leaf`, `leaf_dither`, `search_leaf_ref`, `leaf_dither_ref`, `OffBeliefSession`, `encode_rows`, `encode_rows_ref`, `rule_playout`, `playout_supported`, `PlayoutResult`, `rule_playout_grouped`, `crossplay_playout_supported`, `GroupedPlayoutResult`, `RuleSearch`, `belief_enumerate`, `belief_enumerate_ref`, `exact_rows`, `exact_supported`, `ExactBelief`, `ExactDeterminizer`, `make_config`, `HbConfig`, `lib`, flag constants.
"""
from ._capi import (FLAG_AUTO_RESET, FLAG_LENIENT_REWARD, FLAG_RESET_START_NEXT, GAME_TYPES, HbConfig, HbError,
                    lib, library_path, make_config)
from . import ops
from .env import HanabiEnv
from .evaluate import EvalResult, Evaluator
from .crossplay import CrossPlay, CrossPlayResult
from .partner_pool import PartnerPool, PartnerStats
from .search import (BeliefSample, BeliefScore, ConditionedDeterminizer, Determinizer, LastMove, PartnerHistory, RolloutSearch, SearchPlayer,
                     SearchResult, belief_carry, belief_figures, belief_score, exact_table, TrackedBelief, TrackedRows, belief_stats_of,
                     belief_select, belief_select_depth, belief_select_soft, belief_splice, belief_splice_alive, last_move_uid, soft_table,
                     LEAF_SCALE, leaf_dither, search_leaf)
from .belief_ref import (belief_carry_ref, belief_enumerate_ref, belief_score_ref, belief_select_soft_ref, leaf_dither_ref,
                         search_leaf_ref)
from .exact import ExactBelief, ExactDeterminizer, belief_enumerate, exact_rows, exact_supported
from .tree import SumTree
from .obl import OffBeliefSession
from .encode import encode_rows, encode_rows_ref
from .playout import (GroupedPlayoutResult, PlayoutResult, crossplay_playout_supported, playout_supported, rule_playout,
                      rule_playout_grouped)
from .rule_search import RuleSearch

__all__ = ["ops", "HanabiEnv", "SumTree", "Evaluator", "EvalResult", "CrossPlay", "CrossPlayResult", "PartnerPool", "PartnerStats", "Determinizer", "ConditionedDeterminizer", "RolloutSearch", "SearchPlayer", "SearchResult", "BeliefSample", "LastMove", "belief_splice", "belief_select", "belief_splice_alive", "belief_select_depth", "belief_select_soft", "belief_select_soft_ref", "soft_table", "belief_score", "belief_score_ref", "belief_carry", "belief_carry_ref", "exact_table", "TrackedBelief", "TrackedRows", "belief_figures", "belief_stats_of", "BeliefScore", "PartnerHistory", "last_move_uid", "LEAF_SCALE", "leaf_dither", "leaf_dither_ref", "search_leaf", "search_leaf_ref", "OffBeliefSession", "encode_rows", "encode_rows_ref", "rule_playout", "playout_supported", "PlayoutResult", "rule_playout_grouped", "crossplay_playout_supported", "GroupedPlayoutResult", "RuleSearch", "belief_enumerate", "belief_enumerate_ref", "exact_rows", "exact_supported", "ExactBelief", "ExactDeterminizer", "make_config", "HbConfig", "HbError", "lib", "library_path", "GAME_TYPES",
           "FLAG_AUTO_RESET", "FLAG_RESET_START_NEXT", "FLAG_LENIENT_REWARD"]
