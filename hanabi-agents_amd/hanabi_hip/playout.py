"""Rule-list teams played to the end in one kernel launch: hb_rule_playout and hb_rule_playout_grouped
(include/hanabi_hip_playout.h, csrc/playout.hip).

The turn loop of `Evaluator.run` and `search.rollout` issues three launches per turn (the seat's moves, the env step, the tally)
and moves every game's state row, observation and legal mask through HBM each time. A team made only of `RulebasedAgent`s reads
no observation: `rule_playout` plays its games from their state rows to the end inside one kernel, one lane per game with the row
in LDS, and leaves the rows, `done`, `final_score`, `length` and the counters bit for bit as the loop leaves them.

    res = rule_playout(cfg, rows, [piers, piers], seed=7)          # rows [n, state_words] int32 on the GPU, played in place
    res.final_score, res.length, res.counters, res.max_len

`playout_supported(agents, **options)` says whether a team and a set of options can take this path; `Evaluator(playout=True)`,
`RolloutSearch(playout=True)`, `SearchPlayer(playout=True)` and `SelfPlaySession.search(playout=True)` ask it and fall back to
the loop otherwise. The switch is off by default everywhere.

`rule_playout_grouped` is the same for many teams at once: blocks of `block_games` games, one team per block, one launch, a
counter row and a longest game per block; block b's outputs are those of `rule_playout` on that block alone.
`crossplay_playout_supported(pool, teams, **options)` is the predicate `CrossPlay(playout=True)` asks.

    res = rule_playout_grouped(cfg, rows, [(piers, piers), (piers, iggi), None], seed=7, block_games=n)   # rows [3 * n, SW]
    res.counters[1], res.max_len[1]                                # None: a block that is not played

The entry points' ctypes signatures live here, bound on first use, and not in `_capi.SIGNATURES`: that table mirrors
include/hanabi_hip.h, and these prototypes are declared in a header of their own (see there for why).
"""
import ctypes as C
from typing import NamedTuple, Optional

import torch

from . import _capi as K

_FN = None


def _fn():
    """hb_rule_playout with its argument types, bound once."""
    global _FN
    if _FN is None:
        f = K.lib().hb_rule_playout
        f.restype = C.c_int
        f.argtypes = [C.POINTER(K.HbConfig), C.c_void_p, C.c_int64, C.c_int64, C.POINTER(C.POINTER(K.HbRule)), C.POINTER(C.c_int32),
                      C.c_uint64, C.c_int32, C.c_void_p, C.c_int32] + [C.c_void_p] * 7 + [C.c_void_p]
        _FN = f
    return _FN


_FN_GROUPED = None


def _fn_grouped():
    """hb_rule_playout_grouped with its argument types, bound once."""
    global _FN_GROUPED
    if _FN_GROUPED is None:
        f = K.lib().hb_rule_playout_grouped
        f.restype = C.c_int
        f.argtypes = ([C.POINTER(K.HbConfig), C.c_void_p] + [C.c_int64] * 4 + [C.c_void_p] * 3 + [C.c_int32, C.c_uint64, C.c_int32,
                      C.c_void_p, C.c_int32] + [C.c_void_p] * 7 + [C.c_void_p])
        _FN_GROUPED = f
    return _FN_GROUPED


def rule_tables(agents):
    """The host arguments `rules` and `n_rules` of hb_rule_playout for one rule agent per seat (the agents keep the tables alive)."""
    P = len(agents)
    tabs = (C.POINTER(K.HbRule) * P)(*[C.cast(a._tab, C.POINTER(K.HbRule)) for a in agents])
    lens = (C.c_int32 * P)(*[len(a.rules) for a in agents])
    return tabs, lens


def _is_rule_agent(a):
    from hanabi_agents.rule_based import RulebasedAgent

    return isinstance(a, RulebasedAgent)


def playout_supported(agents, responses=False, color_shuffle=False, horizon=None, **options):
    """True exactly when hb_rule_playout can play this team with these options: every seat a `RulebasedAgent` (a DQN seat, a
    `SearchPlayer`, a `PartnerPool` or anything else that is asked for its moves turn by turn is not), and no option on that the
    kernel does not cover: response counts, colour-shuffled frames, a rollout horizon, or any other option that is set. Pure host
    code."""
    agents = list(agents)
    if not agents or not all(_is_rule_agent(a) for a in agents):
        return False
    if responses or color_shuffle or horizon is not None:
        return False
    return not any(v not in (None, False) for v in options.values())


def crossplay_playout_supported(pool, teams, responses=False, color_shuffle=False, **options):
    """True exactly when hb_rule_playout_grouped can play these teams of this pool: `playout_supported` for every team, which
    looks only at the agents a team uses (a DQN agent in a pool slot no team names does not matter). teams: P-tuples of pool
    indices. Pure host code."""
    pool, teams = list(pool), list(teams)
    if not teams:
        return False
    used = {i for t in teams for i in t}
    if not all(0 <= i < len(pool) for i in used):
        return False
    return playout_supported([pool[i] for i in sorted(used)], responses=responses, color_shuffle=color_shuffle, **options)


class PlayoutResult(NamedTuple):
    """rows [n, SW] int32 as the games were left, done [n] uint8 (bit 7: finished, bits 0-6: lives lost), final_score [n] int8,
    length [n] int16, counters [hb_eval_counters] int64 (hb_eval_tally's; [0] = games still running), illegal [1] int64,
    max_len [1] int32: device tensors; actions [max_turns, n] int32 with log=True (-1 from a game's end on), else None."""
    rows: torch.Tensor
    done: torch.Tensor
    final_score: torch.Tensor
    length: torch.Tensor
    counters: torch.Tensor
    illegal: torch.Tensor
    max_len: torch.Tensor
    actions: Optional[torch.Tensor] = None


class GroupedPlayoutResult(NamedTuple):
    """PlayoutResult's fields over n_blocks * block_games games, the blocks one after another; counters [n_blocks,
    hb_eval_counters] int64 and max_len [n_blocks] int32 are per block, illegal [1] int64 is the launch's. A block that was not
    played (team None) keeps its rows, done, final_score, length and counter row as they were; its log entries are -1."""
    rows: torch.Tensor
    done: torch.Tensor
    final_score: torch.Tensor
    length: torch.Tensor
    counters: torch.Tensor
    illegal: torch.Tensor
    max_len: torch.Tensor
    actions: Optional[torch.Tensor] = None


def _check(t, shape, dtype, name):
    if not isinstance(t, torch.Tensor) or t.shape != tuple(shape) or t.dtype != dtype or not t.is_contiguous():
        got = f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"{name}: expected a contiguous {dtype} tensor of shape {tuple(shape)}, got {got}")


def rule_playout(cfg, rows, teams, seed, first_seat=0, first_moves=None, max_turns=None, first_game_id=0, done=None, log=False,
                 out=None):
    """Play the games of `rows` to the end (or for `max_turns` turns) IN PLACE with one `RulebasedAgent` per seat (`teams`).

    cfg: the games' configuration (its flags are ignored: no auto-reset, no leniency, as `evaluate.eval_config` builds it).
    rows [n, state_words] int32, contiguous, on the GPU. Turn t is seat (first_seat + t) % P's in every game; its move is the
    seat's rule walk with Philox (seed, draw t + 1, game id first_game_id + g), or first_moves[g] ([n] int32) on turn 0 when
    given. done: optional [n] uint8 status bytes as before turn 0 of the loop (0x80: a slot that is not played); default all
    zero. log=True records the moves. out: optional (final_score [n] int8, length [n] int16, counters [hb_eval_counters] int64)
    to write into; they are zeroed here and counters[0] set to the games played, as the loop's caller does. With out, `done` is
    used in place. Returns a `PlayoutResult`; nothing is read back to the host."""
    from .evaluate import max_turns as turn_bound

    L = K.lib()
    cfg = K.HbConfig(cfg.players, cfg.colors, cfg.ranks, cfg.hand_size, cfg.max_info, cfg.max_life, 0)
    if L.hb_config_validate(C.byref(cfg)) != 0:
        raise ValueError(f"invalid configuration {cfg!r}: {L.hb_last_error().decode()}")
    P, SW = cfg.players, L.hb_state_words(C.byref(cfg))
    teams = list(teams)
    if len(teams) != P:
        raise ValueError(f"one agent per seat: {P} players, {len(teams)} agents")
    if not playout_supported(teams):
        raise TypeError("rule_playout plays RulebasedAgent seats only: " + ", ".join(type(a).__name__ for a in teams))
    if not isinstance(rows, torch.Tensor) or rows.dim() != 2 or rows.shape[1] != SW or rows.dtype != torch.int32 or not rows.is_contiguous():
        got = f"{rows.dtype} {tuple(rows.shape)}" if isinstance(rows, torch.Tensor) else type(rows).__name__
        raise ValueError(f"rows: expected a contiguous torch.int32 tensor of shape [n, {SW}] (played in place), got {got}")
    n = rows.shape[0]
    bound = turn_bound(cfg)
    max_turns = bound if max_turns is None else int(max_turns)
    if not 1 <= max_turns <= bound:
        raise ValueError(f"max_turns must be 1..{bound} for this configuration, got {max_turns}")
    if not 0 <= int(first_seat) < P:
        raise ValueError(f"first_seat must be 0..{P - 1}, got {first_seat}")
    n_counters = L.hb_eval_counters(C.byref(cfg))
    if first_moves is not None:
        _check(first_moves, (n,), torch.int32, "first_moves")
    if done is not None:
        _check(done, (n,), torch.uint8, "done")
    if out is not None:
        final_score, length, counters = out
        _check(final_score, (n,), torch.int8, "out[0] (final_score)")
        _check(length, (n,), torch.int16, "out[1] (length)")
        _check(counters, (n_counters,), torch.int64, "out[2] (counters)")
    if not rows.is_cuda:
        raise K.HbError("the state rows must live on the GPU (there is no CPU path)")
    dev = rows.device
    for name, t in (("first_moves", first_moves), ("done", done)) + ((("out", out[0]), ("out", out[1]), ("out", out[2])) if out else ()):
        if t is not None and t.device != dev:
            raise K.HbError(f"{name} must be on the rows' GPU {dev}, got {t.device}")
    with torch.cuda.device(dev):
        if done is None:
            done = torch.zeros(n, dtype=torch.uint8, device=dev)
        elif out is None:
            done = done.clone()
        if out is None:
            final_score = torch.empty(n, dtype=torch.int8, device=dev)
            length = torch.empty(n, dtype=torch.int16, device=dev)
            counters = torch.empty(n_counters, dtype=torch.int64, device=dev)
        final_score.zero_()
        length.zero_()
        counters.zero_()
        counters[0] = (done < 0x80).sum()
        actions = torch.empty((max_turns, n), dtype=torch.int32, device=dev) if log else None
        return _launch(cfg, rows, teams, seed, first_seat, first_moves, max_turns, first_game_id, done, final_score, length, counters,
                       actions)


def _launch(cfg, rows, teams, seed, first_seat, first_moves, max_turns, first_game_id, done, final_score, length, counters, actions,
            tail=None):
    """hb_rule_playout on prepared buffers (the current device is the rows'). tail: an optional (illegal [1] int64, max_len [1]
    int32) pair to reuse; zeroed here."""
    dev = rows.device
    if tail is None:
        tail = (torch.empty(1, dtype=torch.int64, device=dev), torch.empty(1, dtype=torch.int32, device=dev))
    illegal, max_len = tail
    illegal.zero_()
    max_len.zero_()
    tabs, lens = rule_tables(teams)
    K.check(_fn()(C.byref(cfg), K.dptr(rows), rows.shape[0], int(first_game_id), tabs, lens, int(seed), int(first_seat),
                  K.dptr(first_moves), int(max_turns), K.dptr(done), K.dptr(final_score), K.dptr(length), K.dptr(counters),
                  K.dptr(actions), K.dptr(illegal), K.dptr(max_len), K.current_stream()))
    return PlayoutResult(rows, done, final_score, length, counters, illegal, max_len, actions)


def rule_playout_grouped(cfg, rows, teams, seed, block_games, id_stride=0, first_seat=0, first_moves=None, max_turns=None,
                         first_game_id=0, done=None, log=False, out=None):
    """`rule_playout` for len(teams) blocks of `block_games` games IN PLACE in one launch, one team per block.

    rows [len(teams) * block_games, state_words] int32 holds the blocks one after another; teams: a list of P-tuples of
    `RulebasedAgent` (None: the block is not played). Row r of block b has game id first_game_id + b * id_stride + r: id_stride 0
    for blocks that replay the same deals, block_games for distinct games. first_moves / done / out: as `rule_playout`'s, over all
    the games, with out[2] (counters) [len(teams), hb_eval_counters]; every played block's counters[b, 0] is set to its games to be
    played, a skipped block's row to zero. Returns a `GroupedPlayoutResult` whose block b is `rule_playout`'s result on that
    block alone; nothing is read back to the host."""
    from .evaluate import max_turns as turn_bound
    from .grouped import RuleSets

    L = K.lib()
    cfg = K.HbConfig(cfg.players, cfg.colors, cfg.ranks, cfg.hand_size, cfg.max_info, cfg.max_life, 0)
    if L.hb_config_validate(C.byref(cfg)) != 0:
        raise ValueError(f"invalid configuration {cfg!r}: {L.hb_last_error().decode()}")
    P, SW = cfg.players, L.hb_state_words(C.byref(cfg))
    teams = [None if t is None else tuple(t) for t in teams]
    nb, bg = len(teams), int(block_games)
    if bg < 1:
        raise ValueError(f"block_games must be >= 1, got {block_games}")
    if int(id_stride) not in (0, bg):
        raise ValueError(f"id_stride must be 0 (repeated deals) or block_games = {bg}, got {id_stride}")
    for b, t in enumerate(teams):
        if t is None:
            continue
        if len(t) != P:
            raise ValueError(f"block {b}: one agent per seat: {P} players, {len(t)} agents")
        if not playout_supported(t):
            raise TypeError(f"block {b}: rule_playout_grouped plays RulebasedAgent seats only: " + ", ".join(type(a).__name__ for a in t))
    n = nb * bg
    if n >= 2 ** 31:
        raise ValueError(f"{nb} blocks of {bg} games: the launch takes fewer than 2^31 games, split it")
    if not isinstance(rows, torch.Tensor) or rows.dim() != 2 or rows.shape != (n, SW) or rows.dtype != torch.int32 or not rows.is_contiguous():
        got = f"{rows.dtype} {tuple(rows.shape)}" if isinstance(rows, torch.Tensor) else type(rows).__name__
        raise ValueError(f"rows: expected a contiguous torch.int32 tensor of shape [{nb} * {bg}, {SW}] (played in place), got {got}")
    bound = turn_bound(cfg)
    max_turns = bound if max_turns is None else int(max_turns)
    if not 1 <= max_turns <= bound:
        raise ValueError(f"max_turns must be 1..{bound} for this configuration, got {max_turns}")
    if not 0 <= int(first_seat) < P:
        raise ValueError(f"first_seat must be 0..{P - 1}, got {first_seat}")
    n_counters = L.hb_eval_counters(C.byref(cfg))
    if first_moves is not None:
        _check(first_moves, (n,), torch.int32, "first_moves")
    if done is not None:
        _check(done, (n,), torch.uint8, "done")
    if out is not None:
        final_score, length, counters = out
        _check(final_score, (n,), torch.int8, "out[0] (final_score)")
        _check(length, (n,), torch.int16, "out[1] (length)")
        _check(counters, (nb, n_counters), torch.int64, "out[2] (counters)")
    if not rows.is_cuda:
        raise K.HbError("the state rows must live on the GPU (there is no CPU path)")
    dev = rows.device
    for name, t in (("first_moves", first_moves), ("done", done)) + ((("out", out[0]), ("out", out[1]), ("out", out[2])) if out else ()):
        if t is not None and t.device != dev:
            raise K.HbError(f"{name} must be on the rows' GPU {dev}, got {t.device}")
    agents = []
    for t in teams:
        for a in t or ():
            if not any(a is x for x in agents):
                agents.append(a)
    if not agents:   # no team at all: one empty set, so that the tables exist
        from hanabi_agents.rule_based import RulebasedAgent

        agents = [RulebasedAgent([])]
    sets = RuleSets(agents)
    index = [[-1] * P if t is None else [sets.index(a) for a in t] for t in teams]
    with torch.cuda.device(dev):
        sets.upload(dev)
        team_of_block = torch.tensor(index, dtype=torch.int32, device=dev).reshape(nb, P)
        if done is None:
            done = torch.zeros(n, dtype=torch.uint8, device=dev)
        elif out is None:
            done = done.clone()
        if out is None:
            final_score = torch.empty(n, dtype=torch.int8, device=dev)
            length = torch.empty(n, dtype=torch.int16, device=dev)
            counters = torch.empty((nb, n_counters), dtype=torch.int64, device=dev)
        final_score.zero_()
        length.zero_()
        counters.zero_()
        played = torch.tensor([t is not None for t in teams], dtype=torch.bool, device=dev)
        counters[:, 0] = (done.view(nb, bg) < 0x80).sum(1) * played
        actions = torch.empty((max_turns, n), dtype=torch.int32, device=dev) if log else None
        return _launch_grouped(cfg, rows, nb, bg, id_stride, team_of_block, sets, seed, first_seat, first_moves, max_turns,
                               first_game_id, done, final_score, length, counters, actions)


def _launch_grouped(cfg, rows, n_blocks, block_games, id_stride, team_of_block, sets, seed, first_seat, first_moves, max_turns,
                    first_game_id, done, final_score, length, counters, actions, tail=None):
    """hb_rule_playout_grouped on prepared buffers (the current device is the rows'). team_of_block [n_blocks, P] int32 on the
    device, sets: an uploaded grouped.RuleSets. tail: an optional (illegal [1] int64, max_len [n_blocks] int32) pair to reuse;
    zeroed here."""
    dev = rows.device
    if tail is None:
        tail = (torch.empty(1, dtype=torch.int64, device=dev), torch.empty(n_blocks, dtype=torch.int32, device=dev))
    illegal, max_len = tail
    illegal.zero_()
    max_len.zero_()
    if n_blocks:   # (no blocks: nothing to launch, and empty tensors have no address)
        K.check(_fn_grouped()(C.byref(cfg), K.dptr(rows), int(n_blocks), int(block_games), int(first_game_id), int(id_stride),
                              K.dptr(team_of_block), K.dptr(sets.table_dev), K.dptr(sets.n_rules_dev), len(sets), int(seed),
                              int(first_seat), K.dptr(first_moves), int(max_turns), K.dptr(done), K.dptr(final_score),
                              K.dptr(length), K.dptr(counters), K.dptr(actions), K.dptr(illegal), K.dptr(max_len),
                              K.current_stream()))
    return GroupedPlayoutResult(rows, done, final_score, length, counters, illegal, max_len, actions)
