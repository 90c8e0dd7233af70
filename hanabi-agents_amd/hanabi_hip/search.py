"""Belief-sampled rollout search on top of a fixed blueprint (single-agent SPARTA, Lerer et al. 2020).

    search = RolloutSearch("Hanabi-Full", players=2, replicas=32, seed=1)
    res = search.run(env.export_state(), env.legal, [agent, agent], draw=t)    # value [m, A] of every move, played now
    res.best                                                                   # ... and the best of them

* `Determinizer.sample` (hb_belief_determinize, csrc/belief.hip) re-draws the observing seat's own hand and the undealt deck of
  each state row from what that seat cannot see, `replicas` times, with importance weights: the public-knowledge-plus-card-
  counting belief. It does NOT condition on the partners' policy, so it is not the exact posterior SPARTA's improvement
  guarantee needs; what the search gains over the blueprint is measured, not promised.
* `RolloutSearch.run` lays the replicas out as [m, A, replicas] rollout games — every action of a root starts from the SAME
  replicas (common random numbers) —, forces action a as the first move of block a and then plays every game to the end with
  the blueprint, in lock step, exactly like `Evaluator.run`: `eval_moves` of the seat to act (Philox seed = the search's
  `seed`, draw = turn + 1, rollout game j keyed by game id first_game_id + j), `HanabiEnv.step`, `hb_eval_tally`. The final
  scores are reduced by hb_search_reduce: value = sum w * score / sum w in exact integer sums.
* `RolloutSearch.run_candidates` is the same search over a per-root candidate list [m, C] instead of all A actions
  (hb_search_layout builds the [m, C, replicas] games on the device); with `base_slot` it also gives every candidate's paired
  difference to the baseline's score, replica by replica, and that difference's standard error (hb_search_compare).
  `RolloutSearch.confirm` re-measures {blueprint move, challenger} of every root on fresh replicas: screen, then confirm.
  There is one rollout path: `run` is `run_candidates` with every legal action as the candidate of slot = uid, and both go
  through one cache of rollout envs and buffers keyed (m, C, replicas).
* `ConditionedDeterminizer.sample_history` conditions that belief on the partner's last `depth` moves, kept in a
  `PartnerHistory`: `replicas * oversample` candidates, carried back to every state the partner moved from
  (hb_belief_splice_alive: the cards of that older hand I still hold are a prefix of the candidate's hand, the others are
  public), the partner's `eval_moves` on each with the real turn's Philox keys, and one hb_belief_select_depth: the first
  `replicas` candidates under which it makes the moves it made. It is the one conditioned-sampling path, and `BeliefSample` its
  one result; `.sample` (the last move alone) is the same path on a `LastMove`, the history of one entry, and so is the tuple
  `history=` that run / run_candidates / confirm take. `SearchPlayer(condition=True[, depth=L])` keeps the history itself (2
  players). `PartnerHistory.advance` is one turn of that bookkeeping (own move, re-dealt games, push) in one kernel call
  (hb_belief_history_step): what a training env, whose games end and are dealt anew at different steps, keeps its histories
  with (hanabi_hip.obl, off-belief learning level 2+).
* `epsilon=e` (to `ConditionedDeterminizer.sample` / `sample_history`, `RolloutSearch`, `SearchPlayer(condition=True)`; default
  None: the exact-match filters above, unchanged) reads the partner as epsilon-greedy on its policy: every candidate keeps a
  likelihood (`soft_table`: 1 - e + e / n per reproduced move, e / n per missed one, n = the legal moves of the hypothetical
  state) and the replicas are drawn in proportion to importance weight times likelihood (hb_belief_select_soft). No depth
  fallback; the results carry the candidates' effective sample size.
* `belief_score` (hb_belief_score) scores any of these beliefs against the cards the seat really holds: per slot the weight of
  the replicas that hold the true card, for the whole hand, and next to the card-counting prior, in exact integers; `BeliefScore` forms the hit rates and cross-entropies. `score_belief=True` (`RolloutSearch`,
  `SearchPlayer`; default False: nothing is computed) scores every search's replicas; `SearchPlayer.belief_stats()` gives the means.
* `TrackedBelief` (`SearchPlayer(condition=True, track=True)`, 2 players) tracks the belief across turns instead of rebuilding it:
  the hand samples of my last turn are carried to this one (hb_belief_carry; `belief_carry`), weighed by the one move the
  partner has made since and resampled (hb_belief_select_soft); a root whose samples run out starts over from the conditioned
  belief above.
* `SearchPlayer` is an agent for `Evaluator.run`: the blueprint's move unless the search finds one that is better by more than
  `threshold` and, with `z` / `confirm_replicas`, by more than z standard errors of the paired difference.
* `horizon=H` (`RolloutSearch`, `SearchPlayer`, `SelfPlaySession.search`; default None: rollouts to the end, unchanged) cuts every
  rollout after H turns and values a game still running at its score so far plus the largest legal q of `leaf`'s `eval_q`
  (default: the blueprint's own agent of the seat then to act; "score": nothing), in quarter points with a shared dither
  (`search_leaf`, `leaf_dither`), in the int8 buffer the two reduce kernels already read.
* The kernels' numpy restatements (`belief_select_soft_ref`, `belief_carry_ref`, `belief_score_ref`) live in hanabi_hip.belief_ref,
  with the leaf step's specification (`search_leaf_ref`, `leaf_dither_ref`).

Colour-shuffled envs are refused: the rollout env's game ids would draw other permutations than the source's.
"""
import ctypes as C
import weakref
from typing import NamedTuple, Optional

import torch

from . import _capi as K
from .encode import encode_rows
from .env import HanabiEnv
from .evaluate import eval_config, max_turns
from .playout import _launch as playout_launch, playout_supported


def _rows(rows, words, device=None):
    r = torch.as_tensor(rows)
    r = r.to(device=device if device is not None else r.device, dtype=torch.int32).contiguous()
    if r.dim() != 2 or r.shape[1] != words:
        raise ValueError(f"state rows have shape [m, {words}], got {tuple(r.shape)}")
    if not r.is_cuda:
        raise K.HbError("the state rows must live on the GPU (there is no CPU path)")
    return r


def _bufs(dev, given, *specs):
    """One tensor per (shape, dtype) of `specs`: the caller's `given` ones, each checked (shape, dtype, contiguous), or, with
    `given` None, new ones on `dev`. The kernels index what they are handed by these shapes alone."""
    if given is None:
        return tuple(torch.empty(shape, dtype=dtype, device=dev) for shape, dtype in specs)
    assert len(given) == len(specs)
    for t, (shape, dtype) in zip(given, specs):
        assert t.shape == tuple(shape) and t.dtype == dtype and t.is_contiguous(), \
            f"expected a contiguous {dtype} tensor of shape {tuple(shape)}, got {t.dtype} {tuple(t.shape)}"
    return tuple(given)


def _reads(dev, tensors, *specs, one_gpu=None):
    """_bufs' check of the tensors a belief kernel reads; the last may be None (an optional mask) and is then left out. one_gpu:
    the name of a kernel whose wrapper also refuses a tensor that is not on the GPU `dev`."""
    if tensors[-1] is None:
        tensors, specs = tensors[:-1], specs[:-1]
    _bufs(dev, tensors, *specs)
    if one_gpu is not None:
        for t in tensors:
            if not t.is_cuda or t.device != dev:
                raise K.HbError(f"{one_gpu} reads tensors of one GPU (there is no CPU path)")


def _ask(agent, env, seed, draw, out, scratch):
    """agent.eval_moves on the env's current states (observed, for an agent that reads observations) -> out. scratch: agent ->
    the buffers its eval_moves writes."""
    if agent.requires_vectorized_observation():
        agent.eval_moves((env, (env.net_obs, env.legal)), seed, draw, out, scratch=scratch.setdefault(agent, {}))
    else:
        agent.eval_moves(env, seed, draw, out)


class Determinizer:
    """hb_belief_determinize on torch tensors; see the module docstring and include/hanabi_hip.h."""

    def __init__(self, game="Hanabi-Full", players=2, config=None):
        self.cfg = eval_config(game, players, config)
        self.players = self.cfg.players
        self.state_words = K.lib().hb_state_words(C.byref(self.cfg))

    def sample(self, rows, seat=-1, replicas=32, seed=1, draw=0, first_row_id=0, out=None):
        """rows [m, state_words] int32 (device) -> (rows_out [m * replicas, state_words] int32, weights [m * replicas] int64).
        Row i * replicas + r is replica r of source row i; weight 0 marks a dead replica (an unchanged copy). `out`: an
        optional (rows_out, weights_u32) pair of buffers to write into (weights int32 holding the u32 bits)."""
        r = _rows(rows, self.state_words)
        m, replicas = r.shape[0], int(replicas)
        n = m * max(replicas, 0)   # (a negative count is the kernel's to refuse)
        rows_out, w = _bufs(r.device, out, ((n, self.state_words), torch.int32), ((n,), torch.int32))
        with torch.cuda.device(r.device):
            K.check(K.lib().hb_belief_determinize(C.byref(self.cfg), K.dptr(r), m, int(seat), replicas, int(seed), int(draw),
                                                  int(first_row_id), K.dptr(rows_out), K.dptr(w), K.current_stream()))
        if out is not None:
            return rows_out, w
        return rows_out, w.long() & 0xFFFFFFFF


def search_reduce(scores, weights, legal):
    """hb_search_reduce: scores [m, A, R] int8, weights [m, R] (u32 bits in int32), legal [m, A] int8 ->
    (value [m, A] f32, wsum [m, A] int64, n_live [m, A] int32, best [m] int32)."""
    (m, A, R), dev = scores.shape, scores.device
    _bufs(dev, (scores, weights, legal), ((m, A, R), torch.int8), ((m, R), torch.int32), ((m, A), torch.int8))
    value, wsum, n_live, best = _bufs(dev, None, ((m, A), torch.float32), ((m, A), torch.int64), ((m, A), torch.int32),
                                      ((m,), torch.int32))
    with torch.cuda.device(dev):
        K.check(K.lib().hb_search_reduce(K.dptr(scores), K.dptr(weights), K.dptr(legal), m, A, R, K.dptr(value), K.dptr(wsum),
                                         K.dptr(n_live), K.dptr(best), K.current_stream()))
    return value, wsum, n_live, best


def search_layout(cfg, det_rows, weights, cand, filler, replicas, out=None):
    """hb_search_layout: det_rows [m * R, SW] int32, weights [m * R] (u32 bits in int32), cand [m, C] int32 (uid, or -1: no
    candidate in this slot), filler [m] int32 -> (rows [m * C * R, SW] int32, forced [m * C * R] int32, done [m * C * R] uint8,
    n_played [m] int32). `out`: an optional tuple of these four buffers to write into."""
    m, Cn = cand.shape
    R, SW = int(replicas), det_rows.shape[1]
    n, dev = m * Cn * R, det_rows.device
    _bufs(dev, (det_rows, weights, cand, filler), ((m * R, SW), torch.int32), ((m * R,), torch.int32), ((m, Cn), torch.int32),
          ((m,), torch.int32))
    rows, forced, done, n_played = _bufs(dev, out, ((n, SW), torch.int32), ((n,), torch.int32), ((n,), torch.uint8),
                                         ((m,), torch.int32))
    with torch.cuda.device(dev):
        K.check(K.lib().hb_search_layout(C.byref(cfg), K.dptr(det_rows), K.dptr(weights), K.dptr(cand), K.dptr(filler), m, Cn, R,
                                         K.dptr(rows), K.dptr(forced), K.dptr(done), K.dptr(n_played), K.current_stream()))
    return rows, forced, done, n_played


def search_compare(scores, weights, cand, base_slot):
    """hb_search_compare: scores [m, C, R] int8, weights [m, R] (u32 bits in int32), cand [m, C] int32, base_slot [m] int32 ->
    (diff [m, C] f64, se [m, C] f64, n_pair [m] int32): every slot's paired difference to the base slot and its standard error."""
    (m, Cn, R), dev = scores.shape, scores.device
    _bufs(dev, (scores, weights, cand, base_slot), ((m, Cn, R), torch.int8), ((m, R), torch.int32), ((m, Cn), torch.int32),
          ((m,), torch.int32))
    diff, se, n_pair = _bufs(dev, None, ((m, Cn), torch.float64), ((m, Cn), torch.float64), ((m,), torch.int32))
    with torch.cuda.device(dev):
        K.check(K.lib().hb_search_compare(K.dptr(scores), K.dptr(weights), K.dptr(cand), K.dptr(base_slot), m, Cn, R, K.dptr(diff),
                                          K.dptr(se), K.dptr(n_pair), K.current_stream()))
    return diff, se, n_pair


LEAF_SCALE = 4   # a depth-limited search keeps its leaf values in quarter points, in the int8 buffer the reduce kernels read


def _mix32(x):
    """belief_ref._mix32_np on int64 tensors below 2^32 (no intermediate reaches 2^49: nothing wraps)."""
    def mul(x, c):
        return (x * (c & 0xFFFF) + (((x * (c >> 16)) & 0xFFFF) << 16)) & 0xFFFFFFFF

    x = x ^ (x >> 16)
    x = mul(x, 0x7FEB352D)
    x = x ^ (x >> 15)
    x = mul(x, 0x846CA68B)
    return x ^ (x >> 16)


def leaf_dither(seed, draw, first_row_id, m, replicas, device=None):
    """belief_ref.leaf_dither_ref in torch int64 ops: u [m, replicas] float64 in [0, 1), a multiple of 2^-24, a pure function of
    (seed, draw, first_row_id + i * replicas + r). The four words of seed and draw are hashed on the host."""
    m, R = int(m), int(replicas)
    seed, draw = int(seed) & _M64, int(draw) & _M64
    h = 0x9E3779B9
    for v in (seed & 0xFFFFFFFF, seed >> 32, draw & 0xFFFFFFFF, draw >> 32):
        h = _mix32(h ^ v)
    rid = torch.arange(m * R, dtype=torch.int64, device=device).view(m, R) + int(first_row_id)
    h = _mix32((rid & 0xFFFFFFFF) ^ h)
    h = _mix32(h ^ ((rid >> 32) & 0xFFFFFFFF))
    return (h >> 8).double() * 2.0 ** -24


def search_leaf(done, final_score, score, q, legal, u, max_score, out=None):
    """belief_ref.search_leaf_ref in torch, the same bits on any device: done [m, C, R] uint8, final_score and score [m, C, R]
    int8, q [m, C, R, A] float32 (None: v = 0), legal [m, C, R, A] int8, u [m, R] float64 -> leaf4 [m, C, R] int8 (`out`, when
    given). Elementwise ops, and one max over the A entries of a row, which no order of evaluation changes."""
    m, Cn, R = done.shape
    x = score.double()
    if q is not None:
        ok = (legal != 0) & torch.isfinite(q)
        v = torch.where(ok, q, float("-inf")).amax(-1)
        x = x + torch.where(ok.any(-1), v, 0.0).double()
    run = torch.floor(LEAF_SCALE * x + u.view(m, 1, R)).clamp(0, LEAF_SCALE * int(max_score))
    leaf4 = torch.where((done & 0x80) != 0, LEAF_SCALE * final_score.long(), run.long()).to(torch.int8)
    return leaf4 if out is None else out.copy_(leaf4)


def belief_splice(cfg, prev_rows, det_rows, seat, n_cand, out=None):
    """hb_belief_splice (belief_splice_alive with every slot alive): prev_rows [m, SW] int32, det_rows [m * K, SW] int32
    (candidate (i, k) = row i * K + k) -> rows [K, m, SW] int32, candidate-major: slab k = prev_rows with word 10 + seat of every
    row taken from candidate (i, k)."""
    m, SW = prev_rows.shape
    Kn, dev = int(n_cand), prev_rows.device
    _reads(dev, (prev_rows, det_rows), ((m, SW), torch.int32), ((m * Kn, SW), torch.int32))
    out, = _bufs(dev, None if out is None else (out,), ((max(Kn, 0), m, SW), torch.int32))
    with torch.cuda.device(dev):
        K.check(K.lib().hb_belief_splice(C.byref(cfg), K.dptr(prev_rows), K.dptr(det_rows), m, int(seat), Kn, K.dptr(out),
                                         K.current_stream()))
    return out


def belief_select(cfg, src_rows, det_rows, weights, hyp_moves, actual, valid, replicas, out=None):
    """hb_belief_select (belief_select_depth at depth 1): src_rows [m, SW] int32, det_rows [m * K, SW] int32, weights [m * K]
    (u32 bits in int32), hyp_moves [K, m] int32, actual [m] int32, valid [m] uint8 or None -> (rows [m * R, SW] int32, weights
    [m * R] int32, n_surv [m] int32, fallback [m] uint8). `out`: an optional tuple of these four buffers to write into."""
    m, SW = src_rows.shape
    Kn, R, dev = hyp_moves.shape[0], int(replicas), src_rows.device
    _reads(dev, (src_rows, det_rows, weights, hyp_moves, actual, valid), ((m, SW), torch.int32), ((m * Kn, SW), torch.int32),
           ((m * Kn,), torch.int32), ((Kn, m), torch.int32), ((m,), torch.int32), ((m,), torch.uint8))
    n = m * max(R, 0)
    rows, w, n_surv, fallback = _bufs(dev, out, ((n, SW), torch.int32), ((n,), torch.int32), ((m,), torch.int32), ((m,), torch.uint8))
    with torch.cuda.device(dev):
        K.check(K.lib().hb_belief_select(C.byref(cfg), K.dptr(src_rows), K.dptr(det_rows), K.dptr(weights), K.dptr(hyp_moves),
                                         K.dptr(actual), K.dptr(valid), m, Kn, R, K.dptr(rows), K.dptr(w), K.dptr(n_surv),
                                         K.dptr(fallback), K.current_stream()))
    return rows, w, n_surv, fallback


def belief_splice_alive(cfg, prev_rows, alive, det_rows, seat, n_cand, out=None):
    """hb_belief_splice_alive: prev_rows [m, SW] int32 states the partner moved from, det_rows [m * K, SW] int32 (candidate (i, k)
    = row i * K + k); alive [m] uint8 (or None: every slot alive) marks the slots of `seat`'s hand in prev_rows whose card is
    still in its hand now. -> rows [K, m, SW] int32, candidate-major: slab k = prev_rows with the alive slots of word 10 + seat
    taken from candidate (i, k)'s hand, in order."""
    m, SW = prev_rows.shape
    Kn, dev = int(n_cand), prev_rows.device
    _reads(dev, (prev_rows, det_rows, alive), ((m, SW), torch.int32), ((m * Kn, SW), torch.int32), ((m,), torch.uint8))
    out, = _bufs(dev, None if out is None else (out,), ((max(Kn, 0), m, SW), torch.int32))
    with torch.cuda.device(dev):
        K.check(K.lib().hb_belief_splice_alive(C.byref(cfg), K.dptr(prev_rows), K.dptr(alive), K.dptr(det_rows), m, int(seat), Kn,
                                               K.dptr(out), K.current_stream()))
    return out


def belief_select_depth(cfg, src_rows, det_rows, weights, hyp_moves, actual, valid, replicas, out=None):
    """hb_belief_select_depth: src_rows [m, SW] int32, det_rows [m * K, SW] int32, weights [m * K] (u32 bits in int32), hyp_moves
    [D, K, m] int32, actual [D, m] int32, valid [D, m] uint8 or None (entry 0 = the most recent move) -> (rows [m * R, SW] int32,
    weights [m * R] int32, n_surv [D, m] int32, depth_used [m] int32, fallback [m] uint8). `out`: an optional tuple of these five
    buffers to write into."""
    m, SW = src_rows.shape
    if hyp_moves.dim() != 3:
        raise ValueError(f"hyp_moves has shape [depth, K, m], got {tuple(hyp_moves.shape)}")
    D, Kn, R, dev = hyp_moves.shape[0], hyp_moves.shape[1], int(replicas), src_rows.device
    _reads(dev, (src_rows, det_rows, weights, hyp_moves, actual, valid), ((m, SW), torch.int32), ((m * Kn, SW), torch.int32),
           ((m * Kn,), torch.int32), ((D, Kn, m), torch.int32), ((D, m), torch.int32), ((D, m), torch.uint8))
    n = m * max(R, 0)
    rows, w, n_surv, depth_used, fallback = _bufs(dev, out, ((n, SW), torch.int32), ((n,), torch.int32), ((D, m), torch.int32),
                                                  ((m,), torch.int32), ((m,), torch.uint8))
    with torch.cuda.device(dev):
        K.check(K.lib().hb_belief_select_depth(C.byref(cfg), K.dptr(src_rows), K.dptr(det_rows), K.dptr(weights), K.dptr(hyp_moves),
                                               K.dptr(actual), K.dptr(valid), m, Kn, R, D, K.dptr(rows), K.dptr(w), K.dptr(n_surv),
                                               K.dptr(depth_used), K.dptr(fallback), K.current_stream()))
    return rows, w, n_surv, depth_used, fallback


MAX_DEPTH = 8   # hb_belief_select_depth's
MAX_SOFT_CANDIDATES = 4096   # hb_belief_select_soft's: the 64-bit sum of the quantised weights


def soft_table(epsilon, n_actions, device=None):
    """The likelihood of an epsilon-greedy partner's move: [2, A + 1] float64, indexed by the number n of legal moves;
    table[0][n] = 1 - eps + eps / n (the move is the policy's: kept, or drawn by the uniform part), table[1][n] = eps / n (it is
    not: the uniform part alone); column 0 is 0. epsilon in [1e-6, 1]: at 0 a single off-policy move would leave no candidate, which is
    the exact-match filter (epsilon=None)."""
    eps, A = float(epsilon), int(n_actions)
    if not 1e-6 <= eps <= 1.0:
        raise ValueError(f"epsilon must be in [1e-6, 1], got {epsilon}")
    if A < 1:
        raise ValueError(f"n_actions must be >= 1, got {n_actions}")
    # (host floats: one correctly rounded division per entry)
    t = torch.tensor([[0.0] + [1.0 - eps + eps / n for n in range(1, A + 1)], [0.0] + [eps / n for n in range(1, A + 1)]],
                     dtype=torch.float64)
    return t if device is None else t.to(device)


def belief_select_soft(cfg, src_rows, det_rows, weights, hyp_moves, n_legal, actual, valid, p_table, replicas, seed, draw,
                       first_row_id=0, out=None):
    """hb_belief_select_soft: belief_select_depth's inputs, with n_legal [D, K, m] int32 (the legal moves of the hypothetical state
    each hypothetical move was computed on) and p_table [2, A + 1] float64 (soft_table), read as a likelihood: `replicas`
    candidates per root drawn with (seed, draw, row id first_row_id + i) in proportion to importance weight times likelihood ->
    (rows [m * R, SW] int32, weights [m * R] int32 (1: drawn, 0: dead), n_surv [D, m] int32, depth_used [m] int32, fallback [m]
    uint8, ess [m] float32). `out`: an optional tuple of these six buffers to write into."""
    m, SW = src_rows.shape
    if hyp_moves.dim() != 3:
        raise ValueError(f"hyp_moves has shape [depth, K, m], got {tuple(hyp_moves.shape)}")
    D, Kn, R, dev = hyp_moves.shape[0], hyp_moves.shape[1], int(replicas), src_rows.device
    if not 1 <= D <= MAX_DEPTH:
        raise ValueError(f"depth must be in 1..{MAX_DEPTH}, got {D}")
    if not 1 <= Kn <= MAX_SOFT_CANDIDATES:
        raise ValueError(f"the soft filter takes 1..{MAX_SOFT_CANDIDATES} candidates per root, got {Kn}")
    A = K.lib().hb_num_actions(C.byref(cfg))
    _reads(dev, (src_rows, det_rows, weights, hyp_moves, n_legal, actual, p_table, valid), ((m, SW), torch.int32),
           ((m * Kn, SW), torch.int32), ((m * Kn,), torch.int32), ((D, Kn, m), torch.int32), ((D, Kn, m), torch.int32),
           ((D, m), torch.int32), ((2, A + 1), torch.float64), ((D, m), torch.uint8), one_gpu="hb_belief_select_soft")
    n = m * max(R, 0)
    rows, w, n_surv, depth_used, fallback, ess = _bufs(dev, out, ((n, SW), torch.int32), ((n,), torch.int32), ((D, m), torch.int32),
                                                       ((m,), torch.int32), ((m,), torch.uint8), ((m,), torch.float32))
    with torch.cuda.device(dev):
        K.check(K.lib().hb_belief_select_soft(C.byref(cfg), K.dptr(src_rows), K.dptr(det_rows), K.dptr(weights), K.dptr(hyp_moves),
                                              K.dptr(n_legal), K.dptr(actual), K.dptr(valid), K.dptr(p_table), m, Kn, R, D,
                                              int(seed) & _M64, int(draw) & _M64, int(first_row_id), K.dptr(rows), K.dptr(w),
                                              K.dptr(n_surv), K.dptr(depth_used), K.dptr(fallback), K.dptr(ess), K.current_stream()))
    return rows, w, n_surv, depth_used, fallback, ess


_M64 = 0xFFFFFFFFFFFFFFFF


def belief_carry(cfg, cur_rows, old_rows, old_weights, own_slot, revealed, drew, seat, n_particles, seed, draw, first_row_id=0,
                 out=None):
    """hb_belief_carry: the hand samples of my previous turn carried to my present one (include/hanabi_hip.h has the rule).
    cur_rows [m, SW] int32 the states now (`seat`, the observer, to act), old_rows [m * K, SW] int32 / old_weights [m * K] (u32
    bits in int32) the K = n_particles particles of each root at my previous turn (only the observer's hand word is read, and
    whether the weight is 0), own_slot [m] int32 the slot I played or discarded then (-1: a hint), revealed [m] int32 the card
    that turned face up (-1: none), drew [m] int32 the card the partner has visibly drawn since (-1: none) -> (rows [m * K, SW]
    int32, weights [m * K] int32). `out`: an optional pair of these two buffers to write into. GPU only."""
    cur = torch.as_tensor(cur_rows)
    if cur.dim() != 2:
        raise ValueError(f"cur_rows has shape [m, state_words], got {tuple(cur.shape)}")
    m, SW = cur.shape
    Kn, dev = int(n_particles), cur.device
    if Kn < 1:
        raise ValueError(f"n_particles must be >= 1, got {n_particles}")
    if not 0 <= int(seat) < cfg.players:
        raise ValueError(f"seat {seat} out of range for {cfg.players} players (the observer, who is to act)")
    n = m * Kn
    _reads(dev, (cur, old_rows, old_weights, own_slot, revealed, drew), ((m, SW), torch.int32), ((n, SW), torch.int32), ((n,), torch.int32),
           ((m,), torch.int32), ((m,), torch.int32), ((m,), torch.int32), one_gpu="hb_belief_carry")
    rows, w = _bufs(dev, out, ((n, SW), torch.int32), ((n,), torch.int32))
    with torch.cuda.device(dev):
        K.check(K.lib().hb_belief_carry(C.byref(cfg), K.dptr(cur), K.dptr(old_rows), K.dptr(old_weights), K.dptr(own_slot),
                                        K.dptr(revealed), K.dptr(drew), m, int(seat), Kn, int(seed) & _M64, int(draw) & _M64,
                                        int(first_row_id), K.dptr(rows), K.dptr(w), K.current_stream()))
    return rows, w


def belief_score(cfg, true_rows, det_rows, weights, seat, replicas, counts=False, out=None):
    """hb_belief_score: true_rows [m, SW] int32 the real states, det_rows [m * R, SW] int32 and weights [m * R] (u32 bits in
    int32) replicas of them from any of the samplers (replica r of root i = row i * R + r), seat (-1: each true row's current
    player) -> `BeliefScore`: what the belief gives the cards the seat really holds, next to the card-counting prior, in exact
    integers (include/hanabi_hip.h). counts=True also fills the [m, H, NC] per-card tally. `out`: an optional tuple of the
    buffers (truth, hit, joint, wsum, n_live, prior[, counts]) to write into. GPU only."""
    m, SW = true_rows.shape
    R, dev = int(replicas), true_rows.device
    H, NC, n = cfg.hand_size, cfg.colors * cfg.ranks, m * max(int(replicas), 0)
    _reads(dev, (true_rows, det_rows, weights), ((m, SW), torch.int32), ((n, SW), torch.int32), ((n,), torch.int32),
           one_gpu="hb_belief_score")
    specs = (((m, H), torch.int8), ((m, H), torch.int64), ((m,), torch.int64), ((m,), torch.int64), ((m,), torch.int32),
             ((m, H, NC), torch.int8)) + ((((m, H, NC), torch.int64),) if counts else ())
    bufs = _bufs(dev, out, *specs)
    truth, hit, joint, wsum, n_live, prior = bufs[:6]
    tally = bufs[6] if counts else None
    with torch.cuda.device(dev):
        K.check(K.lib().hb_belief_score(C.byref(cfg), K.dptr(true_rows), K.dptr(det_rows), K.dptr(weights), m, int(seat), R,
                                        K.dptr(truth), K.dptr(hit), K.dptr(joint), K.dptr(wsum), K.dptr(n_live), K.dptr(tally),
                                        K.dptr(prior), K.current_stream()))
    return BeliefScore(truth, hit, joint, wsum, n_live, prior, tally)


def belief_figures(sums):
    """The means of a `BeliefScore.sums()` tensor (or of a sum of several; None: nothing yet) as plain numbers: `cards` (the
    scored (root, slot) pairs), `roots`, `hit_rate`, `prior_rate`, `joint_rate`, `cross_entropy`, `prior_cross_entropy` and
    `by_slot`, the same five per-card figures as lists over the slot's age (slot 0 = the oldest card). A mean over nothing is 0.0.
    One device-to-host copy."""
    rows = [[0.0]] * len(BeliefScore.SUMS) if sums is None else sums.tolist()
    mean = lambda total, count: total / count if count else 0.0
    cards, hit, prior, ce, pce, roots, joint = rows
    n = sum(cards)
    names = ("hit_rate", "prior_rate", "cross_entropy", "prior_cross_entropy")
    out = dict(cards=int(n), roots=int(roots[0]), joint_rate=mean(joint[0], roots[0]))
    out.update({k: mean(sum(v), n) for k, v in zip(names, (hit, prior, ce, pce))})
    slots = range(0 if sums is None else len(cards))
    out["by_slot"] = dict(cards=[int(cards[s]) for s in slots],
                          **{k: [mean(v[s], cards[s]) for s in slots] for k, v in zip(names, (hit, prior, ce, pce))})
    return out


def belief_stats_of(sums, split=False):
    """SearchPlayer.belief_stats() of a `SearchPlayer.belief_sums()` tensor (or of a sum of several players'; None: zeros):
    belief_figures over all roots and, with `split`, also over the `conditioned` and the `unconditioned` ones."""
    out = belief_figures(None if sums is None else sums.sum(0))
    if split:
        for j, name in enumerate(("conditioned", "unconditioned")):
            out[name] = belief_figures(None if sums is None else sums[j])
    return out


class BeliefScore:
    """What a sampled belief gives the cards a seat really holds (hb_belief_score; `belief_score`, or `belief_score_ref`'s arrays).

        truth  [m, H] int8       the card id in slot s of the true hand (-1: no such slot, or the root is not scored)
        hit    [m, H] int64      the weight of the replicas that hold that card in that slot
        joint  [m] int64         the weight of the replicas that hold the whole true hand
        wsum   [m] int64         the weight of all replicas; n_live [m] int32 the replicas of weight != 0
        prior  [m, H, NC] int8   card counting alone: the copies of card c the seat cannot see, where slot s's hints allow c
        counts [m, H, NC] int64  the weight of the replicas that hold card c in slot s (None unless asked for)

    Everything the kernel writes is an integer; the ratios are formed here, in float64, on the tensors' device. `scored` [m] bool:
    the root is running (it has a slot 0) and wsum > 0; only scored roots, and of those only the slots that have a truth, enter
    any figure. A sampled belief gives a card it never drew no mass at all, so the cross-entropy is taken of the mixture
    p = (1 - l) * hit / wsum + l * prior[truth] / sum_c prior (see cross_entropy)."""

    SUMS = ("cards", "hit", "prior", "ce", "prior_ce", "roots", "joint")

    def __init__(self, truth, hit, joint, wsum, n_live, prior, counts=None):
        t = torch.as_tensor
        self.truth, self.hit, self.joint, self.wsum, self.n_live, self.prior = t(truth), t(hit), t(joint), t(wsum), t(n_live), t(prior)
        self.counts = None if counts is None else t(counts)

    @property
    def scored(self):
        return (self.truth[:, 0] >= 0) & (self.wsum > 0)

    def sums(self, smoothing=None, where=None):
        """The raw sums behind every figure, [len(SUMS), H] float64 on the tensors' device, one column per slot: `cards` (scored
        slots with a truth), `hit` (sum of hit / wsum), `prior` (sum of prior[truth] / sum_c prior), `ce` and `prior_ce` (sums of
        -log p, `smoothing` as in cross_entropy), and in column 0 `roots` (scored roots) and `joint` (sum of joint / wsum).
        where: an optional [m] bool mask of the roots to count. No host synchronisation: sums of several calls add up, and
        `belief_figures` turns the total into means."""
        scored = self.scored if where is None else self.scored & where
        has = scored.unsqueeze(1) & (self.truth >= 0)
        NC = self.prior.shape[2]
        ws = self.wsum.clamp(min=1).double().unsqueeze(1)
        q = self.hit.double() / ws
        at = self.prior.gather(2, self.truth.long().clamp(0, NC - 1).unsqueeze(2)).squeeze(2).double()
        pr = torch.where(self.truth < NC, at, 0.0) / self.prior.sum(2).clamp(min=1).double()
        lam = 1.0 / (self.n_live.double().unsqueeze(1) + 1.0) if smoothing is None else float(smoothing)
        zero = torch.zeros((), dtype=torch.float64, device=q.device)
        nll = lambda p: torch.where(has, -torch.log(p), zero).sum(0)
        first = torch.zeros_like(q[0])
        first[0] = 1.0
        return torch.stack([has.sum(0).double(), torch.where(has, q, zero).sum(0), torch.where(has, pr, zero).sum(0),
                            nll((1.0 - lam) * q + lam * pr), nll(pr), first * scored.sum(),
                            first * torch.where(scored, self.joint.double() / ws.squeeze(1), zero).sum()])

    def figures(self, smoothing=None, where=None):
        """belief_figures(self.sums(...)): every figure at once."""
        return belief_figures(self.sums(smoothing, where))

    def hit_rate(self):
        """The mean over the scored roots' slots of hit / wsum: the mass the belief puts on the true card."""
        return self.figures()["hit_rate"]

    def prior_rate(self):
        """The same mean of prior[truth] / sum_c prior: the mass card counting alone puts on it."""
        return self.figures()["prior_rate"]

    def joint_rate(self):
        """The mean over the scored roots of joint / wsum: the mass on the whole true hand."""
        return self.figures()["joint_rate"]

    def cross_entropy(self, smoothing=None):
        """Minus the mean natural log of p = (1 - l) * hit / wsum + l * prior[truth] / sum_c prior over the scored roots' slots;
        l = `smoothing`, or 1 / (n_live + 1) per root when None (one pseudo-replica drawn from the prior). The mixture is what
        keeps the figure finite: a sampled belief gives no mass to a card it never drew. On states reached by play the true
        card is in the pool and plausible, so prior[truth] >= 1 and every p > 0; on edited rows (a truth the hints exclude, or
        smoothing=0 with a missed card) the result may be inf."""
        return self.figures(smoothing)["cross_entropy"]

    def prior_cross_entropy(self):
        """cross_entropy at l = 1: the card-counting baseline's own figure."""
        return self.figures()["prior_cross_entropy"]

    def by_slot(self, smoothing=None):
        """The per-card figures by the slot's age (slot 0 = the oldest card): belief_figures' `by_slot`."""
        return self.figures(smoothing)["by_slot"]


def running(rows):
    """[m] bool: the game of each state row has not ended (the status bits of word 0 are 0)."""
    return ((rows[:, 0] >> 19) & 3) == 0


def current_player(rows):
    """[m]: the seat to act in each state row (word 0)."""
    return (rows[:, 0] >> 13) & 7


def last_move_uid(cfg, rows):
    """The uid (App. A.2 order, in the frame of the seat that made it) of the last move recorded in word 2 of each state row
    (DESIGN.md section 3): [m] int32, -1 where the word's valid bit is 0 (no move yet in this deal)."""
    r = torch.as_tensor(rows)
    if r.dim() != 2 or r.shape[1] < 3:
        raise ValueError(f"state rows have shape [m, state_words], got {tuple(r.shape)}")
    w2 = r[:, 2].long() & 0xFFFFFFFF
    H, P, Cn, Rn = cfg.hand_size, cfg.players, cfg.colors, cfg.ranks
    kind, idx, off = (w2 >> 4) & 3, (w2 >> 6) & 7, ((w2 >> 9) & 7) - 1
    col, rank = (w2 >> 12) & 7, (w2 >> 15) & 7
    uid = torch.where(kind == 1, idx, torch.where(kind == 0, H + idx, torch.where(
        kind == 2, 2 * H + off * Cn + col, 2 * H + (P - 1) * Cn + off * Rn + rank)))
    return torch.where((w2 & 1) != 0, uid, -1).to(torch.int32)


class LastMove:
    """The history (prev_rows, partner_seed, partner_draw, first_game_id[, valid]) as a history of one entry: it presents what
    `ConditionedDeterminizer.sample_history` reads from a `PartnerHistory`, for the partner's last move alone.

        prev_rows [1, m, SW] int32   the states the partner moved from
        valid     [1, m] uint8       0: no usable previous state; None: every root has one
        draws     [partner_draw]     the Philox draw of that turn; depth = filled = 1
        alive     None               every card I held then I hold now: the splice takes a null mask
        moves     None               the move is the last one the sampled rows record: last_move_uid(cfg, rows), at call time

    prev_rows [m, words] and valid [m] (or None) are checked and moved to `device`. Unpacks as the tuple it was made from."""

    depth = filled = 1
    alive = moves = None

    def __init__(self, prev_rows, partner_seed, partner_draw, first_game_id, valid=None, *, m, words, device):
        prev = torch.as_tensor(prev_rows)
        if prev.dim() != 2 or tuple(prev.shape) != (m, words):
            raise ValueError(f"history's previous rows have shape ({m}, {words}), got {tuple(prev.shape)}")
        self.m, self.state_words = m, words
        self.prev_rows = prev.to(device=device, dtype=torch.int32).contiguous().view(1, m, words)
        self.valid = None
        if valid is not None:
            valid = torch.as_tensor(valid)
            if tuple(valid.shape) != (m,):
                raise ValueError(f"history's valid mask has shape ({m},), got {tuple(valid.shape)}")
            self.valid = (valid.to(device) != 0).to(torch.uint8).contiguous().view(1, m)
        self.partner_seed, self.partner_draw, self.first_game_id = int(partner_seed), int(partner_draw), int(first_game_id)
        self.draws = [self.partner_draw]

    def __iter__(self):
        return iter((self.prev_rows[0], self.partner_seed, self.partner_draw, self.first_game_id,
                     None if self.valid is None else self.valid[0]))

    def __getitem__(self, i):
        return tuple(self)[i]


def _history(history, m, words, dev):
    """(prev_rows, partner_seed, partner_draw, first_game_id[, valid]) checked -> the `LastMove` of it, tensors on the device."""
    if not isinstance(history, (tuple, list)) or len(history) not in (4, 5):
        raise ValueError("history is (prev_rows, partner_seed, partner_draw, first_game_id[, valid])")
    return LastMove(*history, m=m, words=words, device=dev)


class PartnerHistory:
    """The partner's last `depth` moves as one observer sees them, newest first:

        prev_rows [depth, m, SW] int32   the states the partner moved from
        moves     [depth, m] int32       the uid it played (last_move_uid of the state after it)
        draws     [depth] ints           the Philox draw of that turn (a list on the host)
        alive     [depth, m] uint8       bit s: the card in slot s of MY hand in prev_rows[d] is still in my hand now
        valid     [depth, m] uint8       0: no usable entry (the entries behind it are then not used either)

    own_move() before I play, push() once the partner has answered. partner_seed / first_game_id: what the partner's eval_moves
    was keyed with in the real game; RolloutSearch hands them to ConditionedDeterminizer.sample_history. The tensors live on
    `device` (any torch device: the mask rule is plain torch); `filled` counts the entries pushed since the last clear()."""

    def __init__(self, cfg, m, depth, device, partner_seed=0, first_game_id=0):
        self.cfg, self.m, self.depth = cfg, int(m), int(depth)
        if not 1 <= self.depth <= MAX_DEPTH:
            raise ValueError(f"depth must be in 1..{MAX_DEPTH}, got {depth}")
        if self.m < 1:
            raise ValueError(f"m must be >= 1, got {m}")
        self.state_words = K.lib().hb_state_words(C.byref(cfg))
        self.partner_seed, self.first_game_id = int(partner_seed), int(first_game_id)
        D = self.depth
        self.prev_rows = torch.zeros((D, self.m, self.state_words), dtype=torch.int32, device=device)
        self.moves = torch.zeros((D, self.m), dtype=torch.int32, device=device)
        self.alive = torch.zeros((D, self.m), dtype=torch.uint8, device=device)
        self.valid = torch.zeros((D, self.m), dtype=torch.uint8, device=device)
        self._slot = torch.arange(5, device=device).view(1, 1, 5)
        self.clear()

    def clear(self):
        self.valid.zero_()
        self.alive.zero_()
        self.draws, self.filled = [0] * self.depth, 0

    def own_move(self, uids):
        """I am about to play uids [m]: a play or discard of slot s takes the s-th card I still hold out of every entry (the
        s-th set bit of its alive mask; a card drawn after the entry — s >= popcount — leaves it unchanged). Hints change
        nothing."""
        H = self.cfg.hand_size
        u = torch.as_tensor(uids).to(self.alive.device).long()
        if tuple(u.shape) != (self.m,):
            raise ValueError(f"uids has shape ({self.m},), got {tuple(u.shape)}")
        card = ((u >= 0) & (u < 2 * H)).view(1, self.m, 1)
        s = (u % H).view(1, self.m, 1)
        bits = (self.alive.long().unsqueeze(-1) >> self._slot) & 1   # [depth, m, 5]
        before = bits.cumsum(-1) - bits                              # set bits below each slot
        kill = (bits != 0) & (before == s) & card
        self.alive.copy_(self.alive.long() & ~((kill.long() << self._slot).sum(-1)))

    def push(self, prev_rows, moves, draw, valid, seat=None):
        """A new newest entry: every entry shifts down by one, the oldest is dropped. Its alive mask is every occupied slot of
        my hand in prev_rows (seat: my seat; default: the seat after prev_rows' current player, row by row)."""
        dev = self.alive.device
        prev = torch.as_tensor(prev_rows).to(device=dev, dtype=torch.int32)
        if tuple(prev.shape) != (self.m, self.state_words):
            raise ValueError(f"history's previous rows have shape ({self.m}, {self.state_words}), got {tuple(prev.shape)}")
        mv, vl = torch.as_tensor(moves).to(dev), torch.as_tensor(valid).to(dev)
        if tuple(mv.shape) != (self.m,) or tuple(vl.shape) != (self.m,):
            raise ValueError(f"moves and valid have shape ({self.m},), got {tuple(mv.shape)} and {tuple(vl.shape)}")
        for t in (self.prev_rows, self.moves, self.alive, self.valid):
            if self.depth > 1:
                t[1:] = t[:-1].clone()
        if seat is None:
            st = (current_player(prev).long() + 1) % self.cfg.players
        else:
            if not 0 <= int(seat) < self.cfg.players:
                raise ValueError(f"seat {seat} out of range for {self.cfg.players} players")
            st = torch.full((self.m,), int(seat), dtype=torch.long, device=dev)
        hand = prev.gather(1, (10 + st).view(self.m, 1)).long().view(self.m, 1)
        occupied = ((hand >> (5 * self._slot.view(1, 5))) & 31) != 31
        self.prev_rows[0], self.moves[0] = prev, mv.to(torch.int32)
        self.alive[0] = (occupied.long() << self._slot.view(1, 5)).sum(-1).to(torch.uint8)
        self.valid[0] = (vl != 0).to(torch.uint8)
        self.draws = [int(draw)] + self.draws[:-1]
        self.filled = min(self.filled + 1, self.depth)

    def advance(self, own_moves=None, reset=None, cur_rows=None, prev_rows=None, seat=None, draw=None):
        """One turn of the observer `seat`, for all m games, in this order; each part is skipped when its argument is None:

          own_moves [m] int32   own_move(own_moves): the move I made since the last call;
          reset [m] (!= 0)      a game that was dealt anew since the last call: its valid and alive entries are cleared;
          cur_rows, prev_rows   [m, SW], given together with `seat` and `draw`: push(prev_rows, last_move_uid(cfg, cur_rows), draw,
                                valid, seat=seat), where an entry is valid iff cur is running and names a last mover other than
                                `seat` in word 2, and prev is running with that mover as its current player.

        A history on the GPU makes ONE kernel call (hb_belief_history_step), in place; on the CPU the same thing is done with the
        methods above, which is what the kernel is tested against."""
        dev, m = self.alive.device, self.m
        push = cur_rows is not None or prev_rows is not None
        if push:
            if cur_rows is None or prev_rows is None:
                raise ValueError("cur_rows and prev_rows go together")
            if seat is None or draw is None:
                raise ValueError("a push needs the observer's seat and the draw of the partner's turn")
        if seat is not None and not 0 <= int(seat) < self.cfg.players:
            raise ValueError(f"seat {seat} out of range for {self.cfg.players} players")

        def arg(x, shape, dtype, name):
            if x is None:
                return None
            t = torch.as_tensor(x)
            if tuple(t.shape) != shape:
                raise ValueError(f"{name} has shape {shape}, got {tuple(t.shape)}")
            if t.device != dev:
                raise ValueError(f"{name} lives on {t.device}, the history on {dev}")
            if dtype == torch.uint8 and t.dtype != torch.uint8:   # a flag of any type
                t = t.view(torch.uint8) if t.dtype in (torch.int8, torch.bool) else (t != 0).to(torch.uint8)
            return t.to(dtype).contiguous()

        own = arg(own_moves, (m,), torch.int32, "own_moves")
        rs = arg(reset, (m,), torch.uint8, "reset")
        cur = arg(cur_rows, (m, self.state_words), torch.int32, "cur_rows")
        prev = arg(prev_rows, (m, self.state_words), torch.int32, "prev_rows")
        if dev.type == "cuda":
            with torch.cuda.device(dev):
                K.check(K.lib().hb_belief_history_step(C.byref(self.cfg), m, self.depth, 0 if seat is None else int(seat), K.dptr(own),
                                                       K.dptr(rs), K.dptr(cur), K.dptr(prev), K.dptr(self.prev_rows),
                                                       K.dptr(self.moves), K.dptr(self.alive), K.dptr(self.valid), K.current_stream()))
            if push:
                self.draws = [int(draw)] + self.draws[:-1]
                self.filled = min(self.filled + 1, self.depth)
            return
        if own is not None:
            self.own_move(own)
        if rs is not None:
            gone = rs != 0
            self.valid[:, gone] = 0
            self.alive[:, gone] = 0
        if push:
            w2 = cur[:, 2]
            partner = (w2 >> 1) & 7
            valid = running(cur) & ((w2 & 1) != 0) & (partner != int(seat)) & running(prev) & (current_player(prev) == partner)
            self.push(prev, last_move_uid(self.cfg, cur), draw, valid, seat=seat)


class BeliefSample(NamedTuple):
    """What `ConditionedDeterminizer.sample` and `.sample_history` return, for a history of depth D:

        rows       [m * replicas, SW] int32   replica r of root i = row i * replicas + r
        weights    [m * replicas] int64       (the caller's int32 buffer with `out`); 0 marks a dead replica
        n_surv     [D, m] int32               the candidates that reproduce the partner's last d + 1 moves
        depth_used [m] int32                  the moves the replicas of the root reproduce (epsilon: the usable moves)
        fallback   [m] uint8                  0: filtered, 1: no survivor at any depth, 2: no usable entry (the unconditioned belief)
        ess        [m] float32                epsilon: the effective sample size of the weighted candidates; None without"""

    rows: torch.Tensor
    weights: torch.Tensor
    n_surv: torch.Tensor
    depth_used: torch.Tensor
    fallback: torch.Tensor
    ess: Optional[torch.Tensor]

    def survivors(self):
        """[m] int32: n_surv at the depth used, the candidates that pass the filter the replicas come from; 0 where
        depth_used is 0."""
        used = self.depth_used.long()
        return torch.where(used > 0, self.n_surv.gather(0, (used - 1).clamp(min=0).view(1, -1)).view(-1), 0)


class ConditionedDeterminizer:
    """The V0 belief conditioned on the partner's last moves: candidates from `Determinizer`, each
    previous state with each candidate hand spliced in (hb_belief_splice_alive), the partner's move in each of them (its
    `eval_moves` on an m-game scratch env, one slab of candidates at a time), and the first `replicas` candidates under which
    those moves are the ones the partner made (hb_belief_select_depth). There is one path, `sample_history`; `sample` is that
    path on the `LastMove`. The scratch env and the buffers are kept per (m, K).

    stateless (default True; an attribute that may be switched between calls): a partner that declares `obs_only_eval = True`
    (DQNAgent: its eval_moves reads only the observation and legal mask it is handed) gets them from ONE hb_encode_rows call over
    all K slabs instead of an import and an observe per slab; the scratch env is not touched and the results are the same bits.
    Every other partner, and stateless=False, takes the scratch env.

    epsilon (to sample / sample_history; default None: the exact-match filter above, unchanged): the partner is read as
    epsilon-greedy on `partner`'s policy. Every candidate keeps a likelihood (soft_table: 1 - eps + eps / n per reproduced move,
    eps / n per missed one, n = the legal moves of the hypothetical state, recorded per slab from the legal mask the partner is
    shown) and the replicas are drawn in proportion to importance weight times likelihood (hb_belief_select_soft): no depth
    fallback, every replica weighs 1, and the result carries the candidates' effective sample size `ess`."""

    def __init__(self, game="Hanabi-Full", players=2, config=None, stateless=True):
        self.det = Determinizer(game, players, config)
        self.cfg, self.players, self.state_words = self.det.cfg, self.det.players, self.det.state_words
        self.stateless = bool(stateless)   # may be switched at any time; False: every slab through the scratch env
        self._sized = {}   # (m, K) -> scratch env and buffers
        self._scratch = weakref.WeakKeyDictionary()   # agent -> the buffers its eval_moves writes
        self._tables = {}   # (epsilon, device) -> soft_table on the device

    def _soft(self, b, epsilon, D, Kn, m, dev):
        """What the soft filter needs beside the hard one's buffers -> (p_table on the device, n_legal [D, Kn, m] int32)."""
        if Kn > MAX_SOFT_CANDIDATES:
            raise ValueError(f"the soft filter takes at most {MAX_SOFT_CANDIDATES} candidates per root, got replicas * oversample = {Kn}")
        key = (float(epsilon), dev)
        if key not in self._tables:
            self._tables[key] = soft_table(epsilon, K.lib().hb_num_actions(C.byref(self.cfg)), device=dev)
        nleg = b.get("n_legal")
        if nleg is None or nleg.shape[0] != D:
            nleg = b["n_legal"] = torch.ones((D, Kn, m), dtype=torch.int32, device=dev)
        return self._tables[key], nleg

    def _setup(self, m, Kn, dev):
        b = self._sized.get((m, Kn))
        if b is None:
            self._sized.clear()   # one size at a time
            SW = self.state_words
            b = self._sized[(m, Kn)] = dict(
                env=HanabiEnv(config=self.cfg, n_games=m, device=dev, packed=True),
                cand_rows=torch.empty((m * Kn, SW), dtype=torch.int32, device=dev),
                cand_w=torch.empty(m * Kn, dtype=torch.int32, device=dev),
                hyp_rows=torch.empty((Kn, m, SW), dtype=torch.int32, device=dev),
                hyp_moves=torch.empty((Kn, m), dtype=torch.int32, device=dev))
        return b

    def _slab_views(self, b, partner, m, Kn, dev):
        """The stateless path: all Kn slabs of b["hyp_rows"] encoded by ONE hb_encode_rows call, for a
        partner whose eval_moves reads nothing but the (observation, legal mask) pair it is handed (`obs_only_eval`). -> (obs
        [Kn, m, obs_words], legal [Kn, m, A]), or None: this partner, or stateless=False, takes the scratch env. Every slab
        starts on a 16-byte boundary, as the scratch env's buffers do: where m rows of either output are no multiple of 16
        bytes (m not a multiple of 4, for the built games) the slabs are padded apart and encoded one call each."""
        if not (self.stateless and getattr(partner, "obs_only_eval", False)):
            return None
        SW = self.state_words
        if "slab_obs" not in b:
            L = K.lib()
            NW, A = L.hb_obs_words(C.byref(self.cfg)), L.hb_num_actions(C.byref(self.cfg))
            mp = m if (m * NW * 4) % 16 == 0 and (m * A) % 16 == 0 else (m + 15) // 16 * 16
            b["slab_obs"] = torch.empty((Kn, mp, NW), dtype=torch.int32, device=dev)
            b["slab_legal"] = torch.empty((Kn, mp, A), dtype=torch.int8, device=dev)
        obs, legal = b["slab_obs"], b["slab_legal"]
        if obs.shape[1] == m:
            encode_rows(self.cfg, b["hyp_rows"].view(Kn * m, SW), out=(obs.view(Kn * m, -1), legal.view(Kn * m, -1)))
            return obs, legal
        for k in range(Kn):
            encode_rows(self.cfg, b["hyp_rows"][k], out=(obs[k, :m], legal[k, :m]))
        return obs[:, :m], legal[:, :m]

    def _slab_moves(self, b, partner, m, Kn, dev, partner_seed, partner_draw, moves, nleg):
        """The partner's eval_moves with (partner_seed, partner_draw) on the Kn slabs of b["hyp_rows"] -> moves [Kn, m] int32 and,
        where nleg [Kn, m] int32 is given, the number of legal moves it was shown in each. The stateless path where the partner
        allows it (_slab_views), else one import and observe of the scratch env per slab (its first_game_id set by the caller)."""
        env = b["env"]
        vec = partner.requires_vectorized_observation()
        slabs = self._slab_views(b, partner, m, Kn, dev)
        if slabs is not None and nleg is not None:
            torch.sum(slabs[1], dim=-1, dtype=torch.int32, out=nleg)
        for k in range(Kn):
            if slabs is not None:
                partner.eval_moves((None, (slabs[0][k], slabs[1][k])), int(partner_seed), int(partner_draw), moves[k],
                                   scratch=self._scratch.setdefault(partner, {}))
                continue
            env.import_state(b["hyp_rows"][k])
            if vec or nleg is not None:   # import_state moves the rows only: the seat's observation and legal mask are encoded here
                env.observe()
            if nleg is not None:
                torch.sum(env.legal, dim=1, dtype=torch.int32, out=nleg[k])
            _ask(partner, env, int(partner_seed), int(partner_draw), moves[k], self._scratch)

    def sample(self, rows, prev_rows, partner, seat, replicas, oversample, seed, draw, partner_seed, partner_draw, first_game_id,
               valid=None, first_row_id=0, out=None, epsilon=None):
        """rows [m, SW] the current states (seat `seat` to act), prev_rows [m, SW] the states the partner moved from, partner:
        the agent that moved (its eval_moves is called with partner_seed / partner_draw on games first_game_id + i: what it was
        called with in the real game), valid [m] (0: no usable previous state; the root keeps the unconditioned belief). A
        prev_rows that is not the state the partner moved from (another deal, a hand of another size for `seat`) gives some
        legal hypothetical state, not a specified one. This is sample_history() on the `LastMove` of these arguments: the
        same `BeliefSample`, n_surv [1, m]."""
        r = _rows(rows, self.state_words)
        last = LastMove(prev_rows, partner_seed, partner_draw, first_game_id, valid, m=r.shape[0], words=self.state_words, device=r.device)
        return self.sample_history(r, last, partner, seat, replicas, oversample, seed, draw, partner_seed, first_game_id,
                                   first_row_id=first_row_id, out=out, epsilon=epsilon)

    @torch.no_grad()
    def sample_history(self, rows, history, partner, seat, replicas, oversample, seed, draw, partner_seed, first_game_id,
                       first_row_id=0, out=None, epsilon=None):
        """rows [m, SW] the current states (seat `seat` to act), conditioned on the partner's last history.depth moves (a
        `PartnerHistory` of these m roots, observer `seat`, or a `LastMove`). K = replicas * oversample candidates per root are
        drawn ONCE, with (seed, draw) and row ids first_row_id + i * K + k; for each entry d they are carried back to its
        previous state with its alive mask (hb_belief_splice_alive) and the partner's eval_moves runs on the K slabs with
        (partner_seed, history.draws[d]) on games first_game_id + i; one hb_belief_select_depth keeps, per root, the first
        `replicas` candidates that reproduce the most leading moves. Entries that were never pushed cost no slab pass.
        -> `BeliefSample`. `out`: an optional (rows_out, weights_u32) pair to write into (the weights then come back as that
        int32 buffer). epsilon: see the class docstring (hb_belief_select_soft: depth_used is the number of usable moves,
        fallback 0 or 2, and the replicas are drawn with (seed, draw) and row ids first_row_id + i)."""
        r = _rows(rows, self.state_words)
        m, R, ov = r.shape[0], int(replicas), int(oversample)
        if R < 1 or ov < 1:
            raise ValueError(f"replicas and oversample must be >= 1, got {replicas} and {oversample}")
        if not 0 <= int(seat) < self.players:
            raise ValueError(f"seat {seat} out of range for {self.players} players")
        if not hasattr(partner, "eval_moves"):
            raise TypeError(f"{type(partner).__name__} has no eval_moves()")
        if not isinstance(history, (PartnerHistory, LastMove)):
            raise TypeError(f"history must be a PartnerHistory or a LastMove, got {type(history).__name__}")
        if history.m != m or history.state_words != self.state_words:
            raise ValueError(f"the history holds {history.m} roots of {history.state_words} words, the rows are {tuple(r.shape)}")
        dev, Kn, D = r.device, R * ov, history.depth
        if history.prev_rows.device != dev:
            raise ValueError(f"the history lives on {history.prev_rows.device}, the rows on {dev}")
        b = self._setup(m, Kn, dev)
        env = b["env"]
        hyp = b.get("hyp_depth")
        if hyp is None or hyp.shape[0] != D:
            hyp = b["hyp_depth"] = torch.zeros((D, Kn, m), dtype=torch.int32, device=dev)
        table, nleg = (None, None) if epsilon is None else self._soft(b, epsilon, D, Kn, m, dev)
        with torch.cuda.device(dev):
            # the chain of usable entries, root by root: an entry behind an invalid one is never read, and a root without a
            # usable entry is never filtered, so their slab rows only have to be states the partner's policy can be run on,
            # and the current row is one
            usable = running(r).view(1, m) if history.valid is None else (history.valid != 0) & running(r).view(1, m)
            chain = usable if D == 1 else usable.cumprod(0) != 0   # [D, m] bool (one entry is its own chain: no launch for it)
            chain_u8 = chain.to(torch.uint8)
            self.det.sample(r, seat=int(seat), replicas=Kn, seed=seed, draw=draw, first_row_id=first_row_id,
                            out=(b["cand_rows"], b["cand_w"]))
            env.first_game_id = int(first_game_id)   # (the scratch env never deals: its game ids key the partner's draws only)
            for d in range(min(D, history.filled)):
                prev = torch.where(chain[d].view(m, 1), history.prev_rows[d], r).contiguous()
                alive = None if history.alive is None else history.alive[d].contiguous()
                belief_splice_alive(self.cfg, prev, alive, b["cand_rows"], int(seat), Kn, out=b["hyp_rows"])
                self._slab_moves(b, partner, m, Kn, dev, partner_seed, history.draws[d], hyp[d], None if nleg is None else nleg[d])
            actual = last_move_uid(self.cfg, r).view(1, m) if history.moves is None else history.moves.contiguous()
            if out is not None:
                out = tuple(out) + _bufs(dev, None, ((D, m), torch.int32), ((m,), torch.int32), ((m,), torch.uint8))
            if epsilon is None:
                res = belief_select_depth(self.cfg, r, b["cand_rows"], b["cand_w"], hyp, actual, chain_u8, R, out=out) + (None,)
            else:
                res = belief_select_soft(self.cfg, r, b["cand_rows"], b["cand_w"], hyp, nleg, actual, chain_u8, table, R, seed, draw,
                                         first_row_id=first_row_id,
                                         out=None if out is None else out + _bufs(dev, None, ((m,), torch.float32)))
        return BeliefSample(res[0], res[1] if out is not None else res[1].long() & 0xFFFFFFFF, *res[2:])


def exact_table(n_actions, device=None):
    """soft_table's layout for a partner that never leaves its policy: [2, A + 1] float64, row 0 all 1 (the move is the policy's),
    row 1 all 0 (it is not), column 0 zero. hb_belief_select_soft with this table is the exact filter on weighted candidates."""
    A = int(n_actions)
    if A < 1:
        raise ValueError(f"n_actions must be >= 1, got {n_actions}")
    t = torch.tensor([[0.0] + [1.0] * A, [0.0] * (A + 1)], dtype=torch.float64)
    return t if device is None else t.to(device)


class TrackedRows:
    """What `TrackedBelief.step` hands to RolloutSearch as `history`: rows [m * K, SW] int32 / weights [m * K] int32, the K
    equally weighted particles of each root (weight 0: dead), of which a search of R replicas takes particles start .. start + R
    - 1; and per root n_surv [m] int32, fallback [m] uint8, depth_used [m] int32, ess [m] float32 (as SearchResult's), tracked /
    restarted [m] bool and carried_live [m] int32 (the live particles after the carry)."""

    def __init__(self, rows, weights, n_particles, n_surv, fallback, depth_used, ess, tracked, restarted, carried_live, start=0):
        self.rows, self.weights, self.n_particles, self.start = rows, weights, int(n_particles), int(start)
        self.n_surv, self.fallback, self.depth_used, self.ess = n_surv, fallback, depth_used, ess
        self.tracked, self.restarted, self.carried_live = tracked, restarted, carried_live

    def shifted(self, by):
        """The same particles, read from `by` places further on (a confirming stage: particles the first stage did not see)."""
        return TrackedRows(self.rows, self.weights, self.n_particles, self.n_surv, self.fallback, self.depth_used, self.ess,
                           self.tracked, self.restarted, self.carried_live, start=self.start + int(by))

    def take(self, m, R, out):
        """Particles start .. start + R - 1 of each of the m roots -> out = (rows [m * R, SW], weights [m * R])."""
        Kn, SW = self.n_particles, self.rows.shape[1]
        if self.rows.shape[0] != m * Kn:
            raise ValueError(f"the tracked belief holds {self.rows.shape[0]} rows, the search has {m} roots of {Kn} particles")
        if self.start + R > Kn:
            raise ValueError(f"the tracked belief holds {Kn} particles per root, particles {self.start}..{self.start + R - 1} were asked for")
        out[0].view(m, R, SW).copy_(self.rows.view(m, Kn, SW)[:, self.start:self.start + R])
        out[1].view(m, R).copy_(self.weights.view(m, Kn)[:, self.start:self.start + R])


class TrackedBelief:
    """The search belief tracked across turns, 2 players ("Tracking the belief"): per root the K = replicas *
    oversample hand samples of the observer's last turn are kept, carried to the present turn (hb_belief_carry: the card I played
    leaves, the others stay if the pool and the hints since allow them, the new card and the deck are drawn afresh, the weight
    counts the copies of the card the partner drew), spliced into the state the partner moved from (hb_belief_splice), weighed
    by the likelihood of the ONE move the partner has made since (its eval_moves on the K slabs, `ConditionedDeterminizer`'s slab
    code) and resampled to K equally weighted particles (hb_belief_select_soft with replicas = K). The first `replicas` of them
    are the search's replicas: the draws are exchangeable.

    A root STARTS OVER when it has no particle set yet, when its previous turn is not usable, or when its resampling total is 0
    (no carried particle explains what was seen): it takes K rows from `ConditionedDeterminizer.sample_history` (on the PartnerHistory
    given, or on the `LastMove`), with the caller's epsilon, K candidates. That path runs only when some root needs it (one host
    synchronisation per step decides). A restart is normal — a first move, a partner that explores — and only counted."""

    def __init__(self, game="Hanabi-Full", players=2, config=None, replicas=32, oversample=8, cdet=None):
        self.cdet = cdet if cdet is not None else ConditionedDeterminizer(game, players, config)
        self.cfg, self.state_words = self.cdet.cfg, self.cdet.state_words
        if self.cfg.players != 2:
            raise ValueError(f"track=True is built for 2 players, got {self.cfg.players}")
        self.replicas, self.oversample = int(replicas), int(oversample)
        if self.replicas < 1 or self.oversample < 1:
            raise ValueError(f"replicas and oversample must be >= 1, got {replicas} and {oversample}")
        self.n_particles = self.replicas * self.oversample
        if self.n_particles > MAX_SOFT_CANDIDATES:
            raise ValueError(f"the soft filter takes at most {MAX_SOFT_CANDIDATES} candidates per root, got replicas * oversample = "
                             f"{self.n_particles}")
        self.num_actions = K.lib().hb_num_actions(C.byref(self.cfg))
        self.rows = self.weights = self.have = None   # [m * K, SW] int32, [m * K] int32, [m] bool: the particle sets
        self._tables, self._nleg = {}, None

    def clear(self):
        """Forget every particle set: the next step starts every root over."""
        if self.have is not None:
            self.have.zero_()

    def observed(self, rows, then_rows, then_moves, prev_rows, seat):
        """What has become public between my last turn and now, on the device, no host synchronisation -> (own_slot, revealed,
        drew) [m] int32 as hb_belief_carry reads them. own_slot: the slot of then_moves where that is a discard or a play;
        revealed: the card word 2 of prev_rows (then_rows stepped with my move) names, where it records a discard or a play of
        mine; drew: the partner's newest hand slot in `rows`, where word 2 of `rows` records a discard or a play of the partner's
        and its hand is as large as in prev_rows."""
        H, Rk, st, pt = self.cfg.hand_size, self.cfg.ranks, int(seat), 1 - int(seat)
        mv = then_moves.long()
        own_slot = torch.where((mv >= 0) & (mv < 2 * H), mv % H, -1)
        w2 = prev_rows[:, 2].long() & 0xFFFFFFFF
        mine = ((w2 & 1) != 0) & (((w2 >> 1) & 7) == st) & (((w2 >> 4) & 3) < 2)
        revealed = torch.where(mine & (own_slot >= 0), ((w2 >> 12) & 7) * Rk + ((w2 >> 15) & 7), -1)
        c2 = rows[:, 2].long() & 0xFFFFFFFF
        size = lambda r: (r[:, 1].long() >> (15 + 3 * pt)) & 7
        n_now = size(rows)
        took = ((c2 & 1) != 0) & (((c2 >> 1) & 7) == pt) & (((c2 >> 4) & 3) < 2) & (n_now == size(prev_rows)) & (n_now >= 1)
        newest = ((rows[:, 10 + pt].long() & 0xFFFFFFFF) >> (5 * (n_now - 1).clamp(min=0))) & 31
        drew = torch.where(took, newest, -1)
        return own_slot.int().contiguous(), revealed.int().contiguous(), drew.int().contiguous()

    def _table(self, epsilon, dev):
        key = (None if epsilon is None else float(epsilon), dev)
        if key not in self._tables:
            self._tables[key] = (exact_table if epsilon is None else lambda A, device: soft_table(epsilon, A, device=device))(
                self.num_actions, device=dev)
        return self._tables[key]

    @torch.no_grad()
    def step(self, rows, then_rows, then_moves, prev_rows, valid, partner, seat, seed, draw, partner_seed, partner_draw, first_game_id,
             epsilon=None, history=None, first_row_id=0):
        """One turn. rows [m, SW] the states now (`seat` to act); then_rows [m, SW] / then_moves [m] my last turn and the moves I
        played there (None: there is none, every root starts over); prev_rows [m, SW] / valid [m] the states the partner moved
        from and where that is usable (SearchPlayer._previous); partner: the agent that moved, called with (partner_seed,
        partner_draw) on games first_game_id + i; (seed, draw, first_row_id) key the carry's and the resampling's draws; epsilon:
        the partner read as epsilon-greedy (None: the exact filter, `exact_table`); history: the PartnerHistory a root that starts
        over is conditioned on (None: prev_rows alone). -> `TrackedRows`; the particle sets are replaced."""
        r = _rows(rows, self.state_words)
        m, Kn, SW, dev = r.shape[0], self.n_particles, self.state_words, r.device
        if not 0 <= int(seat) < 2:
            raise ValueError(f"seat {seat} out of range for 2 players")
        if not hasattr(partner, "eval_moves"):
            raise TypeError(f"{type(partner).__name__} has no eval_moves()")
        last = LastMove(prev_rows, partner_seed, partner_draw, first_game_id, valid, m=m, words=SW, device=dev)
        prev, valid = last.prev_rows[0], None if last.valid is None else last.valid[0]
        if self.rows is None or self.rows.shape[0] != m * Kn or self.rows.device != dev:
            self.rows = torch.zeros((m * Kn, SW), dtype=torch.int32, device=dev)
            self.weights = torch.zeros(m * Kn, dtype=torch.int32, device=dev)
            self.have = torch.zeros(m, dtype=torch.bool, device=dev)
            self._next = (torch.empty_like(self.rows), torch.empty_like(self.weights))
            self._nleg = torch.ones((1, Kn, m), dtype=torch.int32, device=dev)
        cd = self.cdet
        b = cd._setup(m, Kn, dev)
        with torch.cuda.device(dev):
            live = running(r)
            usable = live & self.have if valid is None else live & self.have & (valid != 0)
            if then_rows is None:
                usable = torch.zeros_like(usable)
                own_slot = revealed = drew = torch.full((m,), -1, dtype=torch.int32, device=dev)
            else:
                then = _rows(then_rows, SW, dev)
                own_slot, revealed, drew = self.observed(r, then, torch.as_tensor(then_moves).to(dev).view(m), prev, seat)
            old_w = torch.where(usable.view(m, 1), self.weights.view(m, Kn), 0).view(-1)
            belief_carry(self.cfg, r, self.rows, old_w, own_slot, revealed, drew, seat, Kn, seed, draw, first_row_id=first_row_id,
                         out=(b["cand_rows"], b["cand_w"]))
            carried_live = (b["cand_w"].view(m, Kn) != 0).sum(1).int()
            # a root that cannot be carried is never weighed: its slab rows only have to be states the partner can be run on
            prev = torch.where(usable.view(m, 1), prev, r).contiguous()
            belief_splice(self.cfg, prev, b["cand_rows"], int(seat), Kn, out=b["hyp_rows"])
            b["env"].first_game_id = int(first_game_id)
            cd._slab_moves(b, partner, m, Kn, dev, partner_seed, partner_draw, b["hyp_moves"], self._nleg[0])
            n_surv, used, fallback, ess = _bufs(dev, None, ((1, m), torch.int32), ((m,), torch.int32), ((m,), torch.uint8),
                                                ((m,), torch.float32))
            belief_select_soft(self.cfg, r, b["cand_rows"], b["cand_w"], b["hyp_moves"].view(1, Kn, m), self._nleg,
                               last_move_uid(self.cfg, r).view(1, m), usable.to(torch.uint8).view(1, m), self._table(epsilon, dev), Kn,
                               seed, draw, first_row_id=first_row_id, out=self._next + (n_surv, used, fallback, ess))
            new_rows, new_w = self._next
            tracked = usable & (new_w.view(m, Kn)[:, 0] != 0)   # (a resampling total of 0 leaves every particle dead)
            restarted = live & ~tracked
            n_surv, used = n_surv[0], tracked.int()
            fallback = torch.where(tracked, 0, 2).to(torch.uint8)
            if bool(restarted.any().item()):
                new = cd.sample_history(r, history if history is not None else last, partner, seat, Kn, 1, seed, draw, partner_seed,
                                        first_game_id, first_row_id=first_row_id, epsilon=epsilon)
                pick = restarted.view(m, 1)
                new_rows.view(m, Kn * SW).copy_(torch.where(pick, new.rows.view(m, Kn * SW), new_rows.view(m, Kn * SW)))
                new_w.view(m, Kn).copy_(torch.where(pick, new.weights.view(m, Kn).int(), new_w.view(m, Kn)))
                n_surv, used = torch.where(restarted, new.survivors(), n_surv), torch.where(restarted, new.depth_used, used)
                fallback = torch.where(restarted, new.fallback, fallback)
                if new.ess is not None:
                    ess = torch.where(restarted, new.ess, ess)
            self._next = (self.rows, self.weights)
            self.rows, self.weights = new_rows, new_w
            self.have = live.clone()
        return TrackedRows(self.rows, self.weights, Kn, n_surv, fallback, used, ess, tracked, restarted,
                           torch.where(tracked, carried_live, 0))


class SearchResult:
    """value [m, A] f32 (NaN: illegal at the root, or no live replica), wsum [m, A] int64, n_live [m, A] int32, best [m] int32
    (-1: no action has a value), rollouts = games played, turns = turns of the longest rollout, dead = replicas of weight 0
    among the running roots' replicas. Device tensors. From run_candidates the second axis is the candidate slot: `cand` [m, C]
    int32 the uids searched, `best` the best slot and `best_uid` [m] int32 its uid (-1: none). With a baseline: `diff` [m, C] f64
    the weighted mean over the replicas of score[slot] - score[baseline], `se` [m, C] f64 its standard error (inf with fewer
    than two live replicas; both 0 in the baseline's slot, NaN where there is no candidate, no baseline or no live replica) and
    `n_pair` [m] int32 the live replicas (hb_search_compare). None when not computed. With `history` (the belief conditioned on
    the partner's last move): `n_surv` [m] int32 and `fallback` [m] uint8 of hb_belief_select_depth; None without. With a
    `PartnerHistory` (its last `depth` moves): `n_surv` [depth, m], `fallback` and `depth_used` [m] int32 of
    hb_belief_select_depth; `depth_used` is None when not computed. With the search's `epsilon` (the soft filter,
    hb_belief_select_soft): `ess` [m] float32, the effective sample size of each root's weighted candidates; None without.
    `sample` is the `BeliefSample` these four are read from (None without a history, and with a `TrackedRows`).
    With the search's `score_belief`: `belief`, the `BeliefScore` of the replicas searched against the roots' real hands.
    `horizon`: the search's (None: rollouts to the end); `leaves`: the played games that were still running after `horizon` turns
    and were valued there (0 without a horizon); `turns` is then at most the horizon."""

    def __init__(self, value, wsum, n_live, best, rollouts, turns, dead=0, replicas=0, diff=None, se=None, n_pair=None, cand=None,
                 best_uid=None, n_surv=None, fallback=None, depth_used=None, ess=None, belief=None, sample=None, horizon=None, leaves=0):
        self.value, self.wsum, self.n_live, self.best = value, wsum, n_live, best
        self.horizon, self.leaves = horizon, int(leaves)
        self.rollouts, self.turns, self.dead, self.replicas = int(rollouts), int(turns), int(dead), int(replicas)
        self.diff, self.se, self.n_pair, self.cand, self.best_uid = diff, se, n_pair, cand, best_uid
        self.n_surv, self.fallback, self.depth_used, self.ess, self.belief = n_surv, fallback, depth_used, ess, belief
        self.sample = sample

    def __repr__(self):
        return f"SearchResult(roots={self.value.shape[0]}, rollouts={self.rollouts}, turns={self.turns})"


def rollout(env, cfg, blueprint, seed, first_seat, forced, done, final_score, length, counters, act, scratch, check_every=8,
            turn_limit=None, horizon=None, playout=False, rows=None):
    """Play the games of `env` (auto-reset off, state imported) to the end: turn 0 plays `forced` for seat `first_seat`, turn
    t >= 1 the move of blueprint[(first_seat + t) % P].eval_moves with draw t + 1; hb_eval_tally after every step. `done`
    (bit 0x80: not played) and `counters` ([0] = games live) are set up by the caller. Returns the number of turns played.
    horizon = H (default None: to the end): at most H turns, the forced one included; returns (turns, games still live), and
    games still live are then no error: seat (first_seat + turns) % P is to act in them, on the env's current observation.
    playout=True with `rows` (default False: the loop above, launch for launch): when the blueprint is rule lists only and there
    is no horizon (`playout_supported`), the games are played by one hb_rule_playout launch on `rows` [n, state_words] in place
    instead — the env is not touched, it need not hold the states —, with the env's game ids; done, final_score, length and
    counters end as the loop leaves them, the slots not played keep their rows, and the turns returned are the longest game's
    length. Illegal moves raise here (the loop's caller reads the env's count). Any other blueprint, or a horizon: the loop."""
    limit = max_turns(cfg) if turn_limit is None else turn_limit
    if playout and rows is not None and playout_supported(blueprint, horizon=horizon):
        res = playout_launch(cfg, rows, blueprint, seed, first_seat, forced, limit, env.first_game_id, done, final_score, length,
                             counters, None)
        live, illegal, t = torch.cat([counters[:1], res.illegal, res.max_len.long()]).tolist()   # the one host read
        if illegal:
            raise RuntimeError(f"{illegal} illegal moves in the rollouts (a candidate that is illegal at its root, or the blueprint's)")
        if live != 0:
            raise RuntimeError(f"{live} rollout games still live after {limit} turns")
        return t
    L, P, n = K.lib(), cfg.players, env.n
    cfg_ref = C.byref(cfg)
    bufs = tuple(K.dptr(t) for t in (env.reward, env.terminal, env.score, done, final_score, length, counters))
    if horizon is not None:
        limit = min(limit, int(horizon))
    live, t = -1, 0
    while t < limit:
        seat = (first_seat + t) % P
        if t == 0:
            moves = forced
        else:
            moves = act
            _ask(blueprint[seat], env, seed, t + 1, act, scratch)
        env.step(moves)
        K.check(L.hb_eval_tally(cfg_ref, n, seat, t, K.dptr(moves), *bufs, K.current_stream()))
        t += 1
        if t % check_every == 0 or t == limit:
            live = int(counters[0].item())
            if live == 0:
                break
    if horizon is not None:
        return t, live
    if live != 0:
        raise RuntimeError(f"{live} rollout games still live after {limit} turns")
    return t


def check_horizon(horizon):
    """horizon as the search keeps it: None (play to the end), or an int >= 1 (a bool or a float is refused)."""
    if horizon is None:
        return None
    if isinstance(horizon, bool) or not isinstance(horizon, int):
        raise TypeError(f"horizon is a number of turns (an int >= 1) or None, got {horizon!r}")
    if horizon < 1:
        raise ValueError(f"horizon must be >= 1 (the forced first move counts), got {horizon}")
    return horizon


def leaf_max_score(cfg):
    """colors * ranks of a config whose scores fit the int8 score buffer in quarter points; ValueError for any other."""
    top = int(cfg.colors) * int(cfg.ranks)
    if LEAF_SCALE * top > 127:
        raise ValueError(f"a depth-limited search keeps quarter points in int8: {LEAF_SCALE} * colors * ranks = {LEAF_SCALE * top} > 127")
    return top


def leaf_agents(blueprint, leaf, seats=None):
    """The agents whose eval_q values the leaves, one per seat, or "score": leaf = None (the blueprint's own), a list of one
    agent per seat, or "score" (no agent: a pure truncated rollout). seats: the seats that can be to act at a leaf; the agent of
    each must have eval_q (TypeError)."""
    n = len(blueprint)
    if isinstance(leaf, str):
        if leaf != "score":
            raise ValueError(f'leaf is None, "score" or one agent per seat, got {leaf!r}')
        return "score"
    agents = list(blueprint) if leaf is None else list(leaf)
    if len(agents) != n:
        raise ValueError(f"one leaf agent per seat: {n} players, {len(agents)} agents")
    for s in range(n) if seats is None else seats:
        if not hasattr(agents[s], "eval_q"):
            raise TypeError(f"{type(agents[s]).__name__} (seat {s}) has no eval_q() to value a leaf with: pass leaf=[one agent with eval_q "
                            f'per seat] (a DQNAgent), or leaf="score" for a truncated rollout that counts the score so far')
    return agents


class RolloutSearch:
    """Value of every root action under `blueprint` by belief-sampled rollouts; see the module docstring.

    horizon = H (default None: every rollout is played to the end, and nothing below exists), leaf: depth-limited rollouts.
    A rollout plays H turns, the forced first move included; a game still running then is worth its score so far plus the
    largest legal q of `eval_q` of the seat then to act, (cp + H) % P, asked once on the env's current observation: leaf = None
    asks the blueprint's own agent of that seat (TypeError when it has no eval_q), leaf = [one agent per seat] any agents with
    eval_q (a DQNAgent valuing a rule list's states), leaf = "score" nobody (v = 0: a pure truncated rollout). The values are
    rounded to quarter points with a dither shared by the slots of a replica (`search_leaf`, `leaf_dither`: stochastic
    rounding, unbiased, and the paired differences keep their common random numbers) into an int8 buffer [m, C, R] that
    hb_search_reduce and hb_search_compare read as they read the final scores; value, diff and se are divided by 4, which is
    exact. When no game reaches the horizon running, nothing of this runs and the result is the full search's, bit for bit.
    The result carries `horizon` and `leaves`, the played games valued at the horizon.

    first_game_id: global id of rollout game 0 (keys the blueprint's draws, like Evaluator's). The rollout env and every
    buffer are built by the first search of a size (m roots, C slots — run(): the A actions —, replicas) and kept for the next,
    one entry per (C, replicas): a screening stage's env survives the confirming stage's, and another number of roots replaces
    the entry of its stage.

    history = (prev_rows, partner_seed, partner_draw, first_game_id[, valid]) to run / run_candidates / confirm: the replicas
    come from `ConditionedDeterminizer` (the belief conditioned on the last move, made from prev_rows by the seat before the
    roots' current player with those Philox keys) with `oversample` candidates per replica; everything after the
    determinization is the same. history may also be a `PartnerHistory` of the roots (the partner's last `depth` moves, with its
    partner_seed and first_game_id): the replicas then come from `ConditionedDeterminizer.sample_history` and the result carries
    `depth_used`. epsilon (default None: the exact-match filter): with a history, the candidates are weighed by the likelihood of
    an epsilon-greedy partner instead of filtered (`ConditionedDeterminizer`'s epsilon) and the result carries `ess`.
    score_belief (default False: nothing is computed): the replicas of every search are scored against the roots' real hands
    right after the determinization (hb_belief_score) and the result carries `belief`; the search itself is unchanged.
    playout (default False: the rollouts run on the turn loop, launch for launch as before): a blueprint of `RulebasedAgent`s only,
    searched without a horizon, is rolled out by ONE hb_rule_playout launch (hanabi_hip.playout) on the
    laid-out rows, with the forced first moves and the preset `done` bytes; the rollout env is not touched. Every figure of the
    result is the loop's bit for bit except `turns`, the longest rollout's length instead of the next multiple of `check_every`.
    Any other blueprint, or a horizon, takes the loop; `last_path` ("playout" or "loop") says what the last search did.
    exact, max_hands (defaults False, None = hanabi_hip.exact.DEFAULT_MAX_HANDS; with exact=False every path issues the launches it
    issued before): where `exact_supported` holds (a 2-player blueprint of `RulebasedAgent`s, no epsilon), the replicas of a search
    with a `PartnerHistory` or a last-move history come from the exact, enumerated belief (hanabi_hip.exact.ExactDeterminizer;
    DESIGN.md section 11f, "The exact belief") instead of filtered candidates. A root with more than max_hands hands takes the
    sampled path above, which runs only when there is such a root, and is merged in root by root. Otherwise the whole call is
    the sampled path. `last_belief` ("exact", "mixed" or "sampled") says which ran, `last_exact` is the search's `ExactBelief`."""

    def __init__(self, game="Hanabi-Full", players=2, replicas=32, seed=1, device=None, config=None, check_every=8, first_game_id=0,
                 oversample=8, epsilon=None, score_belief=False, horizon=None, leaf=None, playout=False, exact=False, max_hands=None):
        self.cfg = eval_config(game, players, config)
        self.players = self.cfg.players
        self.set_horizon(horizon, leaf)
        self.set_exact(exact, max_hands)
        self.edet = None          # hanabi_hip.exact.ExactDeterminizer, built by the first exact search
        self.last_belief = None   # "exact", "mixed" (some roots over max_hands took the sampled path) or "sampled"
        self.last_exact = None    # the ExactBelief of the last search that enumerated (None: it did not)
        if not isinstance(playout, bool):
            raise TypeError(f"playout is a switch (True or False), got {playout!r}")
        self.playout = playout
        self.last_path = None   # "playout" or "loop": how the last search's rollouts were played
        self.replicas = int(replicas)
        if self.replicas < 1:
            raise ValueError(f"replicas must be >= 1, got {replicas}")
        self.seed = int(seed)
        self.first_game_id = int(first_game_id)
        self.device = device
        self.check_every = max(1, int(check_every))
        self.det = Determinizer(config=self.cfg)
        self.oversample = int(oversample)
        if self.oversample < 1:
            raise ValueError(f"oversample must be >= 1, got {oversample}")
        self.cdet = None   # ConditionedDeterminizer, built by the first search with a history
        self.num_actions = K.lib().hb_num_actions(C.byref(self.cfg))
        self.epsilon = None if epsilon is None else float(epsilon)
        if self.epsilon is not None:
            soft_table(self.epsilon, self.num_actions)   # (the range check)
            if self.replicas * self.oversample > MAX_SOFT_CANDIDATES:
                raise ValueError(f"the soft filter takes at most {MAX_SOFT_CANDIDATES} candidates per root, got replicas * oversample = "
                                 f"{self.replicas * self.oversample}")
        if not isinstance(score_belief, bool):
            raise TypeError(f"score_belief is a switch (True or False), got {score_belief!r}")
        self.score_belief = score_belief
        self.n_counters = K.lib().hb_eval_counters(C.byref(self.cfg))
        self._sized = {}   # (m, C, replicas) -> the rollout env and buffers of that size, with the scratch of its blueprint
        self._uid = None   # [1, A] int32: every uid, on the device (built by the first run())

    def set_horizon(self, horizon, leaf=None):
        """The horizon and leaf agents of the searches from here on (the constructor's arguments, and its checks)."""
        horizon = check_horizon(horizon)
        if horizon is not None:
            self.max_score = leaf_max_score(self.cfg)
            if leaf is not None:
                leaf_agents([None] * self.players, leaf, seats=())   # (the checks that need neither blueprint nor seat)
        elif leaf is not None:
            raise ValueError("leaf= values the games a horizon cuts short: it needs horizon=H")
        self.horizon, self.leaf = horizon, leaf

    def set_exact(self, exact, max_hands=None):
        """The exact-belief switch of the searches from here on (the constructor's arguments, and its checks)."""
        from .exact import DEFAULT_MAX_HANDS

        if not isinstance(exact, bool):
            raise TypeError(f"exact is a switch (True or False), got {exact!r}")
        max_hands = DEFAULT_MAX_HANDS if max_hands is None else int(max_hands)
        if max_hands < 1:
            raise ValueError(f"max_hands must be >= 1, got {max_hands}")
        self.exact, self.max_hands = exact, max_hands

    def _sample_exact(self, b, r, history, blueprint, cp, R, draw, first_row_id):
        """The conditioned replicas of an exact search -> `BeliefSample` in b["det_rows"] / b["weights"]: every root from the
        enumerated belief (hanabi_hip.exact), except those with more than max_hands hands (status 1), which take
        `ConditionedDeterminizer`'s path, run only when there is such a root, and are merged in root by root."""
        from .exact import ExactDeterminizer

        m, dev, SW = r.shape[0], r.device, self.det.state_words
        if self.edet is None:
            self.edet = ExactDeterminizer(config=self.cfg)
        out = (b["det_rows"], b["weights"])
        sample, belief = self.edet.sample_history(r, history, blueprint, cp, R, self.seed, draw, history.partner_seed,
                                                  history.first_game_id, first_row_id=first_row_id, max_hands=self.max_hands, out=out)
        self.last_exact = belief
        large = belief.status == 1
        if not bool(large.any().item()):
            self.last_belief = "exact"
            return sample
        self.last_belief = "mixed"
        keep_rows, keep_w = sample.rows.clone(), sample.weights.clone()
        if self.cdet is None:
            self.cdet = ConditionedDeterminizer(config=self.cfg)
        other = self.cdet.sample_history(r, history, blueprint[(cp - 1) % self.players], cp, R, self.oversample, self.seed, draw,
                                         history.partner_seed, history.first_game_id, first_row_id=first_row_id, out=out)
        pick = lambda a, x: torch.where(large.view((1,) * (a.dim() - 1) + (m,)), a, x)
        b["det_rows"].copy_(torch.where(large.view(m, 1, 1), other.rows.view(m, R, SW), keep_rows.view(m, R, SW)).view(m * R, SW))
        b["weights"].copy_(torch.where(large.view(m, 1), other.weights.view(m, R), keep_w.view(m, R)).view(m * R))
        return BeliefSample(b["det_rows"], b["weights"], pick(other.n_surv, sample.n_surv), pick(other.depth_used, sample.depth_used),
                            pick(other.fallback, sample.fallback), None)

    def _setup(self, m, Cn, R, first_game_id, dev):
        b = self._sized.get((m, Cn, R))
        if b is None:
            # the same stage at another number of roots: a rollout env of the old size is memory the new one needs
            for k in [k for k in self._sized if k[1:] == (Cn, R)]:
                del self._sized[k]
            SW, n = self.det.state_words, m * Cn * R
            env = HanabiEnv(config=self.cfg, n_games=n, seed=self.seed, first_game_id=first_game_id, device=dev, packed=True)
            b = self._sized[(m, Cn, R)] = dict(
                env=env, det_rows=torch.empty((m * R, SW), dtype=torch.int32, device=dev),
                weights=torch.empty(m * R, dtype=torch.int32, device=dev),
                rows=torch.empty((n, SW), dtype=torch.int32, device=dev),
                forced=torch.empty(n, dtype=torch.int32, device=dev), act=torch.empty(n, dtype=torch.int32, device=dev),
                done=torch.empty(n, dtype=torch.uint8, device=dev), final_score=torch.empty(n, dtype=torch.int8, device=dev),
                length=torch.empty(n, dtype=torch.int16, device=dev),
                counters=torch.empty(self.n_counters, dtype=torch.int64, device=dev),
                n_played=torch.empty(m, dtype=torch.int32, device=dev),
                scratch=weakref.WeakKeyDictionary())   # agent -> the buffers its eval_moves writes
        # a rollout env never deals (auto-reset off, states imported): its game ids key the blueprint's draws only
        b["env"].first_game_id = first_game_id
        return b

    def _roots(self, rows, blueprint, seat):
        """The checks run() and run_candidates() share -> (rows on the device, blueprint, live [m] bool, current players)."""
        blueprint = list(blueprint)
        if len(blueprint) != self.players:
            raise ValueError(f"one blueprint agent per seat: {self.players} players, {len(blueprint)} agents")
        for a in blueprint:
            if not hasattr(a, "eval_moves"):
                raise TypeError(f"{type(a).__name__} has no eval_moves()")
        r = _rows(rows, self.det.state_words, self.device)
        if r.shape[0] < 1:
            raise ValueError("no roots")
        live = running(r)
        cps = torch.unique(current_player(r)[live]).tolist()
        if len(cps) > 1:
            raise ValueError(f"all roots must have the same current player, got seats {cps}")
        if seat is not None and cps and cps[0] != int(seat):
            raise ValueError(f"the roots' current player is seat {cps[0]}, not seat {seat}")
        return r, blueprint, live, cps

    def _nothing(self, m, Cn, dev, compared):
        """The result when no root is running: nothing to play."""
        z = torch.zeros((m, Cn), dtype=torch.int64, device=dev)
        res = SearchResult(torch.full((m, Cn), float("nan"), device=dev), z, z.int(), torch.full((m,), -1, dtype=torch.int32, device=dev),
                           0, 0)
        if compared:
            res.diff = torch.full((m, Cn), float("nan"), dtype=torch.float64, device=dev)
            res.se, res.n_pair = res.diff.clone(), torch.zeros(m, dtype=torch.int32, device=dev)
        return res

    def _run(self, roots, cand, filler, R, draw, first_row_id, first_game_id, base_slot, history):
        """The search itself, for run() and run_candidates() alike (arguments checked): determinize the roots R times, lay the
        replicas out as the [m, C, R] games of this size's env (hb_search_layout), play them to the end with the blueprint, reduce
        the final scores per slot (hb_search_reduce) and, with a base_slot, compare the slots to it (hb_search_compare). The
        result's cand and best_uid stay None."""
        r, blueprint, live, cps = roots
        (m, Cn), dev = cand.shape, r.device
        b = self._setup(m, Cn, R, first_game_id, dev)
        if not cps:
            res = self._nothing(m, Cn, dev, compared=base_slot is not None)
            res.horizon = self.horizon
            return res
        cp, env = int(cps[0]), b["env"]
        H, leaves = self.horizon, 0
        if H is not None:   # (before anything is played: the agent that values a leaf must be able to)
            valuers = leaf_agents(blueprint, self.leaf, seats=((cp + H) % self.players,))
        n_surv = fallback = depth_used = ess = sample = None
        self.last_belief, self.last_exact = "sampled", None
        with torch.cuda.device(dev):
            if history is None:
                self.det.sample(r, seat=cp, replicas=R, seed=self.seed, draw=draw, first_row_id=first_row_id,
                                out=(b["det_rows"], b["weights"]))
            elif isinstance(history, TrackedRows):
                history.take(m, R, (b["det_rows"], b["weights"]))
                n_surv, fallback, depth_used, ess = history.n_surv, history.fallback, history.depth_used, history.ess
            else:   # a PartnerHistory or a LastMove
                if self.exact:
                    from .exact import exact_supported
                if self.exact and exact_supported(blueprint, self.players, epsilon=self.epsilon):
                    sample = self._sample_exact(b, r, history, blueprint, cp, R, draw, first_row_id)
                else:
                    if self.cdet is None:
                        self.cdet = ConditionedDeterminizer(config=self.cfg)
                    sample = self.cdet.sample_history(
                        r, history, blueprint[(cp - 1) % self.players], cp, R, self.oversample, self.seed, draw, history.partner_seed,
                        history.first_game_id, first_row_id=first_row_id, out=(b["det_rows"], b["weights"]), epsilon=self.epsilon)
                # (the result of a last-move history keeps its public shapes: n_surv [m], no depth_used)
                n_surv, depth_used = (sample.n_surv[0], None) if isinstance(history, LastMove) else (sample.n_surv, sample.depth_used)
                fallback, ess = sample.fallback, sample.ess
            belief = belief_score(self.cfg, r, b["det_rows"], b["weights"], cp, R) if self.score_belief else None
            # [m, C, R]: block c of root i holds the same R replicas. A slot without a candidate (an illegal action, in run()) is
            # never counted (done up front); its games move in step with the others on the root's filler move, so that no illegal
            # move reaches the env
            search_layout(self.cfg, b["det_rows"], b["weights"], cand, filler, R, out=(b["rows"], b["forced"], b["done"], b["n_played"]))
            b["final_score"].zero_()
            b["length"].zero_()
            b["counters"].zero_()
            b["counters"][0] = b["n_played"].sum()
            scores, weights = b["final_score"].view(m, Cn, R), b["weights"].view(m, R)
            # enqueued ahead of the rollouts, read after them: games played, dead replicas of the running roots, running roots
            counts = torch.stack([b["counters"][0], (live.view(m, 1) & (weights == 0)).sum(), live.sum()])
            slots = (cand >= 0).to(torch.int8)
            # a blueprint of rule lists, no horizon: one hb_rule_playout launch on b["rows"] instead of the env and the loop
            fast = self.playout and playout_supported(blueprint, horizon=H)
            self.last_path = "playout" if fast else "loop"
            illegal0 = 0
            if not fast:
                env.import_state(b["rows"])
                illegal0 = env.illegal_count()
            turns = rollout(env, self.cfg, blueprint, self.seed, cp, b["forced"], b["done"], b["final_score"], b["length"],
                            b["counters"], b["act"], b["scratch"], self.check_every, horizon=H, playout=fast, rows=b["rows"])
            if H is not None:
                turns, leaves = turns
            illegal = 0 if fast else env.illegal_count() - illegal0
            if illegal:
                raise RuntimeError(f"{illegal} illegal moves in the rollouts (a candidate that is illegal at its root, or the blueprint's)")
            if leaves:   # games cut short by the horizon: every game's value in quarter points, where the final scores were read
                scores = self._leaves(b, valuers, (cp + turns) % self.players, m, Cn, R, draw, first_row_id)
            value, wsum, n_live, best = search_reduce(scores, weights, slots)
            rollouts, dead, roots = counts.tolist()
            res = SearchResult(value, wsum, n_live, best, rollouts, turns, dead=dead, replicas=roots * R, n_surv=n_surv,
                               fallback=fallback, depth_used=depth_used, ess=ess, belief=belief, sample=sample, horizon=H, leaves=leaves)
            if base_slot is not None:
                res.diff, res.se, res.n_pair = search_compare(scores, weights, cand, base_slot)
            if leaves:   # quarter points -> points: a division by a power of two, exact
                res.value = value / LEAF_SCALE
                if base_slot is not None:
                    res.diff, res.se = res.diff / LEAF_SCALE, res.se / LEAF_SCALE
        return res

    def _leaves(self, b, valuers, seat, m, Cn, R, draw, first_row_id):
        """The leaf step (class docstring) on the rollout env of `b` as the horizon left it, `seat` to act in every running game ->
        the quarter-point buffer [m, C, R] int8 of this size (built by the first search that reaches a leaf)."""
        env, A = b["env"], self.num_actions
        leaf4 = b.get("leaf4")
        if leaf4 is None:
            leaf4 = b["leaf4"] = torch.empty((m, Cn, R), dtype=torch.int8, device=env.device)
        q = None
        if valuers != "score":
            agent = valuers[seat]
            q = agent.eval_q((env, (env.net_obs, env.legal)), scratch=b["scratch"].setdefault(agent, {})).view(m, Cn, R, A)
        u = leaf_dither(self.seed, draw, first_row_id, m, R, device=env.device)
        return search_leaf(b["done"].view(m, Cn, R), b["final_score"].view(m, Cn, R), env.score.view(m, Cn, R), q,
                           env.legal.view(m, Cn, R, A), u, self.max_score, out=leaf4)

    @torch.no_grad()
    def run(self, rows, legal, blueprint, draw, seat=None, baseline=None, history=None):
        """rows [m, state_words] int32 state rows (hb_env_export_state), legal [m, A] int8 the legal mask of each root's seat to
        act, blueprint: one agent per seat with eval_moves, draw: Philox draw of the determinization (with the search's seed).
        All running roots must have the same current player (`seat`, when given, must be that player). baseline: optional [m]
        int32 uids (the blueprint's moves): the result's diff / se / n_pair are then every action's paired difference to it.
        history: see the class docstring."""
        roots = self._roots(rows, blueprint, seat)
        r = roots[0]
        dev = r.device
        m, A = r.shape[0], self.num_actions
        if history is not None and not isinstance(history, (PartnerHistory, TrackedRows, LastMove)):
            history = _history(history, m, self.det.state_words, dev)
        lg = torch.as_tensor(legal).to(device=dev, dtype=torch.int8).contiguous()
        if lg.shape != (m, A):
            raise ValueError(f"legal has shape ({m}, {A}), got {tuple(lg.shape)}")
        if baseline is not None:
            baseline = torch.as_tensor(baseline).to(device=dev, dtype=torch.int32).contiguous()
            if baseline.shape != (m,):
                raise ValueError(f"baseline has shape ({m},), got {tuple(baseline.shape)}")
        if self._uid is None:
            self._uid = torch.arange(A, dtype=torch.int32, device=dev).view(1, A)
        # run_candidates() with every legal action as the candidate of its own slot (slot = uid: the baseline is its own slot)
        lgb = lg != 0
        cand = torch.where(lgb, self._uid, -1).int().contiguous()
        filler = lgb.int().argmax(1).int()   # the root's lowest legal uid
        return self._run(roots, cand, filler, self.replicas, draw, 0, self.first_game_id, baseline, history)

    @torch.no_grad()
    def run_candidates(self, rows, cand, filler, blueprint, draw, replicas=None, first_row_id=0, first_game_id=None, base_slot=None,
                       history=None):
        """run() over a candidate list: cand [m, C] int32 (C <= 64) holds the uids to play first at each root (-1: no candidate
        in this slot; a candidate must be legal at its root), filler [m] int32 the move that the games of empty slots make (the
        root's lowest legal uid). replicas: per candidate (default: the search's); first_row_id: row id of replica 0 of root 0
        (keys the determinization, with the search's seed and `draw`); first_game_id: game id of rollout game 0 (default: the
        search's). The result's second axis is the slot: `best` is the best slot, `best_uid` its uid, `cand` the list. base_slot:
        optional [m] int32 slot of each root's baseline (-1: none): fills diff / se / n_pair (hb_search_compare). history: see
        the class docstring (the candidates' row ids then start at first_row_id and take replicas * oversample per root)."""
        roots = self._roots(rows, blueprint, None)
        dev = roots[0].device
        m = roots[0].shape[0]
        if history is not None and not isinstance(history, (PartnerHistory, TrackedRows, LastMove)):
            history = _history(history, m, self.det.state_words, dev)
        R = self.replicas if replicas is None else int(replicas)
        if R < 1:
            raise ValueError(f"replicas must be >= 1, got {replicas}")
        cand = torch.as_tensor(cand).to(device=dev, dtype=torch.int32).contiguous()
        if cand.dim() != 2 or cand.shape[0] != m or not 1 <= cand.shape[1] <= 64:
            raise ValueError(f"cand has shape ({m}, C) with C in 1..64, got {tuple(cand.shape)}")
        filler = torch.as_tensor(filler).to(device=dev, dtype=torch.int32).contiguous()
        if filler.shape != (m,):
            raise ValueError(f"filler has shape ({m},), got {tuple(filler.shape)}")
        if base_slot is not None:
            base_slot = torch.as_tensor(base_slot).to(device=dev, dtype=torch.int32).contiguous()
            if base_slot.shape != (m,):
                raise ValueError(f"base_slot has shape ({m},), got {tuple(base_slot.shape)}")
        res = self._run(roots, cand, filler, R, draw, int(first_row_id),
                        self.first_game_id if first_game_id is None else int(first_game_id), base_slot, history)
        res.cand = cand
        res.best_uid = torch.where(res.best >= 0, cand.gather(1, res.best.long().clamp(min=0).view(m, 1)).view(m), res.best)
        return res

    @torch.no_grad()
    def confirm(self, rows, legal, blueprint, draw, baseline, challenger, replicas, history=None):
        """The second stage of screen-then-confirm: re-measure {baseline[i], challenger[i]} (uids, [m] int32) of every root on
        `replicas` replicas that run() did not see, and compare the two on those alone: slot 0 is the baseline, slot 1 the
        challenger, diff[:, 1] / se[:, 1] the challenger's paired difference to the baseline. A root plays nothing (both slots
        -1, diff and se NaN) when it has no challenger (< 0), the challenger is the baseline, either move is illegal, or it is
        not running. Fresh randomness by construction: the replicas' row ids start behind run()'s (m * self.replicas), the
        rollout games' ids behind run()'s (first_game_id + m * A * self.replicas). With a history the row ids start behind run()'s
        candidates instead (m * self.replicas * self.oversample)."""
        r = _rows(rows, self.det.state_words, self.device)
        dev = r.device
        m, A = r.shape[0], self.num_actions
        lg = torch.as_tensor(legal).to(device=dev, dtype=torch.int8).contiguous()
        if lg.shape != (m, A):
            raise ValueError(f"legal has shape ({m}, {A}), got {tuple(lg.shape)}")
        pair = []
        for name, x in (("baseline", baseline), ("challenger", challenger)):
            x = torch.as_tensor(x).to(device=dev, dtype=torch.int32).contiguous()
            if x.shape != (m,):
                raise ValueError(f"{name} has shape ({m},), got {tuple(x.shape)}")
            pair.append(x)
        bl, ch = pair
        lgb = lg != 0
        is_legal = lambda u: (u >= 0) & (u < A) & lgb.gather(1, u.long().clamp(0, A - 1).view(m, 1)).view(m)
        ok = running(r) & (ch != bl) & is_legal(bl) & is_legal(ch)
        cand = torch.where(ok.view(m, 1), torch.stack([bl, ch], 1), -1).int().contiguous()
        if isinstance(history, TrackedRows):   # the particles behind run()'s
            history = history.shifted(self.replicas)
        return self.run_candidates(r, cand, lgb.int().argmax(1).int(), blueprint, draw, replicas=replicas,
                                   first_row_id=m * self.replicas * (1 if history is None else self.oversample),
                                   first_game_id=self.first_game_id + m * A * self.replicas,
                                   base_slot=torch.zeros(m, dtype=torch.int32, device=dev), history=history)


class SearchPlayer:
    """An agent for Evaluator.run that plays seat `seat` by search over `blueprint` (one agent per seat):

        Evaluator(...).run([SearchPlayer(team, 0), team[1]])

    Its move per game is the blueprint's own move b unless value[best] - value[b] > threshold and both have live replicas
    (SPARTA's deviation rule); finished games and roots without a live replica get the blueprint's move. The blueprint's move is
    computed with the caller's seed and draw, exactly as Evaluator.run(blueprint) would; the search uses this player's `seed`
    and the caller's draw.

    z, confirm_replicas (defaults None, 0: the rule above alone) add a test on the paired difference d of the two moves' scores,
    replica by replica, and its standard error (hb_search_compare). The challenger is `best` where the rule above holds.
    confirm_replicas = 0: it is played iff d > z * se on the search's own replicas. confirm_replicas > 0 (screen, then confirm):
    {b, challenger} are re-measured on that many fresh replicas (RolloutSearch.confirm) and the challenger is played iff
    d > z * se on those alone (z = None counts as 0 there): the estimate that picked the challenger is not the one that tests
    it. A standard error that is not finite (fewer than two live replicas) never deviates.
    z stays None by default. Measured on Full, 2 players, [Piers, Piers], 1 024 games (DESIGN.md section 11f's table,
    profiles/search/confirm_probe.json): z = 2 is the setting to try first — with both seats searching at 32 replicas it scores
    19.32 where the threshold alone scores 16.45 (blueprint 17.20), at the same cost; confirm_replicas = 256 with z = 2 scores
    19.81 for 1.75 times the rollouts, z = 2 at 128 replicas 20.01 for four times.

    condition=True (2 players; default False): the belief of every stage is conditioned on the partner's last move
    (ConditionedDeterminizer, `oversample` candidates per replica). After each call the player remembers
    the rows it searched and the move it finally played; on the next call it rebuilds the state the partner moved from (those
    rows stepped with that move in a scratch env) and hands it to the search with the caller's seed and draw - 1 — what the
    partner's eval_moves was called with —, assuming the partner plays blueprint[partner] on the caller's random stream. A root
    is conditioned only if the remembered call was on the same env object at draw - 2, the game was running then and is
    running now, and word 2 of its row names the partner as the last mover; every other root (a seat's first move of a game
    among them) is searched unconditioned.

    depth=L (1..8, default 1: the rule above, unchanged; L > 1 needs condition=True): the belief is conditioned on the partner's
    last L moves (ConditionedDeterminizer.sample_history). The player keeps a `PartnerHistory`: on each call it takes the move it
    remembered playing at draw - 2 out of the stored alive masks (own_move), rebuilds S_prev as above and pushes it with
    draw - 1 and the validity rule above; where the remembered call is not on the same env at draw - 2 the stack is cleared
    first. A root whose deepest filter leaves no survivor takes the deepest that does: `last_result.depth_used` says which, and
    that is a fallback, not the exact posterior given L moves. depth_stats() gives the sums per depth.

    epsilon (default None: the exact-match filter above, unchanged; needs condition=True): the partner is read as epsilon-greedy
    on blueprint[partner] (RolloutSearch's epsilon, hb_belief_select_soft): the candidates of a conditioned root are weighed, not
    filtered, every usable move counts (`depth_used` = their number, `fallbacks` stays 0, `survivors` counts the candidates that
    reproduce all of them) and depth_stats() gains `ess`, the mean effective sample size of the conditioned roots' candidates.

    Counters: `moves` (moves made in live games), `deviations` (those that left the blueprint), `dead_replicas` /
    `replicas_drawn` (of the first stage), `confirmed` (challengers that went to the second stage), `rejected` (of those, the
    ones not played), `rollouts` (games played, both stages); with condition=True, of the first stage: `conditioned` (live roots
    searched with the filter), `unconditioned` (live roots without), `survivors` / `candidates` (sums over the conditioned
    roots), `fallbacks` (conditioned roots without a survivor), `depth_used` (sum over the conditioned roots of the number of
    partner moves their replicas reproduce: 1 per root that did not fall back at depth 1; with depth > 1 `survivors` counts the
    candidates that pass the filter of the depth used).

    track=True (default False: nothing is allocated and the player is the one above bit for bit; needs condition=True): the
    belief is tracked across turns instead of rebuilt at each (`TrackedBelief`, hb_belief_carry): the
    replicas * oversample hand samples of my last turn are carried, weighed by the one move the partner has made since and
    resampled; the first `replicas` of them are searched, the next `confirm_replicas` confirm (so replicas + confirm_replicas <=
    replicas * oversample). A root without particles, without a usable previous turn or without one particle that explains what
    was seen starts over from the belief above (depth, epsilon, replicas * oversample candidates). TRACK_COUNTERS: `tracked` (live
    roots that carried), `restarts` (live roots that started over; tracked + restarts = conditioned + unconditioned = moves),
    `carried_live` (live particles after the carry, summed over the tracked roots). `conditioned` then counts the tracked roots
    and the restarted ones whose belief was filtered, `survivors` the particles (or candidates) that reproduce the partner's move,
    `depth_used` 1 per tracked root; depth_stats() gains `carried_ess`, the mean effective sample size of the tracked roots'
    weighed particles, and its per-depth sums are not kept. belief_stats() also splits by `tracked` / `restarted`.

    score_belief (default False: nothing is computed or allocated, and the moves played are the same bits either way): every
    first-stage search scores its replicas against the real hands (RolloutSearch's score_belief, hb_belief_score) and the player
    adds the sums up on the device; belief_stats() gives the means.

    horizon, leaf (defaults None: rollouts to the end, the player above bit for bit): RolloutSearch's depth-limited rollouts, in
    both stages. The seat whose agent values the leaves is (seat + horizon) % P; with leaf=None it is the blueprint's own agent of
    that seat and must have eval_q (TypeError here, at construction). `leaf_games` totals the rollout games valued at the horizon.

    exact, max_hands (defaults False, None: the player above bit for bit; exact=True needs condition=True): RolloutSearch's exact
    belief, in both stages. With a blueprint of two `RulebasedAgent`s and neither epsilon nor track, every conditioned root's
    replicas are drawn from the enumerated posterior given the partner's last `depth` moves; a root with more than max_hands hands
    takes the sampled path. `last_belief` says which ran; depth_stats() gains `exact_roots`, `too_large_roots` (together the
    first stage's conditioned roots) and `exact_hands` (the hands walked for the former)."""

    COUNTERS =("moves", "deviations", "confirmed", "rejected", "conditioned", "unconditioned", "survivors", "candidates", "fallbacks",
                "depth_used")
    TRACK_COUNTERS = ("tracked", "restarts", "carried_live")

    def __init__(self, blueprint, seat, replicas=32, threshold=0.0, seed=1, check_every=8, z=None, confirm_replicas=0,
                 condition=False, oversample=8, depth=1, epsilon=None, score_belief=False, track=False, horizon=None, leaf=None,
                 playout=False, exact=False, max_hands=None):
        self.blueprint = list(blueprint)
        self.seat = int(seat)
        if not isinstance(exact, bool):
            raise TypeError(f"exact is a switch (True or False), got {exact!r}")
        if exact and not condition:
            raise ValueError("exact=True needs condition=True")
        if max_hands is not None and int(max_hands) < 1:
            raise ValueError(f"max_hands must be >= 1, got {max_hands}")
        self.exact, self.max_hands = exact, None if max_hands is None else int(max_hands)
        if not isinstance(playout, bool):
            raise TypeError(f"playout is a switch (True or False), got {playout!r}")
        self.playout = playout   # RolloutSearch's: rule-list blueprints without a horizon roll out in one launch per search
        if not 0 <= self.seat < len(self.blueprint):
            raise ValueError(f"seat {seat} out of range for {len(self.blueprint)} players")
        self.horizon, self.leaf = check_horizon(horizon), leaf
        if self.horizon is not None:   # the one seat that can be to act at a leaf of this player's searches
            leaf_agents(self.blueprint, leaf, seats=((self.seat + self.horizon) % len(self.blueprint),))
        elif leaf is not None:
            raise ValueError("leaf= values the games a horizon cuts short: it needs horizon=H")
        self.own = self.blueprint[self.seat]
        for a in self.blueprint:
            if not hasattr(a, "eval_moves"):
                raise TypeError(f"{type(a).__name__} has no eval_moves()")
        self.replicas, self.threshold, self.seed, self.check_every = int(replicas), float(threshold), int(seed), int(check_every)
        self.z = None if z is None else float(z)
        if self.z is not None and not self.z >= 0:
            raise ValueError(f"z must be >= 0 (or None), got {z}")
        self.confirm_replicas = int(confirm_replicas)
        if self.confirm_replicas < 0:
            raise ValueError(f"confirm_replicas must be >= 0, got {confirm_replicas}")
        self.condition, self.oversample = bool(condition), int(oversample)
        if self.oversample < 1:
            raise ValueError(f"oversample must be >= 1, got {oversample}")
        if self.condition and len(self.blueprint) != 2:
            raise ValueError(f"condition=True is built for 2 players, got {len(self.blueprint)}")
        self.depth = int(depth)
        if not 1 <= self.depth <= MAX_DEPTH:
            raise ValueError(f"depth must be in 1..{MAX_DEPTH}, got {depth}")
        if self.depth > 1 and not self.condition:
            raise ValueError(f"depth={depth} needs condition=True")
        self.epsilon = None if epsilon is None else float(epsilon)
        if self.epsilon is not None:
            if not self.condition:
                raise ValueError(f"epsilon={epsilon} needs condition=True")
            soft_table(self.epsilon, 1)   # (the range check)
            if self.replicas * self.oversample > MAX_SOFT_CANDIDATES:
                raise ValueError(f"the soft filter takes at most {MAX_SOFT_CANDIDATES} candidates per root, got replicas * oversample = "
                                 f"{self.replicas * self.oversample}")
        if not isinstance(score_belief, bool):
            raise TypeError(f"score_belief is a switch (True or False), got {score_belief!r}")
        self.score_belief = score_belief
        if not isinstance(track, bool):
            raise TypeError(f"track is a switch (True or False), got {track!r}")
        if track:
            if not self.condition:
                raise ValueError("track=True needs condition=True")
            if self.replicas * self.oversample > MAX_SOFT_CANDIDATES:
                raise ValueError(f"the soft filter takes at most {MAX_SOFT_CANDIDATES} candidates per root, got replicas * oversample = "
                                 f"{self.replicas * self.oversample}")
            if self.replicas + self.confirm_replicas > self.replicas * self.oversample:
                raise ValueError(f"track=True searches and confirms on particles of one set: replicas + confirm_replicas = "
                                 f"{self.replicas + self.confirm_replicas} exceeds replicas * oversample = {self.replicas * self.oversample}")
        self.track = track
        self._tracked = None   # track: the TrackedBelief of the env of the last call
        self._history = None   # depth > 1: the PartnerHistory of the env of the last call
        self._search = None
        self.last_result = None   # the SearchResult of the last call's first stage
        self.last_belief = None   # RolloutSearch's, of the last call's first stage: "exact", "mixed" or "sampled"
        self._memory = None   # condition: (env, draw, rows, moves played) of the last call
        self._prev_env = None  # condition: the scratch env that rebuilds the partner's state
        self.reset_stats()

    def requires_vectorized_observation(self):
        return self.own.requires_vectorized_observation()

    def reset_stats(self):
        self._stats = None   # [len(COUNTERS)] int64 on the device, built by the first eval_moves: read through the properties
        self.dead_replicas = self.replicas_drawn = self.searches = self.rollouts = 0
        self.leaf_games = 0   # horizon: rollout games valued at the horizon instead of played out (both stages)
        self._by_depth = None   # depth > 1: [4, depth] int64 on the device, see depth_stats()
        self._ess = None        # epsilon: [2] float64 on the device, sum of ess and count over the conditioned roots
        self._belief = None     # score_belief: [2, len(BeliefScore.SUMS), H] float64 on the device (conditioned roots, the others)
        self._track_stats = None    # track: [len(TRACK_COUNTERS)] int64 on the device
        self._track_ess = None      # track: [2] float64 on the device, sum of ess and count over the tracked roots
        self._belief_track = None   # track and score_belief: the sums of _belief, split (tracked roots, restarted roots)
        self._exact_stats = None    # exact: [3] int64 on the device, see depth_stats()

    def belief_stats(self):
        """score_belief: the first stage's beliefs against the real hands since reset_stats(), over every live root searched:
        belief_figures' dict (`cards`, `roots`, `hit_rate`, `prior_rate`, `joint_rate`, `cross_entropy`, `prior_cross_entropy`,
        `by_slot`). With condition=True it also holds the same dict for the `conditioned` roots (fallback != 2) and for the
        `unconditioned` ones. All zeros before the first call (and without score_belief)."""
        out = belief_stats_of(self._belief, self.condition)
        if self.track:   # the same figures over the roots that carried their particles and over those that started over
            for j, name in enumerate(("tracked", "restarted")):
                out[name] = belief_figures(None if self._belief_track is None else self._belief_track[j])
        return out

    def belief_sums(self):
        """score_belief: the sums behind belief_stats(), [2 (conditioned roots, the others), len(BeliefScore.SUMS), H] float64 on
        the device (None before the first call): several players' sums add up, and `belief_stats_of` gives the figures."""
        return self._belief

    def depth_stats(self):
        """depth > 1: sums over the first stage's conditioned roots since reset_stats(), one figure per D = 1 .. depth:
        `reached` (roots with at least D usable partner moves), `survivors` (over those roots, the candidates that reproduce
        the last D moves), `used` (roots whose replicas reproduce exactly D moves) and `shallow` (roots with exactly D usable
        moves that use fewer: the deepest filter left no survivor; roots without any survivor among them)."""
        t = torch.zeros((4, self.depth), dtype=torch.int64) if self._by_depth is None else self._by_depth.cpu()
        out = dict(zip(("reached", "survivors", "used", "shallow"), t.tolist()))
        if self.epsilon is not None:   # the mean effective sample size of the conditioned roots' candidates (0.0: none yet)
            total, count = (0.0, 0.0) if self._ess is None else self._ess.tolist()
            out["ess"] = total / count if count else 0.0
        if self.track:   # the mean effective sample size of the tracked roots' carried, weighed particles
            total, count = (0.0, 0.0) if self._track_ess is None else self._track_ess.tolist()
            out["carried_ess"] = total / count if count else 0.0
        if self.exact:   # of the first stage's conditioned roots: enumerated, over max_hands (sampled instead), hands walked
            ex = [0, 0, 0] if self._exact_stats is None else self._exact_stats.tolist()
            out.update(exact_roots=int(ex[0]), too_large_roots=int(ex[1]), exact_hands=int(ex[2]))
        return out

    def _previous(self, env, rows, draw):
        """history for this call: the remembered rows stepped with the remembered moves, and which roots that is usable for."""
        m, dev = rows.shape[0], rows.device
        partner = 1 - self.seat
        mem = self._memory
        if mem is None or mem[0]() is not env or mem[1] != int(draw) - 2 or mem[2].shape != rows.shape:
            return rows, torch.zeros(m, dtype=torch.uint8, device=dev)
        _, _, then_rows, then_moves = mem
        pe = self._prev_env
        if pe is None or pe.n != m or pe.device != dev or pe.cfg.players != env.cfg.players:
            pe = self._prev_env = HanabiEnv(config=eval_config(None, None, env.cfg), n_games=m, device=dev, packed=True)
        pe.import_state(then_rows)
        pe.step(then_moves)
        prev = pe.export_state()
        w2 = rows[:, 2]   # the last move of this deal: bit 0 set once there is one, bits 1-3 the seat that made it
        partner_moved_last = ((w2 & 1) != 0) & (((w2 >> 1) & 7) == partner)
        valid = running(then_rows) & running(rows) & partner_moved_last & running(prev) & (current_player(prev) == partner)
        return prev, valid.to(torch.uint8)

    def _stack(self, env, rows, seed, draw, prev, valid):
        """depth > 1: the PartnerHistory for this call. The move remembered from draw - 2 leaves the stored alive masks, then
        (prev, valid) of _previous goes on top; a remembered call that is not this env's at draw - 2 empties the stack first."""
        m, dev = rows.shape[0], rows.device
        mem, h = self._memory, self._history
        same = mem is not None and mem[0]() is env and mem[1] == int(draw) - 2 and mem[2].shape == rows.shape
        if h is None or h.m != m or h.alive.device != dev or h.state_words != rows.shape[1]:
            h = self._history = PartnerHistory(eval_config(None, None, env.cfg), m, self.depth, dev)
        h.partner_seed, h.first_game_id = int(seed), env.first_game_id
        if not same:   # (nothing to push either: _previous found no usable previous state for any root)
            h.clear()
            return h
        h.own_move(mem[3])
        h.push(prev, last_move_uid(env.cfg, rows), int(draw) - 1, valid, seat=self.seat)
        return h

    def _carry(self, env, rows, seed, draw, prev, valid, stack):
        """track: this call's TrackedRows. The particle sets of the call remembered from draw - 2 are carried; a remembered call
        that is not this env's at draw - 2 forgets them first (every root then starts over)."""
        mem, tb = self._memory, self._tracked
        if tb is None or tb.cfg.players != env.cfg.players or (tb.rows is not None and tb.rows.device != rows.device):
            tb = self._tracked = TrackedBelief(config=eval_config(None, None, env.cfg), replicas=self.replicas, oversample=self.oversample)
        same = mem is not None and mem[0]() is env and mem[1] == int(draw) - 2 and mem[2].shape == rows.shape
        if not same:
            tb.clear()
        return tb.step(rows, mem[2] if same else None, mem[3] if same else None, prev, valid, self.blueprint[1 - self.seat], self.seat,
                       self.seed, draw, int(seed), int(draw) - 1, env.first_game_id, epsilon=self.epsilon, history=stack)

    def _significant(self, diff, se, z):
        """diff > z * se, never with a standard error that is not finite (0 * inf must not pass) or a NaN."""
        return torch.isfinite(se) & (diff > z * se)

    @torch.no_grad()
    def eval_moves(self, observations, seed, draw, actions_out, scratch=None):
        env = observations[0] if isinstance(observations, (tuple, list)) else observations
        if not hasattr(env, "h"):
            raise TypeError("SearchPlayer reads the env's state rows: pass (env, (obs, legal)) or the HanabiEnv itself")
        if env.color_shuffled:
            raise ValueError("search on a colour-shuffled env is not supported: the rollout env's game ids would draw other "
                             "permutations (DESIGN.md section 11f)")
        if self.own.requires_vectorized_observation():   # (the caller's observation and scratch, as it handed them over)
            self.own.eval_moves(observations, seed, draw, actions_out, scratch=scratch)
        else:
            self.own.eval_moves(env, seed, draw, actions_out)
        if self.condition and env.cfg.players != 2:
            raise ValueError(f"condition=True is built for 2 players, the env has {env.cfg.players}")
        if self._search is None or self._search.cfg.players != env.cfg.players:
            self._search = RolloutSearch(config=env.cfg, replicas=self.replicas, seed=self.seed, device=env.device,
                                         check_every=self.check_every, oversample=self.oversample, epsilon=self.epsilon,
                                         score_belief=self.score_belief, horizon=self.horizon, leaf=self.leaf,
                                         playout=self.playout, exact=self.exact, max_hands=self.max_hands)
        rows = env.export_state()
        staged = self.z is not None or self.confirm_replicas > 0
        history = None
        if self.condition:
            prev, valid = self._previous(env, rows, draw)
            if self.depth == 1:
                history = (prev, int(seed), int(draw) - 1, env.first_game_id, valid)
            else:
                history = self._stack(env, rows, seed, draw, prev, valid)
            if self.track:
                history = self._carry(env, rows, seed, draw, prev, valid, history if self.depth > 1 else None)
        res = self._search.run(rows, env.legal, self.blueprint, draw, seat=self.seat,
                               baseline=actions_out if self.z is not None else None, history=history)
        self.last_result = res
        self.last_belief = self._search.last_belief
        if self.exact and self._search.last_exact is not None and res.fallback is not None:
            eb = self._search.last_exact   # (the first stage's: a confirming stage enumerates again)
            cond = running(rows) & (res.fallback != 2)
            done = cond & (eb.status == 0)
            ex = torch.stack([done.sum(), (cond & (eb.status == 1)).sum(), (eb.space * done).sum()])
            self._exact_stats = ex if self._exact_stats is None else self._exact_stats + ex
        if res.belief is not None:   # (None: the switch is off, or no root was running)
            filtered = res.fallback != 2 if self.condition and res.fallback is not None else torch.zeros_like(res.belief.scored)
            sums = torch.stack([res.belief.sums(where=filtered), res.belief.sums(where=~filtered)])
            self._belief = sums if self._belief is None else self._belief + sums
            if self.track:
                split = torch.stack([res.belief.sums(where=history.tracked), res.belief.sums(where=history.restarted)])
                self._belief_track = split if self._belief_track is None else self._belief_track + split
        live = running(rows)
        bp = actions_out.long().clamp(0, env.num_actions - 1).view(-1, 1)
        best = res.best.long().clamp(min=0).view(-1, 1)
        v_bp, v_best = res.value.gather(1, bp), res.value.gather(1, best)
        ok = (res.best.view(-1, 1) >= 0) & (res.n_live.gather(1, bp) > 0) & (res.n_live.gather(1, best) > 0)
        deviate = (ok & ((v_best - v_bp) > self.threshold)).view(-1) & live   # (NaN compares false)
        counts = {}   # this call's share of the device counters
        self.rollouts += res.rollouts
        self.leaf_games += res.leaves
        if staged:
            challenger = deviate & (res.best != actions_out)
            if self.confirm_replicas > 0:
                deviate = torch.zeros_like(challenger)
                if bool(challenger.any().item()):   # (nothing to confirm: no second stage)
                    second = self._search.confirm(rows, env.legal, self.blueprint, draw, actions_out,
                                                  torch.where(challenger, res.best, -1), self.confirm_replicas, history=history)
                    deviate = challenger & self._significant(second.diff[:, 1], second.se[:, 1], self.z or 0.0)
                    self.rollouts += second.rollouts
                    self.leaf_games += second.leaves
                counts.update(confirmed=challenger.sum(), rejected=(challenger & ~deviate).sum())
            else:
                deviate = challenger & self._significant(res.diff.gather(1, best).view(-1), res.se.gather(1, best).view(-1), self.z)
        actions_out.copy_(torch.where(deviate, res.best, actions_out))
        if self.condition:
            self._memory = (weakref.ref(env), int(draw), rows, actions_out.clone())
            if res.fallback is not None:   # (None: no root was running)
                filtered = live & (res.fallback != 2)
                if res.ess is not None and self.epsilon is not None:
                    soft = filtered & history.restarted if self.track else filtered
                    ess = torch.stack([(res.ess.double() * soft).sum(), soft.sum().double()])
                    self._ess = ess if self._ess is None else self._ess + ess
                if self.track:   # (per root already: the carried particles' figures, or those of the belief it started over with)
                    n_surv, used = res.n_surv, res.depth_used.long()
                    t_ess = torch.stack([(res.ess.double() * history.tracked).sum(), history.tracked.sum().double()])
                    self._track_ess = t_ess if self._track_ess is None else self._track_ess + t_ess
                    t_counts = torch.stack([history.tracked.sum(), history.restarted.sum(), history.carried_live.sum()]).long()
                    self._track_stats = t_counts if self._track_stats is None else self._track_stats + t_counts
                else:   # the candidates that pass the filter of the depth used, root by root
                    n_surv, used = res.sample.survivors(), res.sample.depth_used.long()
                    if self.depth > 1:
                        D = torch.arange(1, self.depth + 1, device=rows.device).view(-1, 1)
                        have = ((history.valid != 0) & live.view(1, -1)).long().cumprod(0).sum(0).view(1, -1)   # L_i
                        by_depth = torch.stack([(have >= D).sum(1), (res.n_surv * (have >= D)).sum(1),
                                                ((used.view(1, -1) == D) & filtered).sum(1), ((have == D) & (used.view(1, -1) < D)).sum(1)])
                        self._by_depth = by_depth if self._by_depth is None else self._by_depth + by_depth
                counts.update(conditioned=filtered.sum(), unconditioned=(live & (res.fallback == 2)).sum(),
                              survivors=(n_surv * filtered).sum(), candidates=filtered.sum() * (self.replicas * self.oversample),
                              fallbacks=(filtered & (res.fallback == 1)).sum(), depth_used=(used * filtered).sum())
        counts.update(moves=live.sum(), deviations=deviate.sum())
        if self._stats is None:
            self._stats = torch.zeros(len(self.COUNTERS), dtype=torch.int64, device=rows.device)
        zero = self._stats.new_zeros(())
        self._stats += torch.stack([counts.get(name, zero) for name in self.COUNTERS])
        self.dead_replicas += res.dead
        self.replicas_drawn += res.replicas
        self.searches += 1
        return actions_out


for _j, _name in enumerate(SearchPlayer.COUNTERS):   # the device counters as read-only ints: 0 before the first call
    setattr(SearchPlayer, _name, property(lambda self, j=_j: 0 if self._stats is None else int(self._stats[j].item())))
for _j, _name in enumerate(SearchPlayer.TRACK_COUNTERS):   # track=True's (0 without)
    setattr(SearchPlayer, _name, property(lambda self, j=_j: 0 if self._track_stats is None else int(self._track_stats[j].item())))
