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
* `SearchPlayer` is an agent for `Evaluator.run`: the blueprint's move unless the search finds one that is better by more than
  `threshold`.

Colour-shuffled envs are refused: the rollout env's game ids would draw other permutations than the source's.
"""
import ctypes as C
import weakref

import torch

from . import _capi as K
from .env import HanabiEnv
from .evaluate import max_turns


def _config(game, players, config):
    if config is not None:
        cfg = K.HbConfig(config.players, config.colors, config.ranks, config.hand_size, config.max_info, config.max_life, 0)
    else:
        cfg = K.make_config(game, players, 0)
    if K.lib().hb_config_validate(C.byref(cfg)) != 0:
        raise ValueError(f"invalid configuration {cfg!r}: {K.lib().hb_last_error().decode()}")
    return cfg


def _rows(rows, words, device=None):
    r = torch.as_tensor(rows)
    r = r.to(device=device if device is not None else r.device, dtype=torch.int32).contiguous()
    if r.dim() != 2 or r.shape[1] != words:
        raise ValueError(f"state rows have shape [m, {words}], got {tuple(r.shape)}")
    if not r.is_cuda:
        raise K.HbError("the state rows must live on the GPU (there is no CPU path)")
    return r


class Determinizer:
    """hb_belief_determinize on torch tensors; see the module docstring and include/hanabi_hip.h."""

    def __init__(self, game="Hanabi-Full", players=2, config=None):
        self.cfg = _config(game, players, config)
        self.players = self.cfg.players
        self.state_words = K.lib().hb_state_words(C.byref(self.cfg))

    def sample(self, rows, seat=-1, replicas=32, seed=1, draw=0, first_row_id=0, out=None):
        """rows [m, state_words] int32 (device) -> (rows_out [m * replicas, state_words] int32, weights [m * replicas] int64).
        Row i * replicas + r is replica r of source row i; weight 0 marks a dead replica (an unchanged copy). `out`: an
        optional (rows_out, weights_u32) pair of buffers to write into (weights int32 holding the u32 bits)."""
        r = _rows(rows, self.state_words)
        m, replicas = r.shape[0], int(replicas)
        if out is None:
            rows_out = torch.empty((m * max(replicas, 0), self.state_words), dtype=torch.int32, device=r.device)
            w = torch.empty(m * max(replicas, 0), dtype=torch.int32, device=r.device)
        else:
            rows_out, w = out
            assert rows_out.shape == (m * replicas, self.state_words) and rows_out.dtype == torch.int32 and rows_out.is_contiguous()
            assert w.shape == (m * replicas,) and w.dtype == torch.int32 and w.is_contiguous()
        with torch.cuda.device(r.device):
            K.check(K.lib().hb_belief_determinize(C.byref(self.cfg), K.dptr(r), m, int(seat), replicas, int(seed), int(draw),
                                                  int(first_row_id), K.dptr(rows_out), K.dptr(w), K.current_stream()))
        if out is not None:
            return rows_out, w
        return rows_out, w.long() & 0xFFFFFFFF


def search_reduce(scores, weights, legal):
    """hb_search_reduce: scores [m, A, R] int8, weights [m, R] (u32 bits in int32), legal [m, A] int8 ->
    (value [m, A] f32, wsum [m, A] int64, n_live [m, A] int32, best [m] int32)."""
    m, A, R = scores.shape
    assert scores.dtype == torch.int8 and scores.is_contiguous()
    assert weights.shape == (m, R) and weights.dtype == torch.int32 and weights.is_contiguous()
    assert legal.shape == (m, A) and legal.dtype == torch.int8 and legal.is_contiguous()
    dev = scores.device
    value = torch.empty((m, A), dtype=torch.float32, device=dev)
    wsum = torch.empty((m, A), dtype=torch.int64, device=dev)
    n_live = torch.empty((m, A), dtype=torch.int32, device=dev)
    best = torch.empty(m, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        K.check(K.lib().hb_search_reduce(K.dptr(scores), K.dptr(weights), K.dptr(legal), m, A, R, K.dptr(value), K.dptr(wsum),
                                         K.dptr(n_live), K.dptr(best), K.current_stream()))
    return value, wsum, n_live, best


class SearchResult:
    """value [m, A] f32 (NaN: illegal at the root, or no live replica), wsum [m, A] int64, n_live [m, A] int32, best [m] int32
    (-1: no action has a value), rollouts = games played, turns = turns of the longest rollout, dead = replicas of weight 0
    among the running roots' replicas. Device tensors."""

    def __init__(self, value, wsum, n_live, best, rollouts, turns, dead=0, replicas=0):
        self.value, self.wsum, self.n_live, self.best = value, wsum, n_live, best
        self.rollouts, self.turns, self.dead, self.replicas = int(rollouts), int(turns), int(dead), int(replicas)

    def __repr__(self):
        return f"SearchResult(roots={self.value.shape[0]}, rollouts={self.rollouts}, turns={self.turns})"


def rollout(env, cfg, blueprint, seed, first_seat, forced, done, final_score, length, counters, act, scratch, check_every=8,
            turn_limit=None):
    """Play the games of `env` (auto-reset off, state imported) to the end: turn 0 plays `forced` for seat `first_seat`, turn
    t >= 1 the move of blueprint[(first_seat + t) % P].eval_moves with draw t + 1; hb_eval_tally after every step. `done`
    (bit 0x80: not played) and `counters` ([0] = games live) are set up by the caller. Returns the number of turns played."""
    L, P, n = K.lib(), cfg.players, env.n
    cfg_ref = C.byref(cfg)
    bufs = tuple(K.dptr(t) for t in (env.reward, env.terminal, env.score, done, final_score, length, counters))
    limit = max_turns(cfg) if turn_limit is None else turn_limit
    live, t = -1, 0
    while t < limit:
        seat = (first_seat + t) % P
        if t == 0:
            moves = forced
        else:
            agent, moves = blueprint[seat], act
            if agent.requires_vectorized_observation():
                agent.eval_moves((env, (env.net_obs, env.legal)), seed, t + 1, act, scratch=scratch.setdefault(agent, {}))
            else:
                agent.eval_moves(env, seed, t + 1, act)
        env.step(moves)
        K.check(L.hb_eval_tally(cfg_ref, n, seat, t, K.dptr(moves), *bufs, K.current_stream()))
        t += 1
        if t % check_every == 0 or t == limit:
            live = int(counters[0].item())
            if live == 0:
                break
    if live != 0:
        raise RuntimeError(f"{live} rollout games still live after {limit} turns")
    return t


class RolloutSearch:
    """Value of every root action under `blueprint` by belief-sampled rollouts; see the module docstring.

    first_game_id: global id of rollout game 0 (keys the blueprint's draws, like Evaluator's). The rollout env and every
    buffer are built by the first run() of a size and kept for the next."""

    def __init__(self, game="Hanabi-Full", players=2, replicas=32, seed=1, device=None, config=None, check_every=8, first_game_id=0):
        self.cfg = _config(game, players, config)
        self.players = self.cfg.players
        self.replicas = int(replicas)
        if self.replicas < 1:
            raise ValueError(f"replicas must be >= 1, got {replicas}")
        self.seed = int(seed)
        self.first_game_id = int(first_game_id)
        self.device = device
        self.check_every = max(1, int(check_every))
        self.det = Determinizer(config=self.cfg)
        self.num_actions = K.lib().hb_num_actions(C.byref(self.cfg))
        self.n_counters = K.lib().hb_eval_counters(C.byref(self.cfg))
        self._sized = {}   # m -> buffers of that size
        self._scratch = weakref.WeakKeyDictionary()   # agent -> the buffers its eval_moves writes

    def _setup(self, m, dev):
        b = self._sized.get(m)
        if b is not None:
            return b
        self._sized.clear()   # one size at a time: a rollout env of the old size is memory the new one needs
        A, R, SW = self.num_actions, self.replicas, self.det.state_words
        n = m * A * R
        env = HanabiEnv(config=self.cfg, n_games=n, seed=self.seed, first_game_id=self.first_game_id, device=dev, packed=True)
        b = dict(env=env, det_rows=torch.empty((m * R, SW), dtype=torch.int32, device=dev),
                 weights=torch.empty(m * R, dtype=torch.int32, device=dev),
                 rows=torch.empty((n, SW), dtype=torch.int32, device=dev),
                 forced=torch.empty(n, dtype=torch.int32, device=dev), act=torch.empty(n, dtype=torch.int32, device=dev),
                 done=torch.empty(n, dtype=torch.uint8, device=dev), final_score=torch.empty(n, dtype=torch.int8, device=dev),
                 length=torch.empty(n, dtype=torch.int16, device=dev),
                 counters=torch.empty(self.n_counters, dtype=torch.int64, device=dev),
                 uid=torch.arange(A, dtype=torch.int32, device=dev).view(1, A, 1))
        self._sized[m] = b
        return b

    @torch.no_grad()
    def run(self, rows, legal, blueprint, draw, seat=None):
        """rows [m, state_words] int32 state rows (hb_env_export_state), legal [m, A] int8 the legal mask of each root's seat to
        act, blueprint: one agent per seat with eval_moves, draw: Philox draw of the determinization (with the search's seed).
        All running roots must have the same current player (`seat`, when given, must be that player)."""
        blueprint = list(blueprint)
        if len(blueprint) != self.players:
            raise ValueError(f"one blueprint agent per seat: {self.players} players, {len(blueprint)} agents")
        for a in blueprint:
            if not hasattr(a, "eval_moves"):
                raise TypeError(f"{type(a).__name__} has no eval_moves()")
        r = _rows(rows, self.det.state_words, self.device)
        dev = r.device
        m, A, R = r.shape[0], self.num_actions, self.replicas
        if m < 1:
            raise ValueError("no roots")
        lg = torch.as_tensor(legal).to(device=dev, dtype=torch.int8).contiguous()
        if lg.shape != (m, A):
            raise ValueError(f"legal has shape ({m}, {A}), got {tuple(lg.shape)}")
        w0 = r[:, 0]
        running = ((w0 >> 19) & 3) == 0
        cps = torch.unique(((w0 >> 13) & 7)[running]).tolist()
        if len(cps) > 1:
            raise ValueError(f"all roots must have the same current player, got seats {cps}")
        if seat is not None and cps and cps[0] != int(seat):
            raise ValueError(f"the roots' current player is seat {cps[0]}, not seat {seat}")
        b = self._setup(m, dev)
        if not cps:   # no root is running: nothing to play
            z = torch.zeros((m, A), dtype=torch.int64, device=dev)
            return SearchResult(torch.full((m, A), float("nan"), device=dev), z, z.int(), torch.full((m,), -1, dtype=torch.int32, device=dev),
                                0, 0)
        cp = int(cps[0])
        env = b["env"]
        with torch.cuda.device(dev):
            self.det.sample(r, seat=cp, replicas=R, seed=self.seed, draw=draw, first_row_id=0, out=(b["det_rows"], b["weights"]))
            SW = self.det.state_words
            # [m, A, R]: block a of root i holds the same R replicas
            b["rows"].view(m, A, R, SW).copy_(b["det_rows"].view(m, 1, R, SW).expand(m, A, R, SW))
            lgb = lg != 0
            played = lgb.view(m, A, 1) & (b["weights"].view(m, 1, R) != 0)
            # an illegal action's block is never counted (done up front); its games move in step with the others on the
            # root's lowest legal uid, so that no illegal move reaches the env
            first_legal = lgb.int().argmax(1).int().view(m, 1, 1)
            b["forced"].view(m, A, R).copy_(torch.where(lgb.view(m, A, 1), b["uid"], first_legal).expand(m, A, R))
            b["done"].view(m, A, R).copy_(torch.where(played, 0, 0x80).to(torch.uint8))
            b["final_score"].zero_()
            b["length"].zero_()
            b["counters"].zero_()
            b["counters"][0] = played.sum()
            rollouts = b["counters"][0].clone()
            dead = (running.view(m, 1) & (b["weights"].view(m, R) == 0)).sum()
            env.import_state(b["rows"])
            illegal0 = env.illegal_count()
            turns = rollout(env, self.cfg, blueprint, self.seed, cp, b["forced"], b["done"], b["final_score"], b["length"],
                            b["counters"], b["act"], self._scratch, self.check_every)
            illegal = env.illegal_count() - illegal0
            if illegal:
                raise RuntimeError(f"the blueprint chose {illegal} illegal moves in the rollouts")
            value, wsum, n_live, best = search_reduce(b["final_score"].view(m, A, R), b["weights"].view(m, R), lg)
        return SearchResult(value, wsum, n_live, best, int(rollouts.item()), turns, dead=int(dead.item()), replicas=int(running.sum().item()) * R)


class SearchPlayer:
    """An agent for Evaluator.run that plays seat `seat` by search over `blueprint` (one agent per seat):

        Evaluator(...).run([SearchPlayer(team, 0), team[1]])

    Its move per game is the blueprint's own move b unless value[best] - value[b] > threshold and both have live replicas
    (SPARTA's deviation rule); finished games and roots without a live replica get the blueprint's move. The blueprint's move is
    computed with the caller's seed and draw, exactly as Evaluator.run(blueprint) would; the search uses this player's `seed`
    and the caller's draw. Counters: `moves` (moves made in live games), `deviations` (those that left the blueprint),
    `dead_replicas` / `replicas_drawn`."""

    def __init__(self, blueprint, seat, replicas=32, threshold=0.0, seed=1, check_every=8):
        self.blueprint = list(blueprint)
        self.seat = int(seat)
        if not 0 <= self.seat < len(self.blueprint):
            raise ValueError(f"seat {seat} out of range for {len(self.blueprint)} players")
        self.own = self.blueprint[self.seat]
        for a in self.blueprint:
            if not hasattr(a, "eval_moves"):
                raise TypeError(f"{type(a).__name__} has no eval_moves()")
        self.replicas, self.threshold, self.seed, self.check_every = int(replicas), float(threshold), int(seed), int(check_every)
        self._search = None
        self._moves = self._dev = None
        self.dead_replicas = self.replicas_drawn = self.searches = 0

    def requires_vectorized_observation(self):
        return self.own.requires_vectorized_observation()

    @property
    def moves(self):
        return 0 if self._moves is None else int(self._moves.item())

    @property
    def deviations(self):
        return 0 if self._dev is None else int(self._dev.item())

    def reset_stats(self):
        self._moves = self._dev = None
        self.dead_replicas = self.replicas_drawn = self.searches = 0

    @torch.no_grad()
    def eval_moves(self, observations, seed, draw, actions_out, scratch=None):
        vec = self.own.requires_vectorized_observation()
        env = observations[0] if isinstance(observations, (tuple, list)) else observations
        if not hasattr(env, "h"):
            raise TypeError("SearchPlayer reads the env's state rows: pass (env, (obs, legal)) or the HanabiEnv itself")
        if env.color_shuffled:
            raise ValueError("search on a colour-shuffled env is not supported: the rollout env's game ids would draw other "
                             "permutations (DESIGN.md section 11f)")
        if vec:
            self.own.eval_moves(observations, seed, draw, actions_out, scratch=scratch)
        else:
            self.own.eval_moves(env, seed, draw, actions_out)
        if self._search is None or self._search.cfg.players != env.cfg.players:
            self._search = RolloutSearch(config=env.cfg, replicas=self.replicas, seed=self.seed, device=env.device,
                                         check_every=self.check_every)
        rows = env.export_state()
        res = self._search.run(rows, env.legal, self.blueprint, draw, seat=self.seat)
        live = ((rows[:, 0] >> 19) & 3) == 0
        bp = actions_out.long().clamp(0, env.num_actions - 1).view(-1, 1)
        best = res.best.long().clamp(min=0).view(-1, 1)
        v_bp, v_best = res.value.gather(1, bp), res.value.gather(1, best)
        ok = (res.best.view(-1, 1) >= 0) & (res.n_live.gather(1, bp) > 0) & (res.n_live.gather(1, best) > 0)
        deviate = (ok & ((v_best - v_bp) > self.threshold)).view(-1) & live   # (NaN compares false)
        actions_out.copy_(torch.where(deviate, res.best, actions_out))
        if self._moves is None:
            self._moves = torch.zeros((), dtype=torch.int64, device=rows.device)
            self._dev = torch.zeros((), dtype=torch.int64, device=rows.device)
        self._moves += live.sum()
        self._dev += deviate.sum()
        self.dead_replicas += res.dead
        self.replicas_drawn += res.replicas
        self.searches += 1
        return actions_out
