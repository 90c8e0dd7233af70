"""Training against a mixed pool of fixed partners (ad-hoc teamplay): one seat occupant that is several frozen agents at once.

    pool = PartnerPool([piers, iggi, frozen_dqn])
    sess = SelfPlaySession(env, [dqn, pool], train_seats=[0])
    sess.run(steps); pool.stats(); sess.evaluate_pool()

* Layout. The env's n games are cut into 128-game tiles; member k owns one contiguous run of tiles, in member order, with tile
  counts from `weights` (default equal) rounded by largest remainder (`pool_layout`, a pure function of n and the weights). Every
  member plays every seat the pool holds in its rows: a P-player team is (trainee, member, ..., member).
* One pool turn issues, on the current stream: the launches of its move table (hanabi_hip.grouped) — one
  hb_actor_fused_act_grouped per (dtype, hidden, n_atoms) group of one-kernel DQN members (other tiles inactive), one
  hb_rule_act_blocks for all rule members — and each other member's own eval_moves on its row range (the generic path). The
  table's tiles are filled once and refilled only when a member's eval_operands() addresses change.
* Randomness: Philox seed = the pool's `seed`, draw = the pool's own call counter (1, 2, ...), row r keyed by its global game id
  env.first_game_id + r. No member's draw counter, histogram, noise, buffers or weights move: members are frozen.
* Statistics: after every env step the session issues `tally` (hb_train_tally): one int64 counter row per member, read by
  `stats()`.
"""
import ctypes as C
import math

import torch

from . import _capi as K
from .evaluate import MOVE_KINDS
from .grouped import TILE, MoveTable, RuleSets, classify

MAX_MEMBERS = K.TRAIN_MAX_MEMBERS
FORMAT = "hanabi-agents_amd/partner_pool/1"


def pool_layout(n, weights):
    """[(first tile, tile count)] per member: n / 128 tiles shared by largest remainder of the weights, contiguous, in member
    order (ties go to the earlier member). ValueError: n not a multiple of 128, more members than tiles, a member with no tile."""
    n, w = int(n), [float(x) for x in weights]
    if n < TILE or n % TILE:
        raise ValueError(f"a partner pool needs a positive multiple of {TILE} games, got {n}")
    tiles = n // TILE
    if len(w) > tiles:
        raise ValueError(f"{len(w)} members but only {tiles} tiles of {TILE} games")
    total = sum(w)
    quota = [tiles * x / total for x in w]
    count = [int(math.floor(q)) for q in quota]
    for k in sorted(range(len(w)), key=lambda k: (-(quota[k] - count[k]), k))[:tiles - sum(count)]:
        count[k] += 1
    for k, c in enumerate(count):
        if c == 0:
            raise ValueError(f"member {k} gets no tile of {TILE} games (weight {w[k]} of {total}, {tiles} tiles)")
    out, first = [], 0
    for c in count:
        out.append((first, c))
        first += c
    return out


def _fingerprint(m):
    from hanabi_agents.rule_based import RulebasedAgent

    if isinstance(m, RulebasedAgent):
        return ("rule", [(r.kind, r.arg, float(r.threshold)) for r in m.rules])
    p = m.params
    return ("dqn", int(m.obs_len), [int(x) for x in p.layers], int(p.n_atoms) if getattr(m, "distributional", True) else 0,
            str(p.compute_dtype))


class PartnerStats:
    """One member's counts since the session started (or reset_stats()): episodes ended in its rows, their mean score and its
    standard error, the score histogram, bomb-out rate and mean length (over the episodes whose deal the tally saw), and the
    moves [P, 4] (MOVE_KINDS) and misplays [P] of every seat in those rows."""

    def __init__(self, row, players, bins):
        row = [int(x) for x in row]
        B, P = bins, players
        self.episodes = row[0]
        self.score_sum, self.score_sq_sum = row[1], row[2]
        self.histogram = torch.tensor(row[3:3 + B], dtype=torch.int64)
        self.bombouts, self.length_sum, self.tracked = row[3 + B], row[4 + B], row[5 + B]
        self.moves = torch.tensor(row[6 + B:6 + B + 4 * P], dtype=torch.int64).view(P, 4)
        self.misplays = torch.tensor(row[6 + B + 4 * P:6 + B + 5 * P], dtype=torch.int64)

    @property
    def mean(self):
        return self.score_sum / self.episodes if self.episodes else float("nan")

    @property
    def stderr(self):
        n = self.episodes
        if n < 2:
            return 0.0 if n == 1 else float("nan")
        var = (self.score_sq_sum - self.score_sum * self.score_sum / n) / (n - 1)
        return math.sqrt(max(var, 0.0) / n)

    @property
    def bombout_rate(self):
        return self.bombouts / self.tracked if self.tracked else float("nan")

    @property
    def mean_length(self):
        return self.length_sum / self.tracked if self.tracked else float("nan")

    def as_dict(self):
        return dict(episodes=self.episodes, mean=self.mean, stderr=self.stderr, histogram=self.histogram.tolist(),
                    bombout_rate=self.bombout_rate, mean_length=self.mean_length,
                    moves=[dict(zip(MOVE_KINDS, r)) for r in self.moves.tolist()], misplays=self.misplays.tolist())

    def __repr__(self):
        return f"PartnerStats(episodes={self.episodes}, mean={self.mean:.4f} +- {self.stderr:.4f})"


class PartnerPool:
    """A seat occupant made of fixed partners; see the module docstring. It is bound to one env (and its seats) by the
    SelfPlaySession it sits in."""

    def __init__(self, members, weights=None, seed=4321):
        from hanabi_agents.rule_based import RulebasedAgent

        members = list(members)
        if not members:
            raise ValueError("a partner pool needs at least one member")
        if len(members) > MAX_MEMBERS:
            raise ValueError(f"at most {MAX_MEMBERS} members")
        for k, m in enumerate(members):
            if isinstance(m, PartnerPool):
                raise ValueError(f"member {k}: a partner pool cannot hold another pool")
            if not isinstance(m, RulebasedAgent) and not (hasattr(m, "eval_moves") and hasattr(m, "requires_vectorized_observation")
                                                          and m.requires_vectorized_observation()):
                raise ValueError(f"member {k}: {type(m).__name__} is neither a RulebasedAgent nor a DQN-style agent with eval_moves()")
        if len({id(m) for m in members}) != len(members):
            raise ValueError("a member appears twice: give it a larger weight instead")
        weights = [1.0] * len(members) if weights is None else [float(w) for w in weights]
        if len(weights) != len(members):
            raise ValueError(f"{len(members)} members but {len(weights)} weights")
        if not all(math.isfinite(w) and w > 0 for w in weights):
            raise ValueError("weights must be positive and finite")
        self.members = members
        self.weights = weights
        self.seed = int(seed)
        self._draws = 0
        self.env = None
        self.seats = ()
        self.tiles = None          # pool_layout of the bound env
        self._restore = None       # a checkpoint loaded before the pool was bound
        self._shuffle_seen = None  # the env's shuffle mask last checked
        self._ops_key = None       # eval_operands() addresses the tile tables were built from

    # ---- layout ----------------------------------------------------------------------------------------------------------
    def layout(self, n):
        return pool_layout(n, self.weights)

    def rows(self, k):
        """(first row, end row) of member k in the bound env."""
        first, count = self.tiles[k]
        return first * TILE, (first + count) * TILE

    def bind(self, env, seats):
        """Called by SelfPlaySession: fixes the env and the seats the pool holds, allocates the tally state and arms every game
        at the first move of its deal (hb_train_tally_init)."""
        seats = tuple(sorted(set(int(s) for s in seats)))
        if self.env is not None:
            if self.env is not env:
                raise ValueError("this partner pool already serves another env")
            self.seats = seats
            return
        tiles = self.layout(env.n)
        L, dev = K.lib(), env.device
        self.env, self.seats, self.tiles = env, seats, tiles
        self.cfg = env.cfg
        self.n_counters = L.hb_train_counters(C.byref(env.cfg))
        K.check(0 if self.n_counters > 0 else self.n_counters)
        tm = torch.empty(env.n // TILE, dtype=torch.int32)
        for k, (first, count) in enumerate(tiles):
            tm[first:first + count] = k
        self._tile_member = tm.to(dev)
        self._lost = torch.empty(env.n, dtype=torch.uint8, device=dev)
        self._length = torch.empty(env.n, dtype=torch.int16, device=dev)
        self.counters = torch.zeros(len(self.members), self.n_counters, dtype=torch.int64, device=dev)
        self._actions = torch.zeros(env.n, dtype=torch.int32, device=dev)
        self._q = None
        self._scratch = [dict() for _ in self.members]
        K.check(L.hb_train_tally_init(C.byref(env.cfg), L.hb_env_state(env.h), env.n, K.dptr(self._lost), K.dptr(self._length),
                                      K.current_stream()))
        # the move table of the env's tiles: the rule members' blocks now, the DQN members' tiles at the first moves(); every
        # tile is a block of the rule launch and row r takes its global game id (id_stride = block_rows)
        from hanabi_agents.rule_based import RulebasedAgent

        self._rule_members = [k for k, m in enumerate(self.members) if isinstance(m, RulebasedAgent)]
        rule_sets = RuleSets(self.members[k] for k in self._rule_members)
        if len(rule_sets):
            rule_sets.upload(dev)
        self._table = MoveTable(env.n // TILE, (env.n // TILE, TILE, TILE), rule_sets)
        for k in self._rule_members:
            first, count = tiles[k]
            for b in range(first, first + count):
                self._table.walk(b, self.members[k])
        self._table.upload(dev)
        if self._restore is not None:
            sd, self._restore = self._restore, None
            self.load_checkpoint_state(sd)

    def move_table(self, env):
        """The move table (grouped.MoveTable, uploaded) with the one-kernel DQN members' tiles and the member indices of the generic path. The tiles are
        refilled when a member's eval_operands() addresses change."""
        kinds = [classify(m, env.obs_len, env.num_actions, fused=env.packed, prefix=f"member {k}: ") for k, m in enumerate(self.members)]
        key = tuple((o["w1f"], o["b1f"], o["w2f"], o["b2f"], o["support"], o["dtype"], o["hidden"], o["n_atoms"]) if kind == "tile" else None
                    for kind, o in kinds)
        tab = self._table
        if key != self._ops_key:
            tab.set_tiles([(first, count, o, env.first_game_id + TILE * first)
                           for (first, count), (kind, o) in zip(self.tiles, kinds) if kind == "tile"])
            tab.generic = [k for k, (kind, _) in enumerate(kinds) if kind == "generic"]
            tab.upload(env.device)
            self._ops_key = key
        return tab

    # ---- colour shuffle ---------------------------------------------------------------------------------------------------
    def check_color_shuffle(self, env):
        """Rule members read the true state: their rows must have the pool's seats clear in the env's shuffle mask."""
        m = env.color_shuffle if getattr(env, "color_shuffled", False) else 0
        if m is self._shuffle_seen or (isinstance(m, int) and m == self._shuffle_seen):
            return
        bits = sum(1 << s for s in self.seats)
        for k in self._rule_members:
            lo, hi = self.rows(k)
            bad = bool(((m[lo:hi] & bits) != 0).any()) if isinstance(m, torch.Tensor) else bool(int(m) & bits)
            if bad:
                raise ValueError(f"member {k} ({type(self.members[k]).__name__}) reads the true state: its rows {lo}..{hi - 1} must "
                                 f"not shuffle the pool's seats {self.seats} (use PartnerPool.shuffle_mask)")
        self._shuffle_seen = m

    def shuffle_mask(self, seats, n=None, pool_seats=None):
        """[n] uint8 per-game seat mask for HanabiEnv.set_color_shuffle: `seats` shuffled in every game, except the pool's seats on
        the rows of rule members. n / pool_seats default to the bound env's size and the seats the pool holds."""
        from hanabi_agents.rule_based import RulebasedAgent

        if self.env is None and (n is None or pool_seats is None):
            raise ValueError("the pool is not in a session yet: pass n and pool_seats")
        n = self.env.n if n is None else int(n)
        pool_seats = self.seats if pool_seats is None else tuple(pool_seats)
        bits = sum(1 << int(s) for s in seats)
        pbits = sum(1 << int(s) for s in pool_seats)
        tiles = self.layout(n)
        m = torch.full((n,), bits, dtype=torch.uint8)
        for k, mem in enumerate(self.members):
            if isinstance(mem, RulebasedAgent):
                first, count = tiles[k]
                m[first * TILE:(first + count) * TILE] = bits & ~pbits
        return m.to(self.env.device) if self.env is not None else m

    # ---- the agent protocol ------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def moves(self, env):
        """Greedy moves of every member on its rows: int32 [n] on the device (the pool's own buffer)."""
        if env is not self.env:
            raise ValueError("a partner pool acts on the env of the session it was bound to")
        self.check_color_shuffle(env)
        self._draws += 1
        act, draw = self._actions, self._draws
        tab = self.move_table(env)
        if tab.groups and self._q is None:
            self._q = torch.empty(env.n, env.num_actions, dtype=torch.float32, device=env.device)
        tab.launch(env, self.seed, draw, env.first_game_id, act, self._q)
        for k in tab.generic:
            m = self.members[k]
            lo, hi = self.rows(k)
            fgid = m.first_game_id
            m.first_game_id = env.first_game_id + lo   # (keys row r by its global game id; restored at once)
            try:
                m.eval_moves((env, (env.net_obs[lo:hi], env.legal[lo:hi])), self.seed, draw, act[lo:hi], scratch=self._scratch[k])
            finally:
                m.first_game_id = fgid
        return act

    def explore(self, observations):
        env = observations[0] if isinstance(observations, (tuple, list)) else observations
        if not hasattr(env, "h"):
            raise TypeError("PartnerPool reads the env: pass (env, (obs, legal)) or the HanabiEnv itself")
        return self.moves(env)

    def exploit(self, observations):
        return self.explore(observations)

    def requires_vectorized_observation(self):
        return False

    def add_experience_first(self, o, st):
        pass

    def add_experience(self, o, a, r, st):
        pass

    def add_experience_dense(self, o, a, r, st):
        pass

    def update(self):
        pass

    # ---- statistics --------------------------------------------------------------------------------------------------------
    def tally(self, env, seat, actions):
        """hb_train_tally of the env step just issued (seat `seat` played `actions`), on the current stream."""
        L = K.lib()
        K.check(L.hb_train_tally(C.byref(env.cfg), env.n, int(seat), K.dptr(actions), K.dptr(env.reward), K.dptr(env.terminal),
                                 K.dptr(env.score), K.dptr(self._tile_member), len(self.members), K.dptr(self._lost),
                                 K.dptr(self._length), K.dptr(self.counters), K.current_stream()))

    def stats(self):
        """One PartnerStats per member."""
        if self.env is None:
            raise ValueError("the pool is not in a session yet")
        c = self.counters.cpu()
        return [PartnerStats(row, self.cfg.players, self.cfg.colors * self.cfg.ranks + 1) for row in c]

    def reset_stats(self):
        if self.env is not None:
            self.counters.zero_()

    # ---- checkpoint ------------------------------------------------------------------------------------------------------------
    def checkpoint_state(self, include_replay=True):
        if self.env is None:
            raise ValueError("the pool is not in a session yet")
        return dict(format=FORMAT, n=self.env.n, tiles=[list(t) for t in self.tiles], weights=list(self.weights), seed=self.seed,
                    draws=self._draws, counters=self.counters.cpu(), lost=self._lost.cpu(), length=self._length.cpu(),
                    members=[_fingerprint(m) for m in self.members])

    def load_checkpoint_state(self, sd):
        if not isinstance(sd, dict) or sd.get("format") != FORMAT:
            raise ValueError("not a partner-pool checkpoint")
        fp = [_fingerprint(m) for m in self.members]
        if [list(map(_as_list, f)) for f in sd["members"]] != [list(map(_as_list, f)) for f in fp]:
            raise ValueError("checkpoint was written by a pool of different members")
        if [list(t) for t in sd["tiles"]] != [list(t) for t in self.layout(sd["n"])]:
            raise ValueError("checkpoint was written with a different layout (weights)")
        if self.env is None:
            self._restore = sd
            return
        if sd["n"] != self.env.n:
            raise ValueError(f"checkpoint was written for {sd['n']} games, the pool serves {self.env.n}")
        if tuple(sd["counters"].shape) != tuple(self.counters.shape):
            raise ValueError("checkpoint counters do not fit this game")
        self.seed, self._draws = int(sd["seed"]), int(sd["draws"])
        self.counters.copy_(sd["counters"])
        self._lost.copy_(sd["lost"])
        self._length.copy_(sd["length"])


def _as_list(x):
    return [_as_list(y) for y in x] if isinstance(x, (list, tuple)) else x
