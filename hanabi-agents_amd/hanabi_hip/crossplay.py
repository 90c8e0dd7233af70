"""Cross-play on the GPU: every team of a pool of agents on the same fixed deals, all teams in one lock-step evaluation.

Ad-hoc teamplay scores an agent against partners other than itself (the reference ships its rule-based partners for that,
rule_based/predefined_rules.py). `CrossPlay` plays a pool of K agents — DQN checkpoints or seeds and rule-based agents — as K^2
teams on the same deals and returns one `EvalResult` per team, each equal to what `Evaluator(...).run(team)` returns:

    cp = CrossPlay("Hanabi-Full", players=2, n_games=4096, seed=7)
    res = cp.run(pool)                      # default teams: (i, j, j, ..., j) for every ordered pair of pool indices
    res.mean_matrix()                       # K x K: candidate i (seat 0) with partner j (every other seat)

* Layout. Team k owns a block of n_pad = ceil(n / 128) * 128 games. Every block starts from the same deals: the state rows of
  one n_pad-game env built with the evaluator's seed and first_game_id (deal g is keyed by the game id alone, so rows 0..n-1
  are the standalone Evaluator's deals). Padding rows are real games, acted on and stepped, but their `done` byte starts at
  "finished", so they are never counted. Teams go into chunks of at most `max_rows` games; a chunk's env and buffers are built
  once and kept.
* One turn (seat t mod P) issues, on the current stream: the launches of the seat's move table (hanabi_hip.grouped) — one
  hb_actor_fused_act_grouped per (dtype, hidden, n_atoms) group for the blocks whose seat agent takes the one-kernel actor (each
  128-row tile reads its own network's descriptor), one hb_rule_act_grouped for the rule-agent blocks — then one HanabiEnv.step
  over the whole chunk and one hb_eval_tally_grouped (a row of counters per block). The descriptor tables are uploaded once per
  chunk and run, the rule-set table once per run, not per turn. Agents off the one-kernel actor take their
  own eval_moves on row slices of their block (the generic path): rows [r0, r0 + n) in one call — exactly the standalone
  shape, which the library GEMMs' kernel choice and the torch path's generator depend on — then the padding rows.
* `color_shuffle=True`: as Evaluator's, per block: the seats of a block held by DQN-style agents play in colour-permuted frames,
  with the permutations the standalone Evaluator draws for the same deals (game id first_game_id + g, not the chunk row).
* Seeds, draws and game ids are those of Evaluator.run: Philox seed = the evaluator's seed, draw = turn + 1; a DQN agent keys
  its row r by its own first_game_id + r, a rule agent by the evaluator's first_game_id + r. No agent's draw counter,
  histogram, noise or buffers move.
* `responses=True`: Evaluator's partner-response counts, per team: one hb_eval_response_tally_grouped per turn (a block of counts
  per team) between the env step and the grouped tally. Every team's EvalResult carries its `responses`;
  `CrossPlayResult.responses` stacks them in team order and `convention_distance()` compares the teams' response rows. As in
  Evaluator, moves of colour-shuffled seats are in their mover's frame (hanabi_hip.symmetry).
* `playout=True` (default False: the loop above, launch for launch): a run whose teams use `RulebasedAgent`s only, with
  `responses` and `color_shuffle` off (`playout.crossplay_playout_supported`), plays each chunk with ONE launch of
  hb_rule_playout_grouped (hanabi_hip.playout) on a scratch copy of the repeated deals — a block per team, id_stride 0, the padding
  rows' `done` at 0x80 and therefore not played — instead of the loop, and builds no env for the chunk; any other run takes the
  loop. `CrossPlay.last_path` says which ran: "playout" or "loop". Every EvalResult is the loop's field for field, except that
  `turns` is the block's longest game and logged moves after a game's end are -1 (as Evaluator(playout=True)).
"""
import ctypes as C
import math
import weakref

import numpy as np
import torch

from . import _capi as K
from . import playout as _playout
from .env import HanabiEnv
from .evaluate import EvalResult, eval_config, max_turns, normalize_rows, shuffle_mask, uid_kinds
from .grouped import TILE, MoveTable, RuleSets, classify


def default_teams(k, players):
    """The K^2 default teams of a pool of k agents: (i, j, j, ..., j) for i, j in range(k) — candidate i in seat 0, partner j
    in every other seat (2 players: every ordered pair)."""
    k, players = int(k), int(players)
    if k < 1 or players < 2:
        raise ValueError(f"need a pool of >= 1 agents and >= 2 players, got {k} agents, {players} players")
    return [(i,) + (j,) * (players - 1) for i in range(k) for j in range(k)]


def check_teams(teams, k, players):
    """Explicit teams as a list of P-tuples of pool indices; raises ValueError on a bad one."""
    out = []
    for team in teams:
        t = tuple(int(x) for x in team)
        if len(t) != players:
            raise ValueError(f"team {team!r}: one pool index per seat ({players} players)")
        if any(x < 0 or x >= k for x in t):
            raise ValueError(f"team {team!r}: pool indices must be in 0..{k - 1}")
        out.append(t)
    if not out:
        raise ValueError("no teams")
    return out


def padded_games(n):
    """Games per team block: n rounded up to whole 128-row tiles."""
    n = int(n)
    if n < 1:
        raise ValueError(f"n_games must be >= 1, got {n}")
    return -(-n // TILE) * TILE


def plan_chunks(n_teams, n_pad, max_rows):
    """[(first team, team count)] covering n_teams teams of n_pad rows each, at most max_rows rows per chunk (at least one team
    per chunk: a team larger than max_rows gets a chunk of its own). Team k sits at row (k - first) * n_pad of its chunk."""
    if n_teams < 1 or n_pad < 1:
        raise ValueError("n_teams and n_pad must be >= 1")
    per = max(1, int(max_rows) // int(n_pad))
    return [(s, min(per, n_teams - s)) for s in range(0, n_teams, per)]


def convention_distance(counts):
    """Occupancy-weighted total variation between teams' response rows. counts: [T, P, A + 1, A] response counts (one
    EvalResult.responses per team). Returns a symmetric [T, T] float64 matrix: with M_i team i's row-normalised counts and
    n_i[p, r] its row sums,

        D(i, j) = sum over the rows (p, r) both teams have counts in of  w[p, r] * 1/2 * sum_a |M_i[p, r, a] - M_j[p, r, a]|,
        w[p, r] = (n_i + n_j)[p, r] / (the sum of n_i + n_j over those rows)

    0 for identical play, at most 1 (disjoint answers on every shared row), NaN when the two teams share no row."""
    c = np.asarray(counts)
    if c.ndim != 4 or c.shape[2] != c.shape[3] + 1:
        raise ValueError(f"counts must be [T, P, A + 1, A], got {c.shape}")
    n = c.sum(-1).astype(np.float64)   # [T, P, A + 1]
    m = normalize_rows(c)
    T = c.shape[0]
    d = np.full((T, T), np.nan)
    for i in range(T):
        for j in range(i, T):
            shared = (n[i] > 0) & (n[j] > 0)
            if not shared.any():
                continue
            w = (n[i] + n[j])[shared]
            tv = 0.5 * np.abs(m[i][shared] - m[j][shared]).sum(-1)
            d[i, j] = d[j, i] = float((w * tv).sum() / w.sum())
    return d


class CrossPlayResult:
    """teams: the P-tuples of pool indices, results: one EvalResult per team (the class Evaluator returns), k: pool size.
    responses: [T, P, A + 1, A] int64 numpy, the teams' response counts in team order (CrossPlay(responses=True)), else None."""

    def __init__(self, teams, results, k, players, default):
        self.teams, self.results, self.k, self.players, self.default = list(teams), list(results), int(k), int(players), bool(default)
        on = bool(self.results) and all(r.responses is not None for r in self.results)
        self.responses = np.stack([r.responses for r in self.results]) if on else None

    def convention_distance(self):
        """[T, T] float64 over the result's teams (team order): the module's convention_distance of their response counts."""
        if self.responses is None:
            raise ValueError("no response counts: run CrossPlay(responses=True)")
        return convention_distance(self.responses)

    def _matrix(self, value):
        if not self.default:
            raise ValueError("a K x K matrix needs the default teams (run without `teams`)")
        m = torch.empty(self.k, self.k, dtype=torch.float64)
        for (i, j), r in zip(((t[0], t[-1]) for t in self.teams), self.results):
            m[i, j] = value(r)
        return m

    def mean_matrix(self):
        """[i, j] = mean score of candidate i in seat 0 with partner j in every other seat."""
        return self._matrix(lambda r: r.mean)

    def stderr_matrix(self):
        return self._matrix(lambda r: r.stderr)

    def as_dict(self):
        d = dict(players=self.players, pool_size=self.k, teams=[list(t) for t in self.teams], results=[r.as_dict() for r in self.results])
        if self.default:
            d["mean_matrix"] = self.mean_matrix().tolist()
            d["stderr_matrix"] = self.stderr_matrix().tolist()
        return d

    def __repr__(self):
        return f"CrossPlayResult({len(self.teams)} teams, pool of {self.k}, {self.players} players)"


class _Chunk:
    """The env and buffers of `nb` team blocks of n_pad games (built once, reused by every run with that many blocks)."""

    def __init__(self, cp, nb, env=True):
        """env=False: the buffers of the playout path alone, which steps no env and asks no agent for moves."""
        n, n_pad, dev = cp.n, cp.n_pad, cp.device
        rows = nb * n_pad
        self.nb, self.rows = nb, rows
        self.env = None
        if env:
            self.env = HanabiEnv(config=cp.cfg, n_games=rows, seed=cp.seed, first_game_id=cp.first_game_id, device=dev, packed=True)
            dev = self.env.device
        self.rows0 = cp._deals.repeat(nb, 1)
        pad = torch.zeros(n_pad, dtype=torch.uint8, device=dev)
        pad[n:] = 0x80   # padding rows start finished: stepped (the playout: not played), never counted
        self.done0 = pad.repeat(nb)
        self.done = torch.empty_like(self.done0)
        self.final_score = torch.zeros(rows, dtype=torch.int8, device=dev)
        self.length = torch.zeros(rows, dtype=torch.int16, device=dev)
        self.counters0 = torch.zeros(nb, cp.n_counters, dtype=torch.int64, device=dev)
        self.counters0[:, 0] = n
        self.counters = torch.empty_like(self.counters0)
        self.actions = torch.zeros(cp.max_turns if cp.record_actions else 1, rows, dtype=torch.int32, device=dev)
        if not env:
            self.play_rows = torch.empty_like(self.rows0)   # the scratch copy of the deals that the kernel plays
            self.tail = (torch.empty(1, dtype=torch.int64, device=dev), torch.empty(nb, dtype=torch.int32, device=dev))
            return
        self.q = torch.empty(rows, self.env.num_actions, dtype=torch.float32, device=dev)
        if cp.responses:
            A = self.env.num_actions
            self.prev = torch.full((rows,), -1, dtype=torch.int32, device=dev)
            self.resp = torch.zeros(nb, cp.players, A + 1, A, dtype=torch.int64, device=dev)


class CrossPlay:
    """Plays every team of a pool on the same `n_games` deals; see the module docstring.

    game / players / config / seed / first_game_id / record_actions / check_every / responses: as Evaluator. max_rows: games per chunk
    (teams of one chunk run in lock-step; more teams than fit take several chunks one after another). playout: a switch, see the
    module docstring."""

    def __init__(self, game="Hanabi-Full", players=2, n_games=4096, seed=1, first_game_id=0, max_rows=262144, record_actions=False,
                 device=None, config=None, check_every=8, color_shuffle=False, responses=False, playout=False):
        n_games = int(n_games)
        if not isinstance(playout, bool):
            raise TypeError(f"playout is a switch (True or False), got {playout!r}")
        self.playout = playout
        self.last_path = None   # "playout" or "loop": the path the last run() took
        self.color_shuffle = bool(color_shuffle)
        self.responses = bool(responses)
        if n_games < 1:
            raise ValueError(f"n_games must be >= 1, got {n_games}")
        if int(max_rows) < 1:
            raise ValueError(f"max_rows must be >= 1, got {max_rows}")
        cfg = eval_config(game, players, config)
        self.cfg = cfg
        self.players = cfg.players
        self.n = n_games
        self.n_pad = padded_games(n_games)
        self.seed = int(seed)
        self.first_game_id = int(first_game_id)
        self.max_rows = int(max_rows)
        self.record_actions = bool(record_actions)
        self.device = device
        self.check_every = max(1, int(check_every))
        self.max_turns = max_turns(cfg)
        self.max_score = cfg.colors * cfg.ranks
        self.n_counters = K.lib().hb_eval_counters(C.byref(cfg))
        self._deals = None    # [n_pad, state words]: built by the first run (construction needs no GPU)
        self._perms = None    # color_shuffle: [n_pad, P, C] every seat's permutation of those deals
        self._chunks = {}     # block count -> _Chunk
        self._play_chunks = {}   # block count -> _Chunk without an env (the playout path)
        # agent -> eval_moves scratch of the generic path: the block's n rows, and its padding rows
        self._scratch = weakref.WeakKeyDictionary()
        self._scratch_pad = weakref.WeakKeyDictionary()
        self.last_turns = []  # turns played by each chunk of the last run

    def chunks(self, n_teams):
        return plan_chunks(n_teams, self.n_pad, self.max_rows)

    def _chunk(self, nb, with_env=True):
        if self._deals is None:
            env = HanabiEnv(config=self.cfg, n_games=self.n_pad, seed=self.seed, first_game_id=self.first_game_id, device=self.device,
                            packed=True)
            self._deals = env.export_state()
            if self.color_shuffle:   # (the rows are byte-identical to an unshuffled env's)
                env.set_color_shuffle(True, observe=False)
                self._perms = env.color_perms()
            self.device = env.device
        store = self._chunks if with_env else self._play_chunks
        ch = store.get(nb)
        if ch is None:
            ch = store[nb] = _Chunk(self, nb, with_env)
        return ch

    @torch.no_grad()
    def run(self, pool, teams=None, grouped=True):
        """pool: list of agents (DQNAgent / RulebasedAgent); teams: P-tuples of pool indices (default: default_teams).
        grouped=False: every agent takes its own eval_moves per block (the generic path). Returns a CrossPlayResult."""
        pool = list(pool)
        k = len(pool)
        default = teams is None
        teams = default_teams(k, self.players) if default else check_teams(teams, k, self.players)
        for a in pool:
            if not hasattr(a, "eval_moves"):
                raise TypeError(f"{type(a).__name__} has no eval_moves()")
        results = [None] * len(teams)
        self.last_turns = []
        if self.playout and _playout.crossplay_playout_supported(pool, teams, responses=self.responses, color_shuffle=self.color_shuffle):
            self.last_path = "playout"
            rule_sets = RuleSets(pool[i] for i in sorted({i for t in teams for i in t}))
            for first, nb in self.chunks(len(teams)):
                ch = self._chunk(nb, with_env=False)
                if rule_sets.table_dev is None:   # once per run
                    rule_sets.upload(self.device)
                out = self._play_kernel(ch, [[rule_sets.index(pool[i]) for i in t] for t in teams[first:first + nb]], rule_sets)
                for b, res in enumerate(out):
                    results[first + b] = res
            return CrossPlayResult(teams, results, k, self.players, default)
        self.last_path = "loop"
        kinds, rule_sets = self.classify_pool(pool, grouped)
        for first, nb in self.chunks(len(teams)):
            ch = self._chunk(nb)
            if len(rule_sets) and rule_sets.table_dev is None:   # once per run, shared by every seat's table
                rule_sets.upload(ch.env.device)
            chunk_teams = teams[first:first + nb]
            tables = [self.seat_table(ch, [pool[t[s]] for t in chunk_teams], kinds, rule_sets) for s in range(self.players)]
            masks = [shuffle_mask([pool[i] for i in t]) for t in chunk_teams] if self.color_shuffle else None
            out = self._play(ch, tables, masks)
            for b, res in enumerate(out):
                results[first + b] = res
        return CrossPlayResult(teams, results, k, self.players, default)

    def classify_pool(self, pool, grouped=True):
        """(kinds, rule_sets) of one run: id(agent) -> grouped.classify's (kind, argument), and the RuleSets (not uploaded) of the
        pool's rule agents in pool order. grouped=False: nothing takes the grouped kernels; a rule agent is ("rule_generic",
        agent), hb_rule_act per block."""
        L, cfg_ref = K.lib(), C.byref(self.cfg)
        obs_len, n_actions = L.hb_obs_len(cfg_ref), L.hb_num_actions(cfg_ref)
        kinds = {}
        for a in pool:
            if id(a) not in kinds:
                kind, arg = classify(a, obs_len, n_actions, fused=grouped)
                kinds[id(a)] = ("rule_generic" if kind == "rule" and not grouped else kind, arg)
        return kinds, RuleSets(arg for kind, arg in kinds.values() if kind == "rule")

    def seat_table(self, ch, agents, kinds, rule_sets):
        """One seat of one chunk: the MoveTable (uploaded) of the blocks' seat agents `agents`; its generic entries are (block,
        agent, kind). A block's tile i keys its rows from the agent's own first_game_id + 128 * i; the rule launch replays the
        evaluator's game ids in every block (id_stride 0)."""
        per_block = self.n_pad // TILE
        tab = MoveTable(ch.rows // TILE, (ch.nb, self.n_pad, 0), rule_sets)
        held = []
        for b, a in enumerate(agents):
            kind, arg = kinds[id(a)]
            if kind == "tile":
                held.append((b * per_block, per_block, arg, arg["first_game_id"]))
            elif kind == "rule":
                tab.walk(b, a)
            else:
                tab.generic.append((b, a, kind))
        tab.set_tiles(held)
        return tab.upload(ch.env.device)

    def _play(self, ch, tables, masks=None):
        env, L, cfg = ch.env, K.lib(), self.cfg
        perms = None
        if masks is not None:
            m = torch.tensor(masks, dtype=torch.uint8, device=env.device).repeat_interleave(self.n_pad)
            env.set_color_shuffle(m, observe=False)
        env.import_state(ch.rows0)
        if masks is not None and env.color_shuffled:
            # the standalone Evaluator's permutations of these deals, block by block, on the block's shuffled seats only
            seat_on = ((m[:, None] >> torch.arange(self.players, device=env.device, dtype=torch.uint8)) & 1).bool()
            ident = torch.arange(cfg.colors, device=env.device, dtype=torch.uint8).expand(ch.rows, self.players, cfg.colors)
            perms = torch.where(seat_on[:, :, None], self._perms.repeat(ch.nb, 1, 1), ident).contiguous()
            env.set_color_perms(perms)
        env.observe()
        illegal0 = env.illegal_count()
        ch.done.copy_(ch.done0)
        ch.final_score.zero_()
        ch.length.zero_()
        ch.counters.copy_(ch.counters0)
        P, n, n_pad, nb, rows = self.players, self.n, self.n_pad, ch.nb, ch.rows
        cfg_ref = C.byref(cfg)
        tally_bufs = tuple(K.dptr(x) for x in (env.reward, env.terminal, env.score, ch.done, ch.final_score, ch.length, ch.counters))
        resp_bufs = None
        if self.responses:
            ch.prev.fill_(-1)
            ch.resp.zero_()
            resp_bufs = tuple(K.dptr(x) for x in (ch.done, ch.prev, ch.resp))
        live, t = nb * n, 0
        while t < self.max_turns:
            seat = t % P
            act = ch.actions[t if self.record_actions else 0]
            tables[seat].launch(env, self.seed, t + 1, self.first_game_id, act, ch.q)
            for b, a, kind in tables[seat].generic:
                self._generic_moves(ch, b, a, kind, t, act)
            env.step(act)
            if resp_bufs is not None:   # before the tally: `done` still says which games were finished before this turn
                K.check(L.hb_eval_response_tally_grouped(cfg_ref, nb, n_pad, seat, K.dptr(act), *resp_bufs, K.current_stream()))
            K.check(L.hb_eval_tally_grouped(cfg_ref, nb, n_pad, seat, t, K.dptr(act), *tally_bufs, K.current_stream()))
            t += 1
            if t % self.check_every == 0 or t == self.max_turns:
                live = int(ch.counters[:, 0].sum().item())
                if live == 0:
                    break
        if live != 0:
            raise RuntimeError(f"{live} cross-play games still live after max_turns = {self.max_turns} turns")
        illegal = env.illegal_count() - illegal0
        if illegal:
            raise RuntimeError(f"cross-play agents chose {illegal} illegal moves")
        self.last_turns.append(t)
        c = ch.counters.cpu()
        fs, ln = ch.final_score.cpu(), ch.length.cpu()
        resp = ch.resp.cpu().numpy() if self.responses else None
        kinds = uid_kinds(P, cfg.colors, cfg.hand_size, env.num_actions)
        out = []
        for b in range(nb):
            r0 = b * n_pad
            lengths = ln[r0:r0 + n]
            # the turns the standalone Evaluator plays: it reads the live count every check_every turns
            tb = min(self.max_turns, math.ceil(int(lengths.max()) / self.check_every) * self.check_every)
            out.append(EvalResult.from_counters(fs[r0:r0 + n], lengths, self.max_score, c[b], P,
                                                actions=ch.actions[:tb, r0:r0 + n].clone() if self.record_actions else None, turns=tb,
                                                perms=perms[r0:r0 + n] if perms is not None and masks[b] else None,
                                                responses=resp[b] if resp is not None else None, kinds=kinds))
        return out

    def _play_kernel(self, ch, index, rule_sets):
        """_play for a chunk of rule-list teams: one hb_rule_playout_grouped launch on a scratch copy of the repeated deals
        (module docstring). index: the chunk's [nb][P] rule-set indices. The same counters, the same errors."""
        cfg, P, n, n_pad, nb = self.cfg, self.players, self.n, self.n_pad, ch.nb
        with torch.cuda.device(self.device):
            ch.play_rows.copy_(ch.rows0)
            ch.done.copy_(ch.done0)
            ch.final_score.zero_()
            ch.length.zero_()
            ch.counters.copy_(ch.counters0)
            team_of_block = torch.tensor(index, dtype=torch.int32, device=self.device).reshape(nb, P)
            res = _playout._launch_grouped(cfg, ch.play_rows, nb, n_pad, 0, team_of_block, rule_sets, self.seed, 0, None, self.max_turns,
                                           self.first_game_id, ch.done, ch.final_score, ch.length, ch.counters,
                                           ch.actions if self.record_actions else None, tail=ch.tail)
            c = ch.counters.cpu()
            fs, ln = ch.final_score.cpu(), ch.length.cpu()
            illegal, max_len = int(res.illegal), res.max_len.tolist()
        live = int(c[:, 0].sum())
        if live != 0:
            raise RuntimeError(f"{live} cross-play games still live after max_turns = {self.max_turns} turns")
        if illegal:
            raise RuntimeError(f"cross-play agents chose {illegal} illegal moves")
        self.last_turns.append(max(max_len))
        kinds = uid_kinds(P, cfg.colors, cfg.hand_size, K.lib().hb_num_actions(C.byref(cfg)))
        out = []
        for b in range(nb):
            r0 = b * n_pad
            out.append(EvalResult.from_counters(fs[r0:r0 + n], ln[r0:r0 + n], self.max_score, c[b], P,
                                                actions=ch.actions[:max_len[b], r0:r0 + n].clone() if self.record_actions else None,
                                                turns=max_len[b], kinds=kinds))
        return out

    def _generic_moves(self, ch, b, agent, kind, t, act):
        """The generic path for block b: the agent's own eval_moves (or hb_rule_act) on the block's rows, the n real rows first
        (the standalone shape), then the padding rows."""
        env, n, n_pad = ch.env, self.n, self.n_pad
        r0 = b * n_pad
        if kind == "rule_generic":
            L = K.lib()
            sw = env.state_words
            state = L.hb_env_state(env.h)
            K.check(L.hb_rule_act(C.byref(self.cfg), C.c_void_p(state + 4 * sw * r0), n_pad, self.first_game_id, agent._tab,
                                  len(agent.rules), self.seed, t + 1, C.c_void_p(act.data_ptr() + 4 * r0), None, K.current_stream()))
            return
        for lo, hi, store in ((r0, r0 + n, self._scratch), (r0 + n, r0 + n_pad, self._scratch_pad)):
            if hi > lo:
                agent.eval_moves((env, (env.obs_bits[lo:hi], env.legal[lo:hi])), self.seed, t + 1, act[lo:hi],
                                 scratch=store.setdefault(agent, {}))
