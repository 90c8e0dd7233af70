"""Greedy evaluation on the GPU: a fixed set of evaluation games, played to the end.

Every Hanabi result is quoted as the greedy policy's mean score over a fixed set of fresh games, with the score histogram
and the perfect-game rate beside it (the reference: `DQNAgent.exploit`, hanabi_agents/rlax_dqn/rlax_rainbow.py:277-282, on
the separate evaluation env of its external session). `Evaluator` does that without disturbing a training run:

    ev = Evaluator("Hanabi-Full", players=2, n_games=32768, seed=7)
    res = ev.run([agent, agent])          # or a mixed team: [agent, RulebasedAgent(piers_rules)]
    res.mean, res.stderr, res.perfect_rate, res.histogram

* It owns a packed `HanabiEnv` with auto-reset off and every buffer it uses. `run` re-imports the state rows dealt at
  construction, so every call plays the SAME deals: deck(g) = Philox(seed, first_game_id + g, episode 1).
* Lock-step: turn t is seat t mod P in every game. Per turn, all asynchronous on the current stream:
  `agents[seat].eval_moves` -> `HanabiEnv.step` -> `hb_eval_tally` (include/hanabi_hip.h, csrc/eval.hip). The agents' moves use
  Philox seed = the evaluator's `seed`, draw = turn + 1; no agent's own draw counter, histogram or buffers move.
* The host reads the live-game counter every `check_every` turns and stops at 0; `max_turns(cfg)` bounds the loop.
* `color_shuffle=True`: the seats held by DQN-style agents (vectorised observations) play in colour-permuted frames
  (the "OP score"); rule-based seats read the true state and stay unshuffled. The permutations are those
  of the deals (seed, game id, deal counter 1, seat) and come back as `EvalResult.perms`; recorded actions are in each seat's
  own frame.
* `responses=True`: the partner-response counts, `EvalResult.responses[seat, prev + 1, uid]` = how often `seat` answered the
  move `prev` made just before its own (row 0: the first move of a game) with `uid`. One more small launch per turn,
  `hb_eval_response_tally`, between the env step and `hb_eval_tally`; nothing else changes, and with the switch off nothing is
  launched or allocated for it. `EvalResult.response_matrix()` normalises the rows to P(my move | the move before mine), the
  conditional action matrix of the Other-Play and SAD papers. With `color_shuffle=True` the combination is allowed, but every
  move is in its mover's own frame: `prev` is in the partner's frame and `uid` in mine, so reveal-colour rows and columns of
  shuffled seats are not in a common frame (hanabi_hip.symmetry maps uids between frames; that mapping is not applied here).
* `playout=True` (default False: the loop above, launch for launch): a team of `RulebasedAgent`s only, with `responses` and
  `color_shuffle` off, is played by ONE launch of hb_rule_playout (hanabi_hip.playout) on a scratch copy of the deals instead of
  the loop; any other team or option takes the loop. `Evaluator.last_path` says which ran: "playout" or "loop". The result is the
  loop's, from the same counters, with two documented differences: `EvalResult.turns` is the longest game's length (the loop
  reports the first multiple of `check_every` at or after it), and recorded actions are -1 from a game's end on (the loop
  records moves the env ignored). The host reads the counters once per run instead of once per `check_every` turns.
"""
import ctypes as C
import math
import weakref

import numpy as np
import torch

from . import _capi as K
from .env import HanabiEnv
from . import playout as _playout


def max_turns(cfg):
    """Upper bound on the length of any game of configuration `cfg`.

    Every discard or play draws a card while the deck lasts, so at most D - P*H of them happen before it runs dry; the game
    then ends after P more turns. Each hint spends an information token: there are INFO at the start, one more per discard
    (a discard is legal only below the maximum) and at most one more per completed colour (C). So before the deck runs dry
    there are at most D - P*H discards / plays and INFO + (D - P*H) + C hints:

        max_turns = (D - P*H) + (INFO + D - P*H + C) + P          (2-player full Hanabi: 40 + 53 + 2 = 95)
    """
    L = K.lib()
    d = L.hb_deck_size(C.byref(cfg))
    if d <= 0:
        raise K.HbError(f"invalid configuration {cfg!r}: {L.hb_last_error().decode()}")
    draws = d - cfg.players * cfg.hand_size
    return draws + (cfg.max_info + draws + cfg.colors) + cfg.players


def eval_config(game, players, config=None):
    """The configuration of games played to the end: the preset `game` / `players`, or `config` with its flags dropped (no
    auto-reset, scores without leniency). Validated: ValueError on a bad one."""
    if config is not None:
        cfg = K.HbConfig(config.players, config.colors, config.ranks, config.hand_size, config.max_info, config.max_life, 0)
    else:
        cfg = K.make_config(game, players, 0)
    if K.lib().hb_config_validate(C.byref(cfg)) != 0:
        raise ValueError(f"invalid configuration {cfg!r}: {K.lib().hb_last_error().decode()}")
    return cfg


MOVE_KINDS = ("discard", "play", "reveal_color", "reveal_rank")


def uid_kinds(players, colors, hand_size, num_actions):
    """[A] int64: the kind (index into MOVE_KINDS) of every move uid, App. A.2 order: H discards, H plays, (P - 1) * C colour
    reveals, then the rank reveals. The decoding hb_eval_tally's move-kind counters use."""
    u = np.arange(int(num_actions))
    h, pc = int(hand_size), (int(players) - 1) * int(colors)
    return np.where(u < h, 0, np.where(u < 2 * h, 1, np.where(u < 2 * h + pc, 2, 3))).astype(np.int64)


def response_counts(actions, lengths, players, num_actions, first_seat=0):
    """The partner-response counts of a recorded action log, in plain numpy (what hb_eval_response_tally accumulates on the
    device). actions [T, n] int: turn t is seat (first_seat + t) % P's move in every game; game g is counted for
    t < lengths[g]. Returns [P, A + 1, A] int64: out[seat, prev + 1, uid], prev = the game's previous counted move, -1 (row 0)
    at its first. A uid outside 0 .. A-1 is not counted and does not become `prev`."""
    actions = np.asarray(actions)
    lengths = np.asarray(lengths).astype(np.int64)
    P, A = int(players), int(num_actions)
    if actions.ndim != 2 or lengths.shape != (actions.shape[1],):
        raise ValueError("actions [T, n] and lengths [n]")
    out = np.zeros((P, A + 1, A), np.int64)
    prev = np.full(actions.shape[1], -1, np.int64)
    for t in range(actions.shape[0]):
        u = actions[t].astype(np.int64)
        ok = (t < lengths) & (u >= 0) & (u < A)
        np.add.at(out[(int(first_seat) + t) % P], (prev[ok] + 1, u[ok]), 1)
        prev[ok] = u[ok]
    return out


def normalize_rows(counts):
    """counts [..., A] -> float64 rows divided by their sums; a row without counts is NaN."""
    c = np.asarray(counts, np.float64)
    tot = c.sum(-1, keepdims=True)
    return np.divide(c, tot, out=np.full_like(c, np.nan), where=tot > 0)


def shuffle_mask(team):
    """Seat mask of a team's colour-shuffled seats: those whose agent reads vectorised observations (DQN-style agents).
    Rule-based agents read the true state rows and keep the true colours."""
    return sum(1 << s for s, a in enumerate(team) if a.requires_vectorized_observation())


class EvalResult:
    """Outcome of one evaluation: plain CPU tensors and ints.

    scores [n] int32 final scores (0 after a bomb-out), lengths [n] int32 turns played, histogram [max_score + 1] int64,
    bombouts (games that lost every life), moves [P, 4] int64 per seat and kind (MOVE_KINDS), misplays [P] int64 per seat,
    actions [turns, n] int32 (record_actions only; rows of finished games hold moves the env ignored), turns = turns played,
    perms [n, P, C] uint8 (colour-shuffled evaluations only): perms[g, p, c] = the colour seat p saw for true colour c.
    responses [P, A + 1, A] int64 numpy (responses=True only, else None): responses[p, prev + 1, uid] = how often seat p played
    uid right after the move prev (row 0: first move of a game); kinds [A] = the move kind of every uid (uid_kinds)."""

    def __init__(self, scores, lengths, max_score, histogram=None, bombouts=0, moves=None, misplays=None, actions=None, turns=None,
                 perms=None, responses=None, kinds=None):
        self.scores = torch.as_tensor(scores).to("cpu", torch.int32)
        self.lengths = torch.as_tensor(lengths).to("cpu", torch.int32)
        n = self.scores.numel()
        if n < 1 or self.lengths.shape != self.scores.shape:
            raise ValueError("scores and lengths: equal, non-empty vectors")
        self.max_score = int(max_score)
        self.histogram = (torch.bincount(self.scores.long(), minlength=self.max_score + 1) if histogram is None
                          else torch.as_tensor(histogram).to("cpu", torch.int64))
        self.bombouts = int(bombouts)
        self.moves = None if moves is None else torch.as_tensor(moves).to("cpu", torch.int64)
        self.misplays = None if misplays is None else torch.as_tensor(misplays).to("cpu", torch.int64)
        self.actions = None if actions is None else actions.cpu()
        self.turns = int(turns) if turns is not None else int(self.lengths.max())
        self.perms = None if perms is None else torch.as_tensor(perms).to("cpu", torch.uint8)
        if responses is None:
            self.responses = None
        else:
            r = responses.cpu().numpy() if isinstance(responses, torch.Tensor) else np.asarray(responses)
            if r.ndim != 3 or r.shape[1] != r.shape[2] + 1:
                raise ValueError(f"responses must be [P, A + 1, A], got {r.shape}")
            self.responses = r.astype(np.int64, copy=True)
        self.kinds = None if kinds is None else np.asarray(kinds, np.int64)

    @classmethod
    def from_counters(cls, final_score, length, max_score, counters_row, players, **rest):
        """The result of a counter row of hb_eval_tally (layout: the header comment of hb_eval_counters / hb_eval_tally): [0] live
        games, [1, 1 + B) the score histogram (B = max_score + 1), [1 + B] bomb-outs, then moves [P][4] and misplays [P]; a
        longer row's tail is ignored. rest: EvalResult's other arguments."""
        c, B, P = counters_row, int(max_score) + 1, int(players)
        return cls(final_score, length, max_score, histogram=c[1:1 + B], bombouts=int(c[1 + B]),
                   moves=c[2 + B:2 + B + 4 * P].view(P, 4), misplays=c[2 + B + 4 * P:2 + B + 5 * P], **rest)

    def response_matrix(self, seat=None, kinds=False):
        """P(my move | the move made just before mine) as float64 [A + 1, A] (seat=None: the seats' counts pooled, then
        normalised) — row 0 is the first move of a game; every row is divided by its sum and a row without counts is NaN.
        kinds=True: both axes collapsed to move kinds first, [5, 4] = (none, *MOVE_KINDS) x MOVE_KINDS."""
        if self.responses is None:
            raise ValueError("no response counts: evaluate with responses=True")
        c = self.responses
        if kinds:
            if self.kinds is None or self.kinds.shape != (c.shape[2],):
                raise ValueError("kinds=True needs the uid kinds of the game (EvalResult(kinds=uid_kinds(...)))")
            rows = np.concatenate(([0], 1 + self.kinds))
            k = np.zeros((c.shape[0], 5, 4), np.int64)
            np.add.at(k, (slice(None), rows[:, None], self.kinds[None, :]), c)
            c = k
        c = c.sum(0) if seat is None else c[int(seat)]
        return normalize_rows(c)

    @property
    def n_games(self):
        return self.scores.numel()

    @property
    def mean(self):
        return float(self.scores.double().mean())

    @property
    def stderr(self):
        """Standard error of the mean: sample standard deviation (n - 1) / sqrt(n); 0 for one game."""
        n = self.n_games
        return float(self.scores.double().std(unbiased=True)) / math.sqrt(n) if n > 1 else 0.0

    @property
    def perfect_rate(self):
        return float((self.scores == self.max_score).double().mean())

    @property
    def bombout_rate(self):
        return self.bombouts / self.n_games

    def cpu(self):
        return self

    def as_dict(self):
        """JSON-able numbers (no per-game vectors)."""
        d = dict(n_games=self.n_games, mean=self.mean, stderr=self.stderr, perfect_rate=self.perfect_rate,
                 bombout_rate=self.bombout_rate, max_score=self.max_score, histogram=self.histogram.tolist(),
                 mean_length=float(self.lengths.double().mean()), max_length=int(self.lengths.max()), turns=self.turns)
        if self.moves is not None:
            d["moves"] = [dict(zip(MOVE_KINDS, row)) for row in self.moves.tolist()]
        if self.misplays is not None:
            d["misplays"] = self.misplays.tolist()
        if self.responses is not None:
            d["responses"] = self.responses.tolist()
        return d

    def __repr__(self):
        return f"EvalResult(n_games={self.n_games}, mean={self.mean:.4f} +- {self.stderr:.4f}, perfect={self.perfect_rate:.4f})"


class Evaluator:
    """Plays the same `n_games` deals to the end every `run(agents)`; see the module docstring.

    game / players: a preset of hanabi_hip.GAME_TYPES (or `config`: an HbConfig whose flags are ignored — evaluation games
    never auto-reset and score without leniency). first_game_id: global id of game 0 (keys the deals and the agents' draws)."""

    def __init__(self, game="Hanabi-Full", players=2, n_games=4096, seed=1, first_game_id=0, device=None, record_actions=False,
                 config=None, check_every=8, color_shuffle=False, responses=False, playout=False):
        n_games = int(n_games)
        if n_games < 1:
            raise ValueError(f"n_games must be >= 1, got {n_games}")
        self.color_shuffle = bool(color_shuffle)
        self.responses = bool(responses)
        if not isinstance(playout, bool):
            raise TypeError(f"playout is a switch (True or False), got {playout!r}")
        self.playout = playout
        self.last_path = None   # "playout" or "loop": the path the last run() took
        cfg = eval_config(game, players, config)
        self.cfg = cfg
        self.players = cfg.players
        self.n = n_games
        self.seed = int(seed)
        self.first_game_id = int(first_game_id)
        self.device = device
        self.record_actions = bool(record_actions)
        self.check_every = max(1, int(check_every))
        self.max_turns = max_turns(cfg)
        self.max_score = cfg.colors * cfg.ranks
        self.n_counters = K.lib().hb_eval_counters(C.byref(cfg))
        self.env = None      # created by the first run(): construction needs no GPU
        # agent -> the buffers its eval_moves writes (q, h, GEMM operand); weak keys: a dead agent's buffers go with it and are
        # never handed to another agent
        self._scratch = weakref.WeakKeyDictionary()

    def _setup(self):
        if self.env is not None:
            return
        env = HanabiEnv(config=self.cfg, n_games=self.n, seed=self.seed, first_game_id=self.first_game_id, device=self.device,
                        packed=True)
        dev = env.device
        self.env = env
        self.rows0 = env.export_state()   # the deals every run starts from
        self.done = torch.zeros(self.n, dtype=torch.uint8, device=dev)
        self.final_score = torch.zeros(self.n, dtype=torch.int8, device=dev)
        self.length = torch.zeros(self.n, dtype=torch.int16, device=dev)
        self.counters = torch.zeros(self.n_counters, dtype=torch.int64, device=dev)
        self.actions = (torch.zeros(self.max_turns, self.n, dtype=torch.int32, device=dev) if self.record_actions
                        else torch.zeros(1, self.n, dtype=torch.int32, device=dev))
        if self.responses:
            A = env.num_actions
            self.prev = torch.full((self.n,), -1, dtype=torch.int32, device=dev)
            self.resp = torch.zeros(self.players, A + 1, A, dtype=torch.int64, device=dev)

    @torch.no_grad()
    def run(self, agents):
        agents = list(agents)
        if len(agents) != self.players:
            raise ValueError(f"one agent per seat: {self.players} players, {len(agents)} agents")
        for a in agents:
            if not hasattr(a, "eval_moves"):
                raise TypeError(f"{type(a).__name__} has no eval_moves()")
        self._setup()
        if self.playout and _playout.playout_supported(agents, responses=self.responses, color_shuffle=self.color_shuffle):
            self.last_path = "playout"
            return self._run_playout(agents)
        self.last_path = "loop"
        env, L, cfg = self.env, K.lib(), self.cfg
        perms = None
        if self.color_shuffle:   # DQN seats shuffled, rule seats not; the import below draws the deals' permutations
            env.set_color_shuffle(shuffle_mask(agents), observe=False)
        env.import_state(self.rows0)
        env.observe()
        if self.color_shuffle and env.color_shuffled:
            perms = env.color_perms()
        illegal0 = env.illegal_count()
        self.done.zero_()
        self.final_score.zero_()
        self.length.zero_()
        self.counters.zero_()
        self.counters[0] = self.n
        P, n = self.players, self.n
        cfg_ref = C.byref(cfg)
        bufs = tuple(K.dptr(t) for t in (env.reward, env.terminal, env.score, self.done, self.final_score, self.length, self.counters))
        resp_bufs = None
        if self.responses:
            self.prev.fill_(-1)
            self.resp.zero_()
            resp_bufs = tuple(K.dptr(t) for t in (self.done, self.prev, self.resp))
        live, t = self.n, 0
        while t < self.max_turns:
            seat = t % P
            agent = agents[seat]
            act = self.actions[t if self.record_actions else 0]
            if agent.requires_vectorized_observation():
                agent.eval_moves((env, (env.net_obs, env.legal)), self.seed, t + 1, act, scratch=self._scratch.setdefault(agent, {}))
            else:
                agent.eval_moves(env, self.seed, t + 1, act)
            env.step(act)
            if resp_bufs is not None:   # before the tally: `done` still says which games were finished before this turn
                K.check(L.hb_eval_response_tally(cfg_ref, n, seat, K.dptr(act), *resp_bufs, K.current_stream()))
            K.check(L.hb_eval_tally(cfg_ref, n, seat, t, K.dptr(act), *bufs, K.current_stream()))
            t += 1
            if t % self.check_every == 0 or t == self.max_turns:
                live = int(self.counters[0].item())
                if live == 0:
                    break
        if live != 0:
            raise RuntimeError(f"{live} evaluation games still live after max_turns = {self.max_turns} turns")
        illegal = env.illegal_count() - illegal0
        if illegal:
            raise RuntimeError(f"evaluation agents chose {illegal} illegal moves")
        return EvalResult.from_counters(self.final_score, self.length, self.max_score, self.counters.cpu(), P,
                                        actions=self.actions[:t].clone() if self.record_actions else None, turns=t, perms=perms,
                                        responses=self.resp if self.responses else None,
                                        kinds=uid_kinds(P, cfg.colors, cfg.hand_size, env.num_actions))

    def _run_playout(self, agents):
        """run() for a team of rule lists: one hb_rule_playout launch on a scratch copy of the deals (module docstring). The
        same buffers, the same counters, the same errors; one host read."""
        cfg, P, dev = self.cfg, self.players, self.env.device
        if getattr(self, "_play_rows", None) is None:
            self._play_rows = torch.empty_like(self.rows0)
            self._play_tail = (torch.empty(1, dtype=torch.int64, device=dev), torch.empty(1, dtype=torch.int32, device=dev))
        with torch.cuda.device(dev):
            self._play_rows.copy_(self.rows0)
            self.done.zero_()
            self.final_score.zero_()
            self.length.zero_()
            self.counters.zero_()
            self.counters[0] = self.n
            log = self.actions if self.record_actions else None
            res = _playout._launch(cfg, self._play_rows, agents, self.seed, 0, None, self.max_turns, self.first_game_id, self.done,
                                   self.final_score, self.length, self.counters, log, tail=self._play_tail)
            c = torch.cat([self.counters, res.illegal, res.max_len.long()]).cpu()   # the one host read of the run
        live, illegal, t = int(c[0]), int(c[-2]), int(c[-1])
        if live != 0:
            raise RuntimeError(f"{live} evaluation games still live after max_turns = {self.max_turns} turns")
        if illegal:
            raise RuntimeError(f"evaluation agents chose {illegal} illegal moves")
        return EvalResult.from_counters(self.final_score, self.length, self.max_score, c, P,
                                        actions=self.actions[:t].clone() if self.record_actions else None, turns=t,
                                        kinds=uid_kinds(P, cfg.colors, cfg.hand_size, self.env.num_actions))
