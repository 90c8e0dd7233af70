"""Off-belief learning, level 1 (Hu et al. 2021): self-play training whose replay rows are played out
from fictitious states drawn from the V0 belief instead of from the real cards.

    sess = OffBeliefSession(env, [agent0, agent1])
    sess.run(10_000)

At step t, seat i = t mod P to act on the real states S_t:

  1. a_t = the agent's move on its real observation, chosen as SelfPlaySession chooses it (act_for_step, explore, exploit).
  2. Trained seat: the fictitious branch. `Determinizer.sample(env.export_state(), seat=i, replicas=1, seed=belief_seed, draw=t,
     first_row_id=env.first_game_id)` re-draws seat i's own hand and the undealt deck of every game from what seat i cannot see —
     the belief of a player who assumes everything so far was played by a uniformly random policy. Seat i's observation and legal
     mask of that state S'_t are those of S_t (they do not show its own hand or the deck order), so a_t is legal there. S'_t is
     imported into a scratch env (same game, players, n, seed and first game id; auto-reset off) and stepped with a_t, then with
     the greedy move (`eval_moves`, seed = belief_seed, draw = t * P + k) of each partner (i + k) mod P, k = 1 .. P - 1, on the
     scratch env's observations. A fictitious game that has ended is stepped on like a finished rollout game of the search
     (hanabi_hip.search.rollout): the env ignores the moves.
  3. One transition per game goes into seat i's replay (DQNAgent.add_transitions_dense, hb_obl_insert): (real observation, a_t,
     sum of the branch's rewards up to its ending step, seat i's next observation and legal mask in the branch, ended). The real
     transition is not inserted: add_experience* is never called.
  4. env.step(a_t) on the real states, then the agent's update as SelfPlaySession schedules it.

Passive seats (rule-based agents, DQN agents outside train_seats) act and get no branch. `eval_moves` moves no draw counter and
no buffer of an agent, so the real game of step(train=False) is the game SelfPlaySession plays.

Levels 2 and above: `OffBeliefSession(env, agents, belief_policy=[pi0, pi1], depth=L, oversample=K)` (2 players). Level k is
level 1 with ONE thing changed: the fictitious state of step 2 comes from the belief that reads the partner's last L moves as
moves of the frozen level k - 1 policy `belief_policy[partner]` (`frozen_copy` of a trained agent) instead of as random play:

  * the session keeps one `PartnerHistory` per branch seat in the TRAINING env, where games end and are dealt anew at different
    steps. At seat i's step t it advances by one turn in one kernel call (`PartnerHistory.advance`, hb_belief_history_step,
    csrc/belief.hip): seat i's real move of step t - 2 leaves the alive masks, games whose terminal flag was set at step t - 1 or
    t - 2 lose their entries (an auto-reset game is a new deal from there on), and (export of step t - 1, export of step t)
    is pushed with draw t - 1. The session exports the env's state on every step for this, also on a passive seat's turn;
  * `ConditionedDeterminizer.sample_history(rows, history_i, partner=belief_policy[j], seat=i, replicas=1, oversample=K,
    seed=belief_seed, draw=t, partner_seed=belief_seed, first_game_id=env.first_game_id, first_row_id=env.first_game_id)`
    replaces `Determinizer.sample`: K candidates per game, and the first one under which the frozen policy reproduces the most
    of the partner's last L moves (hb_belief_select_depth);
  * everything after that (scratch import, the real move, the LIVE partners' greedy moves, hb_obl_insert) is unchanged.

The real partner plays the epsilon-greedy live policy, not the frozen one, so a game's first moves, a chain cut by a re-deal and a
real move the frozen policy makes under no candidate hand fall back as hb_belief_select_depth defines: to a shallower filter, then
to the V0 belief. Fallbacks are normal; they are counted (`conditioned_rows`, `fallback_rows`, `unconditioned_rows`, `survivors`,
`depth_used_sum`, `belief_forwards`), never errors. With `belief_policy=None` (the default) nothing of this exists and the session
is level 1, bit for bit.

`belief_epsilon=eps` (default None: the exact-match filter above; needs a belief policy) reads the partner as epsilon-greedy on the
frozen policy, which is what the real partner is while it explores: every candidate keeps a likelihood (1 - eps + eps / n per
reproduced move, eps / n per missed one, n = the legal moves of the hypothetical state) and the fictitious state is drawn in
proportion to importance weight times likelihood (`ConditionedDeterminizer`'s epsilon, hb_belief_select_soft). There is no depth
fallback: `fallback_rows` stays 0, `conditioned_rows` counts the live rows with at least one usable partner move, `depth_used_sum`
their usable moves, and `ess_sum` adds up the effective sample size of the conditioned rows' weighted candidates (a move nobody
explains leaves the likelihoods equal: the V0 belief, by itself). No learning gain is claimed for it.

`score_belief=True` (default False: nothing is computed, and training is the same bits either way) scores the fictitious state of
every branch against the real cards before the branch is played (hb_belief_score, `hanabi_hip.search.belief_score`, one replica per
game): `belief_cards` (the cards scored), `belief_hit_sum` (those the fictitious hand gets right, slot by slot), `belief_prior_sum`
(the sum of the mass card counting alone puts on the true card), `belief_joint_sum` (whole hands right) and `belief_roots`. At one
replica per game hit_sum / cards is still an unbiased estimate of the mass the belief puts on the true card; a cross-entropy needs
more replicas and is not reported here.

The frozen policy's observations of the K candidate slabs come from one hb_encode_rows call (`self.cdet.stateless`, on by default;
False: an import and an observe per slab on a scratch env, the same bits).

Not built: three and more players at level 2+, the branch on hb_chain_run, and one forward over all `oversample` slabs.
"""
import weakref

import torch

from . import _capi as K
from .env import HanabiEnv
from .search import (MAX_DEPTH, MAX_SOFT_CANDIDATES, ConditionedDeterminizer, Determinizer, PartnerHistory, _ask, belief_score,
                     running, soft_table)
from .selfplay import SelfPlaySession


class OffBeliefSession(SelfPlaySession):
    """SelfPlaySession whose trained seats learn from fictitious branches; see the module docstring.

    Counters: env_steps (real), grad_steps, branch_steps (fictitious env steps: n * P per trained step) and dead_rows (rows whose
    determinizer weight was 0: the unchanged real row, inserted all the same; none on states reached by play).

    belief_policy (one entry per seat: a frozen agent with eval_moves, or None for a seat nobody conditions on), depth (1..8) and
    oversample (>= 1): level k >= 2, see the module docstring; 2 players. Further counters, device sums read with one sync each:
    conditioned_rows (live rows whose fictitious state reproduces at least one partner move: fallback == 0), fallback_rows (usable
    moves, no surviving candidate: the V0 belief), unconditioned_rows (no usable move), survivors (sum over the conditioned rows
    of the candidates that pass the filter of the depth used), depth_used_sum, and belief_forwards (eval_moves calls made for the
    belief, counted on the host). belief_epsilon (the soft filter, see the module docstring) adds ess_sum (a float).
    score_belief (both levels; see the module docstring) adds belief_cards, belief_roots (ints), belief_hit_sum, belief_prior_sum
    and belief_joint_sum (floats): device sums, read with one sync each, 0 in a session built without the switch (one built with
    it may set `score_belief` to False and back between steps)."""

    LEVEL_COUNTERS = ("conditioned_rows", "fallback_rows", "unconditioned_rows", "survivors", "depth_used_sum")
    BELIEF_COUNTERS = ("belief_cards", "belief_hit_sum", "belief_prior_sum", "belief_joint_sum", "belief_roots")

    _select_in_env = False   # a_t is needed before the env steps

    def __init__(self, env, agents, train_seats=None, belief_seed=1, updates_per_step=1, min_replay=None, belief_policy=None,
                 depth=1, oversample=4, belief_epsilon=None, score_belief=False):
        import torch.distributed as dist

        from .partner_pool import PartnerPool

        agents = list(agents)
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise ValueError("off-belief training is single-rank: torch.distributed is initialised with more than one rank")
        if getattr(env, "color_shuffled", False):
            raise ValueError("off-belief training on a colour-shuffled env is not supported: the scratch env's deals would draw "
                             "other permutations than the real env's")
        for s, a in enumerate(agents):
            if isinstance(a, PartnerPool):
                raise ValueError(f"seat {s}: a partner pool has no single partner to play the fictitious branch with")
        seats = set(range(env.players)) if train_seats is None else set(train_seats)
        for s, a in enumerate(agents):
            if not hasattr(a, "eval_moves"):
                raise TypeError(f"seat {s}: {type(a).__name__} has no eval_moves()")
            if s not in seats or not hasattr(a, "add_transitions_dense"):
                continue
            p = a.params
            if p.n_step != 1:
                raise ValueError(f"seat {s}: n_step must be 1 (consecutive replay rows come from different fictitious worlds), got {p.n_step}")
            if not p.mask_terminal:
                raise ValueError(f"seat {s}: mask_terminal must be True (a finished fictitious game has no next observation to "
                                 "bootstrap through)")
            if int(getattr(a, "actor_lag", 0)) != 0:
                raise ValueError(f"seat {s}: actor_lag must be 0, got {a.actor_lag}")
        if not isinstance(score_belief, bool):
            raise TypeError(f"score_belief is a switch (True or False), got {score_belief!r}")
        depth, oversample = int(depth), int(oversample)
        if belief_epsilon is not None:
            if belief_policy is None:
                raise ValueError("belief_epsilon belongs to a belief policy: it is the exploration rate that policy's moves are read with")
            belief_epsilon = float(belief_epsilon)
            soft_table(belief_epsilon, 1)   # (the range check)
            if oversample > MAX_SOFT_CANDIDATES:
                raise ValueError(f"the soft filter takes at most {MAX_SOFT_CANDIDATES} candidates per row, got oversample = {oversample}")
        if belief_policy is None:
            if depth != 1 or oversample != 4:
                raise ValueError("depth and oversample belong to a belief policy: without one the belief is the V0 belief (level 1)")
        else:
            belief_policy = list(belief_policy)
            if env.players != 2:
                raise ValueError(f"a belief policy needs 2 players (the conditioned belief is built for two), the env has {env.players}")
            if len(belief_policy) != env.players:
                raise ValueError(f"belief_policy has one entry per seat: {env.players} players, {len(belief_policy)} entries")
            if not 1 <= depth <= MAX_DEPTH:
                raise ValueError(f"depth must be in 1..{MAX_DEPTH}, got {depth}")
            if oversample < 1:
                raise ValueError(f"oversample must be >= 1, got {oversample}")
            for s, b in enumerate(belief_policy):
                if b is not None and any(b is a for a in agents):
                    raise ValueError(f"belief_policy[{s}] is one of the session's own agents: belief policies are frozen "
                                     "(hanabi_hip.obl.frozen_copy)")
            for s, a in enumerate(agents):   # the seats that will get a branch need their partner's policy
                if s in seats and s < env.players and hasattr(a, "add_transitions_dense"):
                    b = belief_policy[1 - s]
                    if b is None:
                        raise ValueError(f"belief_policy[{1 - s}] is None, but seat {s} is trained on the belief over seat {1 - s}'s moves")
                    if not hasattr(b, "eval_moves"):
                        raise TypeError(f"belief_policy[{1 - s}]: {type(b).__name__} has no eval_moves()")
        super().__init__(env, agents, updates_per_step=updates_per_step, min_replay=min_replay, train_seats=train_seats,
                         native_chain=False)
        # the seats that get a branch: trained ones whose agent keeps a replay
        self.branch_seats = {s for s in self.train_seats if 0 <= s < env.players and hasattr(self.agents[s], "add_transitions_dense")}
        self.belief_seed = int(belief_seed)
        self.det = Determinizer(config=env.cfg)
        P, n, dev = env.players, env.n, env.device
        self.scratch = HanabiEnv(config=_without_reset(env.cfg), n_games=n, seed=env.seed, first_game_id=env.first_game_id,
                                 auto_reset=False, device=dev, packed=env.packed)
        self._det_rows = torch.empty((n, self.det.state_words), dtype=torch.int32, device=dev)
        self._det_w = torch.empty(n, dtype=torch.int32, device=dev)
        self._rew = torch.zeros((P, n), dtype=torch.float32, device=dev)
        self._term = torch.zeros((P, n), dtype=torch.int8, device=dev)
        self.branch_moves = torch.zeros((P, n), dtype=torch.int32, device=dev)   # row k: what seat i + k played in the last branch
        self._dead = torch.zeros((), dtype=torch.int64, device=dev)
        self._ask_scratch = weakref.WeakKeyDictionary()   # agent -> the buffers its eval_moves writes
        self.branch_steps = 0
        self.score_belief = score_belief
        self._belief = torch.zeros(len(self.BELIEF_COUNTERS), dtype=torch.float64, device=dev) if score_belief else None
        # level k >= 2: the partner histories of the training env and what advancing them needs from the last two steps
        self.belief_policy, self.depth, self.oversample = belief_policy, depth, oversample
        self.belief_epsilon = belief_epsilon
        self.belief_forwards = 0
        if belief_policy is not None:
            self.cdet = ConditionedDeterminizer(config=env.cfg)
            self.histories = {s: PartnerHistory(env.cfg, n, depth, dev, partner_seed=self.belief_seed, first_game_id=env.first_game_id)
                              for s in sorted(self.branch_seats)}
            self._own = {s: torch.zeros(n, dtype=torch.int32, device=dev) for s in self.histories}   # the seat's last real move
            self._own_t = {}                # seat -> the step that move was made at
            self._prev_rows = None          # the export of the previous step
            self._term_old = torch.zeros(n, dtype=torch.int8, device=dev)   # the terminal flags of the step before the last
            self._reset = torch.zeros(n, dtype=torch.int8, device=dev)
            self._level = torch.zeros(len(self.LEVEL_COUNTERS), dtype=torch.int64, device=dev)
            self._ess = torch.zeros((), dtype=torch.float64, device=dev)
            self.last_belief = None         # (n_surv [depth, n], depth_used [n], fallback [n]) of the last branch

    @property
    def dead_rows(self):
        return int(self._dead.item())

    @property
    def ess_sum(self):
        """belief_epsilon: the sum over the conditioned rows of their candidates' effective sample size (0.0 without)."""
        return 0.0 if self.belief_policy is None else float(self._ess.item())

    def _clear_histories(self):
        for h in self.histories.values():
            h.clear()
        self._own_t.clear()
        self._prev_rows = None
        self._term_old.zero_()

    def load_checkpoint_state(self, sd):
        """SelfPlaySession's. The partner histories are not part of a checkpoint: they are cleared, so the first `depth` partner
        moves after a load are unconditioned (a resumed level k >= 2 run is not bit-identical to the uninterrupted one for that
        long; level 1 is)."""
        super().load_checkpoint_state(sd)
        if self.belief_policy is not None:
            self._clear_histories()

    def _conditioned_sample(self, seat, rows, first):
        """The fictitious states of seat `seat` at this step from the belief conditioned on its partner history -> _det_rows,
        _det_w. `first`: the first step after construction or a load (nothing to advance the histories with)."""
        env, t, h = self.env, self.t, self.histories[seat]
        if not first:
            h.advance(own_moves=self._own[seat] if self._own_t.get(seat) == t - 2 else None, reset=self._reset, cur_rows=rows,
                      prev_rows=self._prev_rows, seat=seat, draw=t - 1)
        got = self.cdet.sample_history(
            rows, h, partner=self.belief_policy[1 - seat], seat=seat, replicas=1, oversample=self.oversample, seed=self.belief_seed,
            draw=t, partner_seed=self.belief_seed, first_game_id=env.first_game_id, first_row_id=env.first_game_id,
            out=(self._det_rows, self._det_w), epsilon=self.belief_epsilon)
        used, fb = got.depth_used, got.fallback
        self.belief_forwards += min(h.depth, h.filled) * self.oversample
        self.last_belief = (got.n_surv, used, fb)
        # fallback 0 and 1 are running rows by construction (hb_belief_select_depth: a finished row has no usable entry)
        # (the soft filter: fallback is 0 with a usable move and 2 without, never 1)
        cond = fb == 0
        if self.belief_epsilon is not None:
            self._ess += (got.ess.double() * cond).sum()
        self._level += torch.stack([cond.sum(), (fb == 1).sum(), (running(rows) & (fb == 2)).sum(), (got.survivors() * cond).sum(),
                                    used.sum()])

    def _score(self, rows, seat):
        """score_belief: the fictitious states in _det_rows / _det_w against the real `rows`, one replica per game."""
        if not self.score_belief:
            return
        s = belief_score(self.det.cfg, rows, self._det_rows, self._det_w, seat, 1).sums()
        self._belief += torch.stack([s[0].sum(), s[1].sum(), s[2].sum(), s[6, 0], s[5, 0]])

    def _record(self, agent, seat, observations):
        """Nothing: the real transition is not inserted (trained seats), and a passive seat's replay is never read."""

    def _scratch_step(self, moves, k):
        """scratch.step(moves) with reward and terminal written straight into row k of the branch's buffers."""
        sc = self.scratch
        out = (K.dptr(sc.legal), K.dptr(self._rew[k]), K.dptr(self._term[k]), K.dptr(sc.agent_reward), K.dptr(sc.agent_step_type),
               K.dptr(sc.score), K.current_stream())
        if sc.packed:
            K.check(sc.L.hb_env_step_packed(sc.h, K.dptr(moves), K.dptr(sc.obs_bits), None, *out))
            sc._obs_stale = True
        else:
            K.check(sc.L.hb_env_step(sc.h, K.dptr(moves), K.dptr(sc._obs), *out))

    @torch.no_grad()
    def _before_env_step(self, agent, seat, actions, observations):
        if self.belief_policy is not None:
            self._before_env_step_conditioned(agent, seat, actions)
            return
        if seat not in self.branch_seats:
            return
        with torch.cuda.device(self.env.device):
            rows = self.env.export_state()
            self.det.sample(rows, seat=seat, replicas=1, seed=self.belief_seed, draw=self.t, first_row_id=self.env.first_game_id,
                            out=(self._det_rows, self._det_w))
            self._score(rows, seat)
            self._branch(agent, seat, actions)

    def _before_env_step_conditioned(self, agent, seat, actions):
        """Level k >= 2: every step exports the state and keeps the terminal flags of the last two steps; a branch seat's step
        advances its history, samples from the conditioned belief and branches as level 1 does."""
        env = self.env
        with torch.cuda.device(env.device):
            rows = env.export_state()
            first = self._prev_rows is None
            if not first:   # (env.terminal: the flags of step t - 1; before the first step they belong to no step of this run)
                torch.bitwise_or(env.terminal, self._term_old, out=self._reset)
            if seat in self.branch_seats:
                self._conditioned_sample(seat, rows, first)
                self._score(rows, seat)
                self._branch(agent, seat, actions)
                self._own[seat].copy_(actions)
                self._own_t[seat] = self.t
            if not first:
                self._term_old.copy_(env.terminal)
            self._prev_rows = rows

    def _branch(self, agent, seat, actions):
        """The fictitious states are in _det_rows / _det_w: play the branch from them and insert its transitions."""
        env, sc, P, t = self.env, self.scratch, self.env.players, self.t
        self._dead += (self._det_w == 0).sum()
        sc.import_state(self._det_rows)
        self.branch_moves[0].copy_(actions)
        self._scratch_step(self.branch_moves[0], 0)
        for k in range(1, P):
            partner = self.agents[(seat + k) % P]
            self._wait_for_update_of(partner)
            _ask(partner, sc, self.belief_seed, t * P + k, self.branch_moves[k], self._ask_scratch)
            self._scratch_step(self.branch_moves[k], k)
        self.branch_steps += env.n * P
        agent.add_transitions_dense(env.net_obs, self.branch_moves[0], self._rew, self._term, sc.net_obs, sc.legal)

    def _wait_for_update_of(self, partner):
        """A partner that trains on a learner stream without the split update guards its weights with the session's `done`
        event alone (split update: eval_moves itself waits for the optimizer step's event)."""
        done = self._update_done.get(id(partner))
        if done is not None and not getattr(partner, "split_update", False):
            done.wait()


def _without_reset(cfg):
    """The env's game without the reset flags (HanabiEnv(auto_reset=False) sets them itself)."""
    return K.HbConfig(cfg.players, cfg.colors, cfg.ranks, cfg.hand_size, cfg.max_info, cfg.max_life,
                      cfg.flags & ~(K.FLAG_AUTO_RESET | K.FLAG_RESET_START_NEXT))


for _j, _name in enumerate(OffBeliefSession.LEVEL_COUNTERS):   # the level k >= 2 device counters as read-only ints (0 at level 1)
    setattr(OffBeliefSession, _name,
            property(lambda self, j=_j: 0 if self.belief_policy is None else int(self._level[j].item())))


for _j, _name in enumerate(OffBeliefSession.BELIEF_COUNTERS):   # score_belief's device sums (0 in a session built without it)
    setattr(OffBeliefSession, _name,
            property(lambda self, j=_j, kind=(float if _name.endswith("_sum") else int): kind(0 if self._belief is None else
                                                                                              self._belief[j].item())))


def frozen_copy(agent):
    """An independent DQNAgent with `agent`'s parameters and current weights (online and target), built as restore_weights()
    builds one from saved weights: a belief policy for the next level, or a fixed partner. It keeps no replay of its own (the
    smallest ring) and shares no tensor with `agent`: further training of `agent` does not reach it. Updates in flight on a
    learner stream must be joined first (SelfPlaySession.flush())."""
    from hanabi_agents.rlax_dqn import ActionSpec, DQNAgent, ObservationSpec

    if not isinstance(agent, DQNAgent):
        raise TypeError(f"frozen_copy copies a DQNAgent, got {type(agent).__name__}")
    params = agent.params._replace(experience_buffer_size=64, actor_lag=0)
    with torch.no_grad():
        copy = DQNAgent(ObservationSpec((1, agent.obs_len)), ActionSpec(agent.n_actions), params, device=agent.device, process_group=False)
        copy.online.load_state_dict({k: v.detach().clone() for k, v in agent.online.state_dict().items()})
        copy.target.load_state_dict({k: v.detach().clone() for k, v in agent.target.state_dict().items()})
    copy._eff_cache = None
    copy.first_game_id = agent.first_game_id
    return copy
