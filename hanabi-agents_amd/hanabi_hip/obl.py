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

Not built: levels 2 and above (they need the belief of the previous level's policy; ConditionedDeterminizer is the obvious
source), the branch on hb_chain_run, and batching the fictitious partner's forward with the real one.
"""
import weakref

import torch

from . import _capi as K
from .env import HanabiEnv
from .search import Determinizer, _ask
from .selfplay import SelfPlaySession


class OffBeliefSession(SelfPlaySession):
    """SelfPlaySession whose trained seats learn from fictitious branches; see the module docstring.

    Counters: env_steps (real), grad_steps, branch_steps (fictitious env steps: n * P per trained step) and dead_rows (rows whose
    determinizer weight was 0: the unchanged real row, inserted all the same; none on states reached by play)."""

    _select_in_env = False   # a_t is needed before the env steps

    def __init__(self, env, agents, train_seats=None, belief_seed=1, updates_per_step=1, min_replay=None):
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

    @property
    def dead_rows(self):
        return int(self._dead.item())

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
        if seat not in self.branch_seats:
            return
        env, sc, P, t = self.env, self.scratch, self.env.players, self.t
        with torch.cuda.device(env.device):
            self.det.sample(env.export_state(), seat=seat, replicas=1, seed=self.belief_seed, draw=t, first_row_id=env.first_game_id,
                            out=(self._det_rows, self._det_w))
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
