"""Trajectory oracle of the replay ring and its n-step gather. TEST INFRASTRUCTURE ONLY.

Written from what the ring MEANS, not from how it is indexed: a transition's successors are the next transitions of the
SAME GAME (spec: hanabi_agents/rainbow/replay_memory.py:316-345 of the reference — sum the discounted rewards of up to
n_step transitions of one trajectory, stop after a terminal one, bootstrap from the last one taken), and the ring is
whatever the writes of hanabi_agents/rlax_dqn/experience_buffer.py:46-81 leave behind (each row goes to the next slot,
the slot after the last one is the first, a later write replaces an earlier one).

It is fed the same inserts as the ring under test, in order. Insert k is a batch of rows; row g belongs to game g.
Per game it keeps the list of that game's transitions; per slot it keeps which (insert, game) the slot holds now, found
by replaying the writes one row at a time. There is no successor-slot arithmetic and no distance to a write pointer in
here: `nstep` reads a game's own list. All arithmetic is float64.

The product never imports this module (tests/test_capi_symbols.py::test_product_never_touches_the_oracle).
"""
import numpy as np


class ReplayOracle:
    def __init__(self, capacity, first_obs, first_slot=0):
        """first_obs [n_games, L]: each game's observation before its first transition (the caller's `last_obs`).
        first_slot: where the first row is written (0 for a fresh ring; the insert-only cases start elsewhere, and for
        those `size` is not meaningful)."""
        self.capacity = int(capacity)
        self.last_obs = np.array(first_obs, copy=True)
        self.games = [[] for _ in range(self.last_obs.shape[0])]   # per game: its transitions, oldest first
        self.holder = [None] * self.capacity                       # per slot: (insert, game) held now
        self._next = int(first_slot)                               # the slot the next row is written to
        self.n_inserts = 0

    # ---- feeding -----------------------------------------------------------------------------------------
    def insert(self, obs, legal, action, reward, step_type):
        """One insert: row g is game g's next transition. Returns the slots written, in row order."""
        n = obs.shape[0]
        assert n == len(self.games), "every insert carries one row per game"
        k, written = self.n_inserts, []
        for g in range(n):
            self.games[g].append(dict(obs_tm1=self.last_obs[g].copy(), obs_t=np.array(obs[g], copy=True),
                                      legal=np.array(legal[g], copy=True), action=int(action[g]),
                                      reward=np.float32(reward[g]), terminal=bool(int(step_type[g]) == 2)))
            self.holder[self._next] = (k, g)   # a later write replaces an earlier one
            written.append(self._next)
            self._next += 1
            if self._next == self.capacity:
                self._next = 0
            self.last_obs[g] = obs[g]
        self.n_inserts += 1
        return written

    # ---- the ring the writes leave behind ------------------------------------------------------------------
    @property
    def size(self):
        return sum(h is not None for h in self.holder)

    @property
    def write_pointer(self):
        return self._next

    def transition(self, slot):
        k, g = self.holder[slot]
        return self.games[g][k]

    def expected_ring(self):
        """The six ring arrays (slots never written: zero, and False in `written`), last_obs, size and write pointer."""
        cap, t0 = self.capacity, self.games[0][0]
        out = dict(obs_tm1=np.zeros((cap,) + t0["obs_tm1"].shape, t0["obs_tm1"].dtype),
                   obs_t=np.zeros((cap,) + t0["obs_t"].shape, t0["obs_t"].dtype),
                   act=np.zeros((cap, 1), np.int8), lms=np.zeros((cap,) + t0["legal"].shape, np.int8),
                   rew=np.zeros((cap, 1), np.float32), term=np.zeros((cap, 1), bool), written=np.zeros(cap, bool))
        for slot, h in enumerate(self.holder):
            if h is None:
                continue
            t = self.transition(slot)
            out["obs_tm1"][slot], out["obs_t"][slot], out["lms"][slot] = t["obs_tm1"], t["obs_t"], t["legal"]
            out["act"][slot, 0], out["rew"][slot, 0], out["term"][slot, 0] = t["action"], t["reward"], t["terminal"]
            out["written"][slot] = True
        out.update(last_obs=self.last_obs.copy(), size=self.size, write_pointer=self.write_pointer)
        return out

    # ---- the n-step transition that starts at a slot ---------------------------------------------------------
    def nstep(self, slot, n_step, gamma32):
        """Transition k of game g sits in `slot`. Take it, then the game's transitions k+1, k+2, ... while fewer than n_step
        are taken, the last one taken is not terminal and the next one exists (its insert has happened).
        Returns R = sum gamma^i r_i, m = transitions taken, disc = gamma^m, the last one's obs_t / legal / terminal and
        S = sum gamma^i |r_i|, with gamma = float64(float32(gamma32)); obs_tm1 and action are the first one's."""
        k, g = self.holder[slot]
        game = self.games[g]
        taken = [game[k]]
        while len(taken) < n_step and not taken[-1]["terminal"] and k + len(taken) < len(game):
            taken.append(game[k + len(taken)])
        gamma = float(np.float32(gamma32))
        R = S = 0.0
        for i, t in enumerate(taken):
            R += gamma ** i * float(t["reward"])
            S += gamma ** i * abs(float(t["reward"]))
        m = len(taken)
        return dict(R=R, S=S, m=m, disc=gamma ** m, obs_tm1=taken[0]["obs_tm1"], action=taken[0]["action"],
                    obs_t=taken[-1]["obs_t"], legal=taken[-1]["legal"], terminal=taken[-1]["terminal"],
                    last=(k + m - 1, g))
