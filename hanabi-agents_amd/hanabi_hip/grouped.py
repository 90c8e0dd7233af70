"""Moves of a batch whose rows are held by different agents, in a few launches: the acting half that cross-play (crossplay.py: team
blocks on repeated deals) and the partner pool (partner_pool.py: members on the distinct games of a training env) share.

`classify` sorts an agent into a rule list, a one-kernel DQN agent (its eval_operands() fill 128-row tile descriptors) or a
generic agent (its own eval_moves, which stays with the caller). `RuleSets` is the [n_sets][MAX_RULES] rule table of
hb_rule_act_grouped / hb_rule_act_blocks. `MoveTable` is one batch's who-holds-what: an hb_fused_tile array per
(dtype, hidden, n_atoms) group and the rule set of every block. Both are plain host objects until `upload`; `MoveTable.launch`
issues one hb_actor_fused_act_grouped per group in sorted key order, then one grouped rule launch, on the current stream."""
import ctypes as C

import torch

from . import _capi as K

TILE = 128   # rows per workgroup of the one-kernel actor, and per hb_fused_tile


def classify(agent, obs_len, n_actions, fused=True, prefix=""):
    """("rule", agent) for a RulebasedAgent, ("tile", eval_operands()) for an agent of vectorised observations on the one-kernel
    actor, ("generic", None) for any other agent of vectorised observations; TypeError for anything else. fused=False: nothing
    takes the one-kernel actor and eval_operands() is not called. ValueError (after `prefix`) when the operands are another
    game's."""
    from hanabi_agents.rule_based import RulebasedAgent

    if isinstance(agent, RulebasedAgent):
        return "rule", agent
    if not agent.requires_vectorized_observation():
        raise TypeError(f"{type(agent).__name__}: cross-play runs DQN-style agents (vectorised observations) and RulebasedAgent")
    ops = agent.eval_operands() if fused and hasattr(agent, "eval_operands") else None
    if ops is None:
        return "generic", None
    if ops["obs_len"] != obs_len or ops["n_actions"] != n_actions:
        raise ValueError(f"{prefix}agent of obs_len {ops['obs_len']} / {ops['n_actions']} actions in a game of {obs_len} / {n_actions}")
    return "tile", ops


def _device_bytes(table, device):
    return torch.frombuffer(bytearray(table), dtype=torch.uint8).to(device)


class RuleSets:
    """The rule lists of `agents` as one table: `table` [len(agents) * MAX_RULES] HbRule (set s at s * MAX_RULES), `n_rules`."""

    def __init__(self, agents):
        self.agents = list(agents)
        self.table = (K.HbRule * (K.MAX_RULES * len(self.agents)))()
        for s, a in enumerate(self.agents):
            for q in range(len(a.rules)):
                self.table[s * K.MAX_RULES + q] = a._tab[q]
        self.n_rules = [len(a.rules) for a in self.agents]
        self.table_dev = self.n_rules_dev = None

    def __len__(self):
        return len(self.agents)

    def index(self, agent):
        return next(s for s, a in enumerate(self.agents) if a is agent)

    def upload(self, device):
        self.table_dev = _device_bytes(self.table, device)
        self.n_rules_dev = torch.tensor(self.n_rules, dtype=torch.int32, device=device)
        return self


class MoveTable:
    """Who holds which rows of a batch of n_tiles 128-row tiles.

    geometry: (n_blocks, block_rows, id_stride) of the rule launch: row r of block b walks the block's rule list keyed by game id
    first_game_id + b * id_stride + r. rule_sets: the RuleSets the blocks index (shared between tables; uploaded by its owner).
    groups: [((dtype, hidden, n_atoms), HbFusedTile[n_tiles])] in sorted key order, unheld tiles inactive; set_of_block: the rule
    set of every block (-1: none); generic: the caller's own entries for agents off both kernels; keep: the support tensors the
    descriptors point to."""

    def __init__(self, n_tiles, geometry, rule_sets):
        self.n_tiles, self.geometry, self.rule_sets = int(n_tiles), tuple(int(x) for x in geometry), rule_sets
        if self.geometry[2] not in (0, self.geometry[1]):
            raise ValueError(f"id_stride must be 0 (repeated deals) or block_rows, got {self.geometry}")
        self.set_of_block = [-1] * self.geometry[0]
        self.groups, self.generic, self.keep = [], [], []
        self.groups_dev = self.sets_dev = None

    def walk(self, block, agent):
        """Block `block` walks the rule list of `agent` (one of rule_sets)."""
        self.set_of_block[block] = self.rule_sets.index(agent)

    def set_tiles(self, held):
        """held: [(first, count, ops, base)]: tiles [first, first + count) are held by the agent of operands `ops`
        (eval_operands()), and tile first + i keys its rows from game id base + TILE * i. Replaces every earlier descriptor."""
        tabs = {}
        for first, count, o, base in held:
            key = (o["dtype"], o["hidden"], o["n_atoms"])
            tab = tabs.get(key)
            if tab is None:
                tab = tabs[key] = (K.HbFusedTile * self.n_tiles)()
            for i in range(count):
                d = tab[first + i]
                d.w1f, d.b1f, d.w2f, d.b2f, d.support = o["w1f"], o["b1f"], o["w2f"], o["b2f"], o["support"]
                d.first_game_id = base + TILE * i
                d.active = 1
        self.groups = sorted(tabs.items())
        self.keep = [o["support_t"] for _, _, o, _ in held]   # (alive while the tables hold their addresses)
        self.groups_dev = None

    def upload(self, device):
        """The device tensors that are not there yet: the tile tables (after set_tiles) and set_of_block (when a block walks a
        rule list)."""
        if self.groups_dev is None:
            self.groups_dev = [_device_bytes(tab, device) for _, tab in self.groups]
        if self.sets_dev is None and any(s >= 0 for s in self.set_of_block):
            self.sets_dev = torch.tensor(self.set_of_block, dtype=torch.int32, device=device)
        return self

    def launch_tiles(self, env, seed, draw, actions, q):
        """One hb_actor_fused_act_grouped per group: greedy moves of the held tiles' rows into `actions` (their q rows into q)."""
        L, stream = K.lib(), K.current_stream()
        for ((dt, hidden, n_atoms), _), tab in zip(self.groups, self.groups_dev):
            K.check(L.hb_actor_fused_act_grouped(K.dptr(tab), self.n_tiles * TILE, K.dptr(env.obs_bits), K.dptr(env.legal), env.obs_len,
                                                 hidden, env.num_actions, n_atoms, K.dptr(q), 0.0, seed, draw, K.dptr(actions), dt, stream))

    def launch_rules(self, env, seed, draw, first_game_id, actions):
        """The one rule launch of the blocks that walk a rule list: hb_rule_act_grouped (id_stride 0) or hb_rule_act_blocks."""
        if self.sets_dev is None:
            return
        L, rs = K.lib(), self.rule_sets
        n_blocks, block_rows, id_stride = self.geometry
        fn = L.hb_rule_act_blocks if id_stride else L.hb_rule_act_grouped
        K.check(fn(C.byref(env.cfg), L.hb_env_state(env.h), n_blocks, block_rows, first_game_id, K.dptr(self.sets_dev),
                   K.dptr(rs.table_dev), K.dptr(rs.n_rules_dev), len(rs), seed, draw, K.dptr(actions), None, K.current_stream()))

    def launch(self, env, seed, draw, first_game_id, actions, q):
        self.launch_tiles(env, seed, draw, actions, q)
        self.launch_rules(env, seed, draw, first_game_id, actions)
