"""The exact belief against rule-list partners: hb_belief_enumerate (include/hanabi_hip_exact.h, csrc/belief_exact.hip; DESIGN.md
section 11f, "The exact belief").

A team made only of `RulebasedAgent`s reads no observation: a seat's move is a pure function of the state row and three Philox
keys. The observer's hand enters that function through one word of the row, and the hands the observer may hold are few enough
to walk them all: `belief_enumerate` weighs every hand by the number of physical deals behind it and keeps those under which the
partners' rule lists make the moves they made. The marginals have no undrawn cards, the replicas are drawn from the true
posterior, and every sampled belief gets a yardstick.

    b = belief_enumerate(cfg, rows, history, [piers, piers], seat=0, replicas=32, seed=1, draw=t)   # -> ExactBelief
    b.posterior()                                   # [m, H, NC] float64: P(slot s holds card c | the partner's moves)
    rows_r, w = exact_rows(cfg, rows, b.hands, 0, seed=1, draw=t)   # the drawn hands as full state rows (hb_belief_carry)

`ExactDeterminizer.sample_history` is the two together and returns `ConditionedDeterminizer`'s `BeliefSample`;
`exact_supported` says whether a blueprint and a set of options can take this path, and `RolloutSearch(exact=True)`,
`SearchPlayer(condition=True, exact=True)` and `SelfPlaySession.search(exact=True)` ask it. The switch is off by default
everywhere.

The entry point's ctypes signature lives here, bound on first use, and not in `_capi.SIGNATURES`: that table mirrors
include/hanabi_hip.h, and this prototype is declared in a header of its own (see there for why).
"""
import ctypes as C
from typing import NamedTuple, Optional

import torch

from . import _capi as K
from .playout import rule_tables

MAX_DEPTH = 8
MAX_REPLICAS = 1 << 20
# The largest power of two MEASURED (2^8 .. 2^20 in steps of 4x; nothing above) at which an exact turn of 1 024 roots costs no more
# than the depth-4 sampled turn: 39.5 ms against 53.8 ms, 93 % of the roots enumerated (scripts/exact_belief_probe.py, part `turn`;
# profiles/exact_belief/exact_belief_probe.json). The scratch buffer takes a byte per hand of the cap and root: 1 MiB per root.
DEFAULT_MAX_HANDS = 1 << 20

_FN = None


def _fn():
    """hb_belief_enumerate and hb_belief_enumerate_scratch with their argument types, bound once."""
    global _FN
    if _FN is None:
        L = K.lib()
        f = L.hb_belief_enumerate
        f.restype = C.c_int
        f.argtypes = ([C.POINTER(K.HbConfig), C.c_void_p, C.c_int64, C.c_int32] + [C.c_void_p] * 4 +
                      [C.c_int32, C.POINTER(C.c_uint64), C.c_uint64, C.c_int64, C.POINTER(C.POINTER(K.HbRule)), C.POINTER(C.c_int32),
                       C.c_int64, C.c_int32, C.c_uint64, C.c_uint64, C.c_int64] + [C.c_void_p] * 10 + [C.c_void_p])
        s = L.hb_belief_enumerate_scratch
        s.restype = C.c_int64
        s.argtypes = [C.POINTER(K.HbConfig), C.c_int64, C.c_int64]
        _FN = (f, s)
    return _FN


def scratch_bytes(cfg, m, max_hands):
    """hb_belief_enumerate_scratch: the bytes of scratch `belief_enumerate` needs for m roots (pure host arithmetic)."""
    n = _fn()[1](C.byref(cfg), int(m), int(max_hands))
    if n < 0:
        raise ValueError(K.lib().hb_last_error().decode())
    return int(n)


def _pool_prior(cfg, rows, seat):
    """From the true rows alone, in torch: truth [m, H] int64 (-1: no such slot, or the root is not running), cnt [m, NC] int64
    (the copies of every card in the seat's pool) and prior [m, H, NC] int64 (hb_belief_score's: cnt where the slot's hints allow
    the card)."""
    r = rows.long() & 0xFFFFFFFF
    m, dev = r.shape[0], r.device
    P, H, Rk, NC = cfg.players, cfg.hand_size, cfg.ranks, cfg.colors * cfg.ranks
    deck_n = K.lib().hb_deck_size(C.byref(cfg))
    live = ((r[:, 0] >> 19) & 3) == 0
    n = torch.where(live, ((r[:, 1] >> (15 + 3 * seat)) & 7).clamp(max=H), 0)
    slot = torch.arange(H, device=dev).view(1, H)
    hand = (r[:, 10 + seat].view(m, 1) >> (5 * slot)) & 31
    held = slot < n.view(m, 1)
    truth = torch.where(held, hand, -1)
    q = torch.arange(deck_n, device=dev).view(1, deck_n)
    deck = (r[:, 10 + 3 * P:].gather(1, (q >> 2).expand(m, deck_n)) >> (8 * (q & 3))) & 255
    undealt = live.view(m, 1) & (q >= (deck_n - (r[:, 0] & 63).clamp(max=deck_n)).view(m, 1))
    card = torch.arange(NC, device=dev).view(1, 1, NC)
    cnt = ((hand.unsqueeze(2) == card) & held.unsqueeze(2)).sum(1) + ((deck.unsqueeze(2) == card) & undealt.unsqueeze(2)).sum(1)
    know = r[:, 10 + P + 2 * seat] | (r[:, 10 + P + 2 * seat + 1] << 32)
    kn = (know.view(m, 1) >> (12 * slot)) & 0xFFF
    ok = (((kn.unsqueeze(2) >> (card // Rk)) & 1) != 0) & (((kn.unsqueeze(2) >> (5 + card % Rk)) & 1) != 0) & held.unsqueeze(2)
    return truth, cnt, torch.where(ok, cnt.view(m, 1, NC), 0)


class ExactBelief(NamedTuple):
    """What hb_belief_enumerate writes (include/hanabi_hip_exact.h has the definitions), for m roots and a history of depth D:

        status     [m] uint8            0: enumerated; 1: more than max_hands hands, nothing else computed; 2: not running
        space      [m] int64            the hands of the enumeration space
        mass       [D + 1, m] int64     level k: the mass of the hands that reproduce the partner's last k moves
        n_hands    [D + 1, m] int32     ... and how many of them have a mass
        depth_used [m] int32            the deepest level with any mass
        fallback   [m] uint8            0: depth_used >= 1, 1: no hand reproduces even the last move, 2: no usable move
        marg       [m, H, NC] int64     the posterior marginal at the level used, unnormalised
        marg0      [m, H, NC] int64     the same at level 0, the exact V0 marginal (None unless asked for)
        hands      [m, R] int32         R hand words (u32 bits) drawn in proportion to the mass at the level used

    cfg and seat: what `figures` needs to read a true row."""
    status: torch.Tensor
    space: torch.Tensor
    mass: torch.Tensor
    n_hands: torch.Tensor
    depth_used: torch.Tensor
    fallback: torch.Tensor
    marg: torch.Tensor
    marg0: Optional[torch.Tensor]
    hands: torch.Tensor
    cfg: Optional[K.HbConfig] = None
    seat: int = 0

    def total(self):
        """[m] int64: the mass at the level used (0 for a root that was not enumerated)."""
        return self.mass.gather(0, self.depth_used.long().view(1, -1)).view(-1)

    def posterior(self):
        """[m, H, NC] float64 = marg / the mass at the level used: P(slot s holds card c). Zeros for a root that was not
        enumerated and for the slots the hand does not have."""
        return self.marg.double() / self.total().clamp(min=1).double().view(-1, 1, 1)

    def sums(self, true_rows, where=None):
        """`BeliefScore.sums`' tensor [len(BeliefScore.SUMS), H] float64 for this belief against the cards `true_rows` [m, SW] really
        hold, over the enumerated roots with any mass (and in `where`, an optional [m] bool mask): no smoothing, the exact
        belief leaves no card undrawn. The whole-hand figure takes the true hand's mass as a survivor's, which it is whenever
        the history's moves were made by the rule lists the belief was computed with."""
        truth, cnt, prior = _pool_prior(self.cfg, true_rows, int(self.seat))
        NC = prior.shape[2]
        T = self.total()
        scored = (self.status == 0) & (T > 0) & (truth[:, 0] >= 0)
        if where is not None:
            scored = scored & where
        has = scored.unsqueeze(1) & (truth >= 0)
        at = truth.clamp(0, NC - 1).unsqueeze(2)
        ws = T.clamp(min=1).double().unsqueeze(1)
        q = torch.where(truth < NC, self.marg.gather(2, at).squeeze(2), 0).double() / ws
        pr = torch.where(truth < NC, prior.gather(2, at).squeeze(2), 0).double() / prior.sum(2).clamp(min=1).double()
        same = truth.unsqueeze(2) == truth.unsqueeze(1)                      # [m, s, t]: slot t holds slot s's card
        H = truth.shape[1]
        earlier = torch.ones((H, H), dtype=torch.int64, device=truth.device).tril(-1) != 0
        before = (same & earlier.unsqueeze(0)).sum(2)                        # ... among the slots t < s
        factor = (cnt.gather(1, truth.clamp(0, NC - 1)) - before).clamp(min=0)
        joint = torch.where(truth >= 0, factor, 1).prod(1).double() / ws.squeeze(1)
        zero = torch.zeros((), dtype=torch.float64, device=q.device)
        nll = lambda p: torch.where(has, -torch.log(p), zero).sum(0)
        first = torch.zeros_like(q[0])
        first[0] = 1.0
        return torch.stack([has.sum(0).double(), torch.where(has, q, zero).sum(0), torch.where(has, pr, zero).sum(0), nll(q), nll(pr),
                            first * scored.sum(), first * torch.where(scored, joint, zero).sum()])

    def figures(self, true_rows, where=None):
        """`belief_figures`' dict (`hit_rate`: the mass on the true card, `joint_rate`: on the whole hand, `cross_entropy`, the
        `prior_` ones, `by_slot`), so that exact and sampled beliefs print side by side."""
        from .search import belief_figures

        return belief_figures(self.sums(true_rows, where))


def _check(t, shape, dtype, name, dev):
    if not isinstance(t, torch.Tensor) or t.shape != tuple(shape) or t.dtype != dtype or not t.is_contiguous():
        got = f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"{name}: expected a contiguous {dtype} tensor of shape {tuple(shape)}, got {got}")
    if t.device != dev:
        raise K.HbError(f"{name} must be on the rows' GPU {dev}, got {t.device}")


def _is_rule_agent(a):
    from hanabi_agents.rule_based import RulebasedAgent

    return isinstance(a, RulebasedAgent)


def exact_supported(blueprint, players, epsilon=None, track=False, color_shuffle=False):
    """True exactly when the exact belief can stand in for the conditioned one: every seat a `RulebasedAgent` (its move is a
    function of the state row alone), 2 players (the gate condition=True has), and no option on that it does not cover: the soft
    likelihood, tracking, colour-shuffled frames. Pure host code."""
    blueprint = list(blueprint)
    if int(players) != 2 or len(blueprint) != 2 or not all(_is_rule_agent(a) for a in blueprint):
        return False
    return epsilon is None and not track and not color_shuffle


def belief_enumerate(cfg, rows, history, team, seat, replicas, seed, draw, partner_seed=0, first_game_id=0, first_row_id=0,
                     max_hands=DEFAULT_MAX_HANDS, marg0=False, out=None):
    """hb_belief_enumerate on torch tensors -> `ExactBelief`.

    rows [m, state_words] int32 on the GPU: the states now. history: a `PartnerHistory` of these roots seen from `seat`, a
    `LastMove` (the move is then the last one `rows` record), or None (no conditioning: the exact V0 belief). team: one
    `RulebasedAgent` per seat, whose lists the partners' moves are walked with, keyed by (partner_seed, the entry's draw, game id
    first_game_id + i): what their eval_moves was called with in the real game. replicas hands per root are drawn with (seed,
    draw, row id first_row_id + i). max_hands (default DEFAULT_MAX_HANDS, see there): a root with more hands than this gets
    status 1 and nothing else. marg0=True also fills the level-0 marginals. out: an optional tuple of the buffers (status, space,
    mass, n_hands, depth_used, fallback, marg, marg0 or None, hands, scratch [scratch_bytes(cfg, m, max_hands)] uint8) to write
    into. Nothing is read back to the host."""
    from .search import LastMove, PartnerHistory, last_move_uid

    L = K.lib()
    cfg = K.HbConfig(cfg.players, cfg.colors, cfg.ranks, cfg.hand_size, cfg.max_info, cfg.max_life, 0)
    if L.hb_config_validate(C.byref(cfg)) != 0:
        raise ValueError(f"invalid configuration {cfg!r}: {L.hb_last_error().decode()}")
    P, SW, H, NC = cfg.players, L.hb_state_words(C.byref(cfg)), cfg.hand_size, cfg.colors * cfg.ranks
    team = list(team)
    if len(team) != P:
        raise ValueError(f"one agent per seat: {P} players, {len(team)} agents")
    if not all(_is_rule_agent(a) for a in team):
        raise TypeError("belief_enumerate walks RulebasedAgent seats only: " + ", ".join(type(a).__name__ for a in team))
    if not isinstance(rows, torch.Tensor) or rows.dim() != 2 or rows.shape[1] != SW or rows.dtype != torch.int32 or not rows.is_contiguous():
        got = f"{rows.dtype} {tuple(rows.shape)}" if isinstance(rows, torch.Tensor) else type(rows).__name__
        raise ValueError(f"rows: expected a contiguous torch.int32 tensor of shape [m, {SW}], got {got}")
    m, R = rows.shape[0], int(replicas)
    if not 0 <= int(seat) < P:
        raise ValueError(f"seat {seat} out of range for {P} players")
    if not 1 <= R <= MAX_REPLICAS:
        raise ValueError(f"replicas must be 1..{MAX_REPLICAS}, got {replicas}")
    if int(max_hands) < 1:
        raise ValueError(f"max_hands must be >= 1, got {max_hands}")
    if history is not None and not isinstance(history, (PartnerHistory, LastMove)):
        raise TypeError(f"history must be a PartnerHistory, a LastMove or None, got {type(history).__name__}")
    if not rows.is_cuda:
        raise K.HbError("the state rows must live on the GPU (there is no CPU path)")
    dev = rows.device
    D = 0 if history is None else int(history.depth)
    hrows = hmoves = alive = valid = None
    draws = (C.c_uint64 * max(D, 1))()
    if history is not None:
        if history.m != m or history.state_words != SW:
            raise ValueError(f"the history holds {history.m} roots of {history.state_words} words, the rows are {tuple(rows.shape)}")
        if history.prev_rows.device != dev:
            raise ValueError(f"the history lives on {history.prev_rows.device}, the rows on {dev}")
        if not 1 <= D <= MAX_DEPTH:
            raise ValueError(f"the history's depth must be 1..{MAX_DEPTH}, got {D}")
        hrows = history.prev_rows.contiguous()
        hmoves = (last_move_uid(cfg, rows).view(1, m) if history.moves is None else history.moves).contiguous()
        alive = None if history.alive is None else history.alive.contiguous()
        valid = None if history.valid is None else history.valid.contiguous()
        for d in range(D):
            draws[d] = int(history.draws[d]) & 0xFFFFFFFFFFFFFFFF
    n_scratch = scratch_bytes(cfg, m, max_hands)
    specs = (((m,), torch.uint8), ((m,), torch.int64), ((D + 1, m), torch.int64), ((D + 1, m), torch.int32), ((m,), torch.int32),
             ((m,), torch.uint8), ((m, H, NC), torch.int64), ((m, H, NC), torch.int64), ((m, R), torch.int32),
             ((n_scratch,), torch.uint8))
    names = ("status", "space", "mass", "n_hands", "depth_used", "fallback", "marg", "marg0", "hands", "scratch")
    if out is None:
        bufs = [torch.empty(shape, dtype=dtype, device=dev) if (name != "marg0" or marg0) else None
                for name, (shape, dtype) in zip(names, specs)]
    else:
        bufs = list(out)
        if len(bufs) != len(specs):
            raise ValueError(f"out holds the {len(specs)} buffers {names}")
        for name, t, (shape, dtype) in zip(names, bufs, specs):
            if name == "marg0" and t is None:
                continue
            _check(t, shape, dtype, f"out ({name})", dev)
    tabs, lens = rule_tables(team)
    if m:   # (no roots: nothing to launch, and empty tensors have no address)
        with torch.cuda.device(dev):
            K.check(_fn()[0](C.byref(cfg), K.dptr(rows), m, int(seat), K.dptr(hrows), K.dptr(hmoves), K.dptr(alive), K.dptr(valid), D,
                             draws, int(partner_seed) & 0xFFFFFFFFFFFFFFFF, int(first_game_id), tabs, lens, int(max_hands), R,
                             int(seed) & 0xFFFFFFFFFFFFFFFF, int(draw) & 0xFFFFFFFFFFFFFFFF, int(first_row_id),
                             *[K.dptr(t) for t in bufs], K.current_stream()))
    return ExactBelief(*bufs[:9], cfg, int(seat))


def exact_rows(cfg, rows, hands, seat, seed, draw, first_row_id=0, out=None):
    """The drawn hand words as full, physically consistent state rows: rows [m, SW] int32 the states now, hands [m, R] int32 (u32
    bits; `ExactBelief.hands`) -> (rows_out [m * R, SW] int32, weights [m * R] int32), replica r of root i in row i * R + r.

    No placement code of its own: the EXISTING hb_belief_carry on copies of the current rows whose word 10 + seat is the drawn
    hand, with own_slot = revealed = drew = -1. Every card is then "kept" and takes its first free pool element, the rest of the
    pool is shuffled onto the undealt deck by the determinizer's keyed shuffle (seed, draw, row id first_row_id + i * R + r),
    and the weight is 1. Precondition, carry's own: `seat` is the rows' current player; a row where it is not, or that is not
    running, comes back unchanged with weight 0. `out`: an optional (rows_out, weights) pair to write into."""
    from .search import belief_carry

    if not isinstance(rows, torch.Tensor) or rows.dim() != 2 or rows.dtype != torch.int32:
        raise ValueError("rows: expected a torch.int32 tensor of shape [m, state_words]")
    m, SW = rows.shape
    if not isinstance(hands, torch.Tensor) or hands.dim() != 2 or hands.shape[0] != m or hands.dtype != torch.int32:
        raise ValueError(f"hands: expected a torch.int32 tensor of shape [{m}, R]")
    if not 0 <= int(seat) < cfg.players:
        raise ValueError(f"seat {seat} out of range for {cfg.players} players")
    R, dev = hands.shape[1], rows.device
    old = rows.view(m, 1, SW).expand(m, R, SW).contiguous()
    old[:, :, 10 + int(seat)] = hands
    minus = torch.full((m,), -1, dtype=torch.int32, device=dev)
    ones = torch.ones(m * R, dtype=torch.int32, device=dev)
    return belief_carry(cfg, rows.contiguous(), old.view(m * R, SW), ones, minus, minus, minus, int(seat), R, seed, draw,
                        first_row_id=first_row_id, out=out)


class ExactDeterminizer:
    """`ConditionedDeterminizer`'s interface on the exact belief: `belief_enumerate`, then `exact_rows` on the drawn hands."""

    def __init__(self, game="Hanabi-Full", players=2, config=None):
        from .evaluate import eval_config

        self.cfg = eval_config(game, players, config)
        self.players = self.cfg.players
        self.state_words = K.lib().hb_state_words(C.byref(self.cfg))

    @torch.no_grad()
    def sample_history(self, rows, history, team, seat, replicas, seed, draw, partner_seed, first_game_id, first_row_id=0,
                       max_hands=DEFAULT_MAX_HANDS, out=None):
        """rows [m, SW] the current states (seat `seat` to act), history a `PartnerHistory`, a `LastMove` or None, team one
        `RulebasedAgent` per seat -> (`BeliefSample`, `ExactBelief`). The sample's rows [m * replicas, SW] are the drawn hands as
        full rows (row ids first_row_id + i * replicas + r key the deck shuffle), its weights 1 (0: a root that is not running),
        n_surv = n_hands[1:] (the hands with a mass that reproduce the partner's last d + 1 moves), depth_used and fallback the
        belief's, ess None. A root of status 1 (more than max_hands hands) is reported, not filled: its rows are copies of the
        root with the deck reshuffled, and the caller decides what stands in for them. `out`: an optional (rows_out, weights
        int32) pair to write into (the weights then come back as that buffer)."""
        from .search import BeliefSample, _rows

        r = _rows(rows, self.state_words)
        belief = belief_enumerate(self.cfg, r, history, team, seat, replicas, seed, draw, partner_seed=partner_seed,
                                  first_game_id=first_game_id, first_row_id=first_row_id, max_hands=max_hands)
        det, w = exact_rows(self.cfg, r, belief.hands, seat, seed, draw, first_row_id=first_row_id, out=out)
        return BeliefSample(det, w if out is not None else w.long() & 0xFFFFFFFF, belief.n_hands[1:], belief.depth_used,
                            belief.fallback, None), belief
