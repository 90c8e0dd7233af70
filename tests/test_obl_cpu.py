"""Off-belief learning (hanabi_hip.obl, csrc/obl.hip), the parts that need no GPU: the numpy restatement of hb_obl_insert, the
CPU reference of one fictitious branch, the OBL invariant on that reference, the fixture the GPU tests use, and the argument
validation of the new entry point. tests/test_obl_gpu.py holds the kernel and the session to these references bit for bit.

The oracle env has no state import, so the reference reaches a determinized state the way a game would: the same moves replayed
on a deck in which the cards of the observer's hand and the undealt cards are the determinized ones (`branch_games`). That the
replay lands on the determinized row, word for word, is asserted for every game."""
import ctypes as C

import numpy as np
import pytest

import deep_play as D
from test_search_cpu import deck_size_of, determinize_ref

BELIEF_SEED = 9
# (game, players) -> turns of open-handed play (tests/deep_play.py) before the session's step; a multiple of the players, so
# that seat 0 is to act. Chosen here on the CPU (test_fixture_reaches_what_the_gpu_test_needs holds them to it).
FIXTURES = {("Hanabi-Full", 2): 118, ("Hanabi-Small", 2): 54, ("Hanabi-Small", 3): 45}


# ---- hb_obl_insert, restated -------------------------------------------------------------------------------------------------
def obl_insert_ref(rings, obs_tm1, actions, rewards, terminal, obs_t, legal_t, start):
    """include/hanabi_hip.h, hb_obl_insert, on numpy arrays, in place. rings = dict(obs_tm1 [cap, L], obs_t [cap, L], act [cap]
    int8, lms [cap, A] int8, rew [cap] f32, term [cap] uint8); rewards / terminal [P, n]."""
    cap = rings["act"].shape[0]
    P, n = rewards.shape
    for g in range(n):
        ended = np.flatnonzero(terminal[:, g] != 0)
        e = int(ended[0]) if len(ended) else P
        r = np.float32(rewards[0, g])
        for k in range(1, min(e, P - 1) + 1):
            r = np.float32(r + np.float32(rewards[k, g]))
        s = (start + g) % cap
        rings["obs_tm1"][s] = obs_tm1[g]
        rings["act"][s] = np.int32(actions[g]).astype(np.int8)
        rings["rew"][s] = r
        rings["term"][s] = e < P
        rings["obs_t"][s] = obs_t[g] if e == P else 0
        rings["lms"][s] = legal_t[g] if e == P else 0
    return rings


def pack_bits(obs):
    """int8 0/1 rows [n, L] -> the bit-packed int32 rows of a packed env (bit i = bit i & 31 of word i >> 5)."""
    n, L = obs.shape
    W = (L + 31) // 32
    padded = np.zeros((n, 32 * W), np.uint8)
    padded[:, :L] = obs != 0
    return np.packbits(padded, axis=1, bitorder="little").view("<u4").astype(np.uint32).view(np.int32).reshape(n, W)


# ---- the fixture: late states reached by open-handed play, with the history of every game's current deal ----------------------
class Fixture:
    """`turns` steps of deep_play.open_hand_moves on the auto-resetting oracle env (deep_play's seed and first game id).
    moves [turns, n]: what a HIP env of the same seed is stepped with to reach the same states; rows / obs / legal: the states and
    what the seat to act sees; per game the deck, start player and moves of the deal in progress."""

    def __init__(self, game, players, turns):
        from oracle import oracle_py as O

        self.game, self.players, self.turns, self.n = game, players, turns, D.N_GAMES
        self.cfg = O.make_config(game, players, D.FLAGS)
        self.cfg0 = O.make_config(game, players, 0)
        env = O.OracleEnv(self.cfg, self.n, seed=D.SEED, first_game_id=D.FIRST_GAME_ID)
        rng = np.random.default_rng(D.SEED)
        episode, start, hist = [0] * self.n, [0] * self.n, [[] for _ in range(self.n)]
        legal = env.observe()["legal"]
        self.moves = np.zeros((turns, self.n), np.int32)
        for t in range(turns):
            act = D.open_hand_moves(self.cfg, env.export_state(), legal, rng, D.P_RAND)
            self.moves[t] = act
            out = env.step(act)
            legal = out["legal"]
            for g in range(self.n):
                hist[g].append(int(act[g]))
                if out["terminal"][g]:
                    episode[g], start[g], hist[g] = episode[g] + 1, (t + 1) % players, []
        assert env.illegal_count() == 0
        self.rows = env.export_state()
        seen = env.observe()
        self.obs, self.legal = seen["obs"], seen["legal"]
        self.seat = turns % players
        assert (((self.rows[:, 0] >> 13) & 7) == self.seat).all()
        self.start, self.hist = start, hist
        self.decks = [O.shuffled_deck(self.cfg, D.SEED, D.FIRST_GAME_ID + g, episode[g]) for g in range(self.n)]


_FIXTURES = {}


def fixture(game, players):
    key = (game, players)
    if key not in _FIXTURES:
        _FIXTURES[key] = Fixture(game, players, FIXTURES[key])
    return _FIXTURES[key]


def hand_positions(cfg, deck_size, start, hist):
    """Deck position of the card in every hand slot after `hist` (oracle/hanabi_oracle.c: deal_one, remove_from_hand)."""
    P, H = cfg.players, cfg.hand_size
    hands, pos = [[] for _ in range(P)], 0

    def deal():
        nonlocal pos
        while pos < deck_size:
            short = [p for p in range(P) if len(hands[p]) < H]
            if not short:
                break
            hands[short[0]].append(pos)
            pos += 1

    deal()
    cur = start
    for u in hist:
        if u < 2 * H:
            hands[cur].pop(u % H)
        deal()
        cur = (cur + 1) % P
    return hands, pos


def _replay(fx, g, deck):
    from oracle import oracle_py as O

    env = O.OracleEnv(fx.cfg0, 1, seed=D.SEED, first_game_id=D.FIRST_GAME_ID + g, decks=np.asarray(deck, np.uint8)[None],
                      start_player=fx.start[g])
    for u in fx.hist[g]:
        env.step_noobs(np.asarray([u], np.int32))
    assert env.illegal_count() == 0
    return env


def _same_state(cfg, a, b, deck_pos):
    """Two state rows agree in everything but the deck bytes already dealt and the per-seat bookkeeping of words 3 - 7."""
    P, Dk = cfg.players, deck_size_of(cfg)
    words = [0, 1, 2, 8, 9] + list(range(10, 10 + 3 * P))
    da, db = (np.ascontiguousarray(x[10 + 3 * P:], dtype="<u4").view(np.uint8) for x in (a, b))
    return all(int(a[w]) == int(b[w]) for w in words) and np.array_equal(da[deck_pos:Dk], db[deck_pos:Dk])


def branch_games(fx, draw, seed=BELIEF_SEED):
    """One oracle env per game, in the determinized state S'_t of seat fx.seat: determinize_ref (replicas = 1, row ids from the
    first game id), then the deal's moves replayed on the deck that has the determinized cards where the seat's hand and the
    undealt cards came from. -> (envs, det_rows, weights)."""
    det, w = determinize_ref(fx.cfg0, fx.rows, fx.seat, 1, seed, draw, first_row_id=D.FIRST_GAME_ID)
    Dk, P = deck_size_of(fx.cfg0), fx.players
    envs = []
    for g in range(fx.n):
        real = _replay(fx, g, fx.decks[g])   # the machinery itself: the recorded deal and moves give the real row
        hands, pos = hand_positions(fx.cfg0, Dk, fx.start[g], fx.hist[g])
        assert _same_state(fx.cfg0, real.export_state()[0], fx.rows[g], 0) and pos == Dk - (int(fx.rows[g, 0]) & 63)
        deck = np.array(fx.decks[g], np.uint8)
        hand = int(det[g, 10 + fx.seat])
        for s, q in enumerate(hands[fx.seat]):
            deck[q] = (hand >> (5 * s)) & 31
        deck[pos:] = np.ascontiguousarray(det[g, 10 + 3 * P:], dtype="<u4").view(np.uint8)[pos:Dk]
        env = _replay(fx, g, deck)
        assert _same_state(fx.cfg0, env.export_state()[0], det[g], pos), f"game {g}: the replay misses the determinized row"
        envs.append(env)
    return envs, det, w


def obl_branch_ref(fx, a_t, t, partner_moves=None, rules=None, seed=BELIEF_SEED):
    """The fictitious branch of OffBeliefSession's step t from the fixture's states (seat fx.seat trained): every game of
    branch_games stepped with a_t, then with each partner's move — partner_moves [P, n] (row k: the move of seat + k), or the
    rule oracle's on `rules` ([(kind, arg, threshold)]) with draw t * P + k. -> dict(rewards [P, n] f32, terminal [P, n] int8,
    obs_t [n, L], legal_t [n, A], weights, det_rows, moves [P, n])."""
    P, n = fx.players, fx.n
    envs, det, w = branch_games(fx, t, seed)
    rew, term = np.zeros((P, n), np.float32), np.zeros((P, n), np.int8)
    moves = np.zeros((P, n), np.int32)
    obs_t, legal_t = np.zeros_like(fx.obs), np.zeros_like(fx.legal)
    for g, env in enumerate(envs):
        for k in range(P):
            if k == 0:
                u = int(a_t[g])
            elif partner_moves is not None:
                u = int(partner_moves[k][g])
            else:
                u = int(env.rule_act(rules, seed, t * P + k)[0][0])
            moves[k, g] = u
            out = env.step(np.asarray([u], np.int32))
            rew[k, g], term[k, g] = out["reward"][0], out["terminal"][0]
        obs_t[g], legal_t[g] = out["obs"][0], out["legal"][0]
    return dict(rewards=rew, terminal=term, obs_t=obs_t, legal_t=legal_t, weights=w, det_rows=det, moves=moves)


def expected_rows(fx, a_t, ref, capacity, start=0):
    """The six rings (packed observation rows) after the session's insert of `ref` at `start`, sentinels elsewhere: None."""
    W, A = (fx.obs.shape[1] + 31) // 32, fx.legal.shape[1]
    rings = dict(obs_tm1=np.zeros((capacity, W), np.int32), obs_t=np.zeros((capacity, W), np.int32), act=np.zeros(capacity, np.int8),
                 lms=np.zeros((capacity, A), np.int8), rew=np.zeros(capacity, np.float32), term=np.zeros(capacity, np.uint8))
    return obl_insert_ref(rings, pack_bits(fx.obs), a_t, ref["rewards"], ref["terminal"], pack_bits(ref["obs_t"]), ref["legal_t"], start)


def piers_table():
    from hanabi_agents.rule_based import predefined_rules as PR

    return [(r.kind, r.arg, r.threshold) for r in PR.piers_rules]


def end_steps(terminal):
    P = terminal.shape[0]
    return np.where((terminal != 0).any(0), (terminal != 0).argmax(0), P)


# ---- tests ---------------------------------------------------------------------------------------------------------------------
def test_obl_is_exported():
    import hanabi_hip
    from hanabi_hip import _capi

    assert "hb_obl_insert" in _capi.SIGNATURES and hasattr(hanabi_hip.lib(), "hb_obl_insert")
    assert hasattr(hanabi_hip, "OffBeliefSession") and "OffBeliefSession" in hanabi_hip.__all__
    from hanabi_agents.rlax_dqn import DQNAgent

    assert callable(DQNAgent.add_transitions_dense)


def test_argument_validation_needs_no_gpu():
    import hanabi_hip

    L = hanabi_hip.lib()
    one = C.c_void_p(16)
    err = lambda: L.hb_last_error()
    ok = [one] * 12 + [4, 2, 84, 20, 256, 0, None]
    for i in range(12):
        args = list(ok)
        args[i] = None
        assert L.hb_obl_insert(*args) < 0 and b"null" in err()

    def call(n=4, n_steps=2, row_bytes=84, A=20, cap=256, start=0):
        return L.hb_obl_insert(*([one] * 12), n, n_steps, row_bytes, A, cap, start, None)

    assert call(n=-1) < 0 and b"n must" in err()
    assert call(n_steps=0) < 0 and b"n_steps" in err()
    assert call(n_steps=6) < 0 and b"n_steps" in err()
    assert call(cap=0) < 0 and b"capacity" in err()
    assert call(cap=-5) < 0 and b"capacity" in err()
    assert call(row_bytes=0) < 0 and b"row_bytes" in err()
    assert call(A=0) < 0 and b"n_actions" in err()
    assert call(n=300) < 0 and b"ring range" in err()
    assert call(start=256) < 0 and b"ring range" in err()
    assert call(start=-1) < 0 and b"ring range" in err()
    assert call(n=0) == 0       # empty: no-op, nothing is launched


def test_insert_restatement_on_a_hand_worked_batch():
    P, n, cap = 3, 4, 5
    rings = dict(obs_tm1=np.full((cap, 2), 7, np.int8), obs_t=np.full((cap, 2), 7, np.int8), act=np.full(cap, 7, np.int8),
                 lms=np.full((cap, 3), 7, np.int8), rew=np.full(cap, 7, np.float32), term=np.full(cap, 7, np.uint8))
    rewards = np.array([[1, 1, 1, 1], [2, 2, 2, 2], [4, 4, 4, 4]], np.float32)
    terminal = np.array([[0, 1, 0, 0], [0, 0, 0, 1], [0, 1, 1, 1]], np.int8)   # never / step 0 (and again) / last step / step 1
    obs_tm1, obs_t = np.arange(8, dtype=np.int8).reshape(4, 2), 10 + np.arange(8, dtype=np.int8).reshape(4, 2)
    legal = np.ones((4, 3), np.int8)
    obl_insert_ref(rings, obs_tm1, np.array([3, 4, 5, 6]), rewards, terminal, obs_t, legal, start=3)
    order = [3, 4, 0, 1]   # the batch wraps
    assert rings["rew"][order].tolist() == [7.0, 1.0, 7.0, 3.0] and rings["term"][order].tolist() == [0, 1, 1, 1]
    assert rings["act"][order].tolist() == [3, 4, 5, 6] and np.array_equal(rings["obs_tm1"][order], obs_tm1)
    assert np.array_equal(rings["obs_t"][3], obs_t[0]) and not rings["obs_t"][[4, 0, 1]].any()
    assert rings["lms"][3].all() and not rings["lms"][[4, 0, 1]].any()
    assert rings["act"][2] == 7 and rings["rew"][2] == 7 and (rings["obs_t"][2] == 7).all()   # untouched


@pytest.mark.parametrize("game,players", list(FIXTURES))
def test_the_learner_cannot_tell_the_fictitious_state_from_the_real_one(game, players):
    """The OBL invariant on the reference: on states reached by play, the trained seat's observation and legal mask of the
    determinized state are those of the real state — so the move chosen on the real observation is legal in the branch and the
    replay row's first observation is the real one."""
    fx = fixture(game, players)
    envs, det, w = branch_games(fx, draw=0)
    assert (w > 0).all(), "a dead replica on a state reached by play"
    differs = 0
    for g, env in enumerate(envs):
        seen = env.observe()
        assert np.array_equal(seen["obs"][0], fx.obs[g]) and np.array_equal(seen["legal"][0], fx.legal[g])
        differs += int(det[g, 10 + fx.seat]) != int(fx.rows[g, 10 + fx.seat])
    assert differs > 0


@pytest.mark.parametrize("game,players", list(FIXTURES))
def test_fixture_reaches_what_the_gpu_test_needs(game, players):
    """Whatever the trained seat plays: games in their final round end at step 0 (one turn left) and at a later step (more than
    one left, at most P), and at least a quarter of the fictitious hands differ from the real ones. With uniformly random legal
    moves of the trained seat the reference shows both kinds of ending and rows that do not end."""
    from oracle import oracle_py as O

    fx = fixture(game, players)
    assert fx.turns % players == 0 and fx.seat == 0
    deck, left = fx.rows[:, 0] & 63, (fx.rows[:, 0] >> 16) & 7
    assert ((deck == 0) & (left == 1)).sum() >= 1, "no game ends at step 0 whatever is played"
    assert ((deck == 0) & (left >= 2) & (left <= players)).sum() >= 1, "no game ends at a later step whatever is played"
    a_t = O.random_legal_actions(fx.legal, 3, 0, D.FIRST_GAME_ID)
    ref = obl_branch_ref(fx, a_t, 0, rules=piers_table())
    e = end_steps(ref["terminal"])
    assert (e == 0).any() and ((e > 0) & (e < players)).any() and (e == players).any()
    hands = np.array([[int(r[10 + fx.seat]) for r in rows] for rows in (fx.rows, ref["det_rows"])])
    assert 4 * int((hands[0] != hands[1]).sum()) >= fx.n, "fewer than a quarter of the fictitious hands differ"
    assert (ref["weights"] > 0).all()
    # nothing a finished game emits is a reward or an ending
    for g in np.flatnonzero(e < players - 1):
        assert not ref["terminal"][e[g] + 1:, g].any() and not ref["rewards"][e[g] + 1:, g].any()
    rows = expected_rows(fx, a_t, ref, 256, start=200)
    ended = np.flatnonzero(e < players)
    assert not rows["obs_t"][(200 + ended) % 256].any() and rows["term"][(200 + ended) % 256].all()
