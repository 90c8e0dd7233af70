"""The search belief conditioned on the partner's last L moves, the parts that need no GPU: numpy restatements of
hb_belief_splice_alive and hb_belief_select_depth (include/hanabi_hip.h), hand-worked cases of every branch, their reduction to
the depth-1 rule, PartnerHistory's alive masks against games played on the CPU oracle, the exactness of the depth-2 survivors by
enumeration, and argument validation. tests/test_search_depth_gpu.py holds the kernels to these restatements byte for byte."""
import ctypes as C

import numpy as np
import pytest

from test_search_belief_cpu import _hand_positions, _labelled, _replay, _rules, _violations, select_ref, splice_ref
from test_search_cpu import FULL_SCRIPT, SMALL_SCRIPTS, _oracle, determinize_ref, enumerate_hands, hand_types


# ---- the restatements -------------------------------------------------------------------------------------------------------------
def splice_hand_ref(prev_hand, alive, cand_hand):
    """The hand word of hb_belief_splice_alive: the occupied slots of prev_hand in order; an alive one takes the next card of
    cand_hand while that has one, every other keeps its own."""
    out, j = int(prev_hand), 0
    for s in range(5):
        if (out >> (5 * s)) & 31 == 31:
            continue
        c = (int(cand_hand) >> (5 * j)) & 31 if j < 5 else 31
        if (alive >> s) & 1 and c != 31:
            out = (out & ~(31 << (5 * s))) | (c << (5 * s))
            j += 1
    return out


def splice_alive_ref(prev_rows, alive, det_rows, seat, K):
    """hb_belief_splice_alive: prev_rows [m, SW], alive [m] or None, det_rows [m * K, SW] -> [K * m, SW]."""
    prev_rows, det_rows = np.asarray(prev_rows).astype(np.uint32), np.asarray(det_rows).astype(np.uint32)
    m = prev_rows.shape[0]
    out = np.empty((K * m, prev_rows.shape[1]), np.uint32)
    for k in range(K):
        for i in range(m):
            out[k * m + i] = prev_rows[i]
            out[k * m + i, 10 + seat] = splice_hand_ref(prev_rows[i, 10 + seat], 0xFF if alive is None else int(alive[i]),
                                                        det_rows[i * K + k, 10 + seat])
    return out


def select_depth_ref(src_rows, det_rows, weights, hyp_moves, actual, valid, K, R):
    """hb_belief_select_depth: hyp_moves [D, K, m], actual [D, m], valid [D, m] or None -> (rows uint32 [m * R, SW], weights
    uint32 [m * R], n_surv int32 [D, m], depth_used int32 [m], fallback uint8 [m])."""
    src_rows, det_rows = np.asarray(src_rows).astype(np.uint32), np.asarray(det_rows).astype(np.uint32)
    weights, actual = np.asarray(weights).astype(np.uint32), np.asarray(actual)
    D, m = actual.shape
    hyp = np.asarray(hyp_moves).reshape(D, K, m)
    rows, w = np.empty((m * R, src_rows.shape[1]), np.uint32), np.empty(m * R, np.uint32)
    n_surv, used, fallback = np.zeros((D, m), np.int32), np.zeros(m, np.int32), np.zeros(m, np.uint8)
    for i in range(m):
        L = 0
        if (int(src_rows[i, 0]) >> 19) & 3 == 0:
            while L < D and (valid is None or valid[L][i] != 0):
                L += 1
        passed = []
        for k in range(K):
            p = 0
            while weights[i * K + k] != 0 and p < L and hyp[p, k, i] == actual[p, i]:
                p += 1
            passed.append(p)
        for d in range(L):
            n_surv[d, i] = sum(1 for p in passed if p >= d + 1)
            if n_surv[d, i] >= 1:
                used[i] = d + 1
        fallback[i] = 2 if L == 0 else 1 if used[i] == 0 else 0
        picks = [k for k in range(K) if passed[k] >= used[i]][:R] if used[i] else list(range(R))
        for j in range(R):
            if j < len(picks):
                rows[i * R + j], w[i * R + j] = det_rows[i * K + picks[j]], weights[i * K + picks[j]]
            else:
                rows[i * R + j], w[i * R + j] = src_rows[i], 0
    return rows, w, n_surv, used, fallback


def occupied_mask(hand):
    return sum(1 << s for s in range(5) if (int(hand) >> (5 * s)) & 31 != 31)


def own_move_ref(alive, uid, H):
    """PartnerHistory.own_move on one mask: a play or discard of slot s clears the s-th set bit, if there is one."""
    if not 0 <= uid < 2 * H:
        return alive
    s, seen = uid % H, 0
    for b in range(5):
        if (alive >> b) & 1:
            if seen == s:
                return alive & ~(1 << b)
            seen += 1
    return alive


# ---- hand-worked cases: the splice -----------------------------------------------------------------------------------------------
def _hand(*cards):
    cards = list(cards) + [31] * (5 - len(cards))
    return sum(c << (5 * s) for s, c in enumerate(cards))


@pytest.mark.parametrize("name,prev,alive,cand,want", [
    ("every slot alive, equal sizes: the candidate's hand", _hand(1, 2, 3, 4, 5), 0b11111, _hand(11, 12, 13, 14, 15), _hand(11, 12, 13, 14, 15)),
    ("the first slot dead", _hand(1, 2, 3, 4, 5), 0b11110, _hand(11, 12, 13, 14, 15), _hand(1, 11, 12, 13, 14)),
    ("a middle slot dead", _hand(1, 2, 3, 4, 5), 0b11011, _hand(11, 12, 13, 14, 15), _hand(11, 12, 3, 13, 14)),
    ("the last slot dead", _hand(1, 2, 3, 4, 5), 0b01111, _hand(11, 12, 13, 14, 15), _hand(11, 12, 13, 14, 5)),
    ("two dead", _hand(1, 2, 3, 4, 5), 0b01010, _hand(11, 12, 13, 14, 15), _hand(1, 11, 3, 12, 5)),
    ("all dead: the previous hand", _hand(1, 2, 3, 4, 5), 0, _hand(11, 12, 13, 14, 15), _hand(1, 2, 3, 4, 5)),
    ("the deck ran out: the hand shrank to 3, two of the old five are gone", _hand(1, 2, 3, 4, 5), 0b10101, _hand(11, 12, 13),
     _hand(11, 2, 12, 4, 13)),
    ("a candidate that runs out of cards keeps the previous row's", _hand(1, 2, 3, 4, 5), 0b11111, _hand(11, 12, 13), _hand(11, 12, 13, 4, 5)),
    ("an empty slot stays empty although its alive bit is set", _hand(1, 2, 3, 4), 0b11111, _hand(11, 12, 13, 14, 15), _hand(11, 12, 13, 14)),
    ("a hand of two (Small)", _hand(6, 7), 0b10, _hand(8, 9), _hand(6, 8)),
])
def test_hand_worked_splice(name, prev, alive, cand, want):
    assert splice_hand_ref(prev, alive, cand) == want, name
    m, K, SW, seat = 2, 3, 32, 1
    rng = np.random.default_rng(5)
    prev_rows = rng.integers(0, 2 ** 32, (m, SW), dtype=np.uint64).astype(np.uint32)
    det = rng.integers(0, 2 ** 32, (m * K, SW), dtype=np.uint64).astype(np.uint32)
    prev_rows[:, 10 + seat] = [_hand(20, 21, 22, 23, 24), prev]
    det[:, 10 + seat] = _hand(0, 0, 0, 0, 0)
    det[K + 1, 10 + seat] = cand   # candidate (1, 1) is the case
    out = splice_alive_ref(prev_rows, np.array([0, alive], np.uint8), det, seat, K).reshape(K, m, SW)
    assert out[1, 1, 10 + seat] == want and out[1, 0, 10 + seat] == prev_rows[0, 10 + seat], name
    same = np.ones(SW, bool)
    same[10 + seat] = False
    assert all(np.array_equal(out[k, i][same], prev_rows[i][same]) for k in range(K) for i in range(m))   # only the hand word
    if alive == 0b11111:   # alive = None means every slot alive
        assert splice_alive_ref(prev_rows[1:], None, det[K:], seat, K)[1, 10 + seat] == want


def test_all_slots_alive_is_the_depth_1_splice():
    O = _oracle()
    for game, players, seat in (("Hanabi-Full", 2, 1), ("Hanabi-Full", 5, 3), ("Hanabi-Small", 2, 0)):
        cfg = O.make_config(game, players, 0)
        env = O.OracleEnv(cfg, 6, seed=4)
        legal = env.observe()["legal"]
        for t in range(7):
            legal = env.step(O.random_legal_actions(legal, 5, t))["legal"]
        rows = env.export_state()
        K = 3
        det, _ = determinize_ref(cfg, rows, seat, K, 11, 3)
        want = splice_ref(rows, det, seat, K)
        assert np.array_equal(splice_alive_ref(rows, None, det, seat, K), want)
        assert np.array_equal(splice_alive_ref(rows, np.full(6, 0x1F, np.uint8), det, seat, K), want)
        assert np.array_equal(splice_alive_ref(rows, np.array([occupied_mask(r[10 + seat]) for r in rows], np.uint8), det, seat, K), want)


# ---- hand-worked cases: the selection ---------------------------------------------------------------------------------------------
# root 1 of a two-root call, K = 5, R = 3, depth 3; hyp[d] lists the five candidates' moves at entry d, the real moves are 7, 8, 9
@pytest.mark.parametrize("name,weights,hyp,valid,picks,want_w,n_surv,used,fallback", [
    ("every candidate reproduces every move", [3] * 5, [[7] * 5, [8] * 5, [9] * 5], [1, 1, 1], [0, 1, 2], [3, 3, 3], [5, 5, 5], 3, 0),
    ("the deepest level decides", [3, 4, 5, 6, 7], [[7] * 5, [8, 1, 8, 8, 8], [9, 9, 1, 9, 9]], [1, 1, 1], [0, 3, 4], [3, 6, 7],
     [5, 4, 3], 3, 0),
    ("fewer survivors than replicas", [3, 4, 5, 6, 7], [[7] * 5, [8, 1, 8, 8, 1], [1, 9, 9, 1, 9]], [1, 1, 1], [2, None, None], [5, 0, 0],
     [5, 3, 1], 3, 0),
    ("a match behind a miss does not count", [3] * 5, [[1, 7, 7, 7, 7], [8, 1, 8, 8, 8], [9, 9, 1, 1, 1]], [1, 1, 1], [2, 3, 4], [3, 3, 3],
     [4, 3, 0], 2, 0),
    ("depth_used < L: nobody reproduces the oldest move", [3] * 5, [[7, 7, 1, 7, 7], [8, 1, 8, 8, 8], [1] * 5], [1, 1, 1], [0, 3, 4],
     [3, 3, 3], [4, 3, 0], 2, 0),
    ("an invalid middle entry cuts the chain", [3] * 5, [[7, 1, 7, 1, 7], [1] * 5, [9] * 5], [1, 0, 1], [0, 2, 4], [3, 3, 3], [3, 0, 0], 1, 0),
    ("no survivor at any depth: fallback 1", [3, 4, 0, 6, 7], [[1] * 5, [8] * 5, [9] * 5], [1, 1, 1], [0, 1, 2], [3, 4, 0], [0, 0, 0], 0, 1),
    ("an invalid newest entry: fallback 2", [3, 4, 5, 6, 7], [[7] * 5, [8] * 5, [9] * 5], [0, 1, 1], [0, 1, 2], [3, 4, 5], [0, 0, 0], 0, 2),
    ("a weight-0 candidate passes nothing", [0, 3, 0, 3, 3], [[7] * 5, [8] * 5, [9, 9, 9, 1, 9]], [1, 1, 1], [1, 4, None], [3, 3, 0],
     [3, 3, 2], 3, 0),
])
def test_hand_worked_selection(name, weights, hyp, valid, picks, want_w, n_surv, used, fallback):
    m, K, R, D = 2, 5, 3, 3
    src, det = _labelled(m, K)
    # root 0: candidates 2 and 4 alone reproduce both usable moves (its oldest entry is invalid); roots do not leak into each other
    w = np.array([9, 0, 9, 9, 9] + weights, np.uint32)
    hyp0 = [[5, 5, 5, 1, 5], [1, 6, 6, 6, 6], [0] * 5]
    hyp_moves = np.stack([np.stack([np.array(hyp0[d]), np.array(hyp[d])], 1) for d in range(D)])   # [D, K, m]
    actual = np.array([[5, 7], [6, 8], [4, 9]])
    rows, ow, ns, du, fb = select_depth_ref(src, det, w, hyp_moves, actual, np.array([[1, 1, 0], valid], np.uint8).T, K, R)
    assert ns[:, 0].tolist() == [3, 2, 0] and int(du[0]) == 2 and int(fb[0]) == 0
    assert np.array_equal(rows[0], det[2]) and np.array_equal(rows[1], det[4]) and np.array_equal(rows[2], src[0])
    assert [int(x) for x in ow[:3]] == [9, 9, 0]
    assert ns[:, 1].tolist() == n_surv and int(du[1]) == used and int(fb[1]) == fallback, name
    for j, k in enumerate(picks):
        assert np.array_equal(rows[R + j], src[1] if k is None else det[K + k]), name
    assert [int(x) for x in ow[R:]] == want_w, name


def test_a_finished_root_is_never_filtered():
    m, K, R, D = 2, 5, 3, 2
    src, det = _labelled(m, K)
    src[1, 0] = 2 << 19
    rows, ow, ns, du, fb = select_depth_ref(src, det, np.full(m * K, 2, np.uint32), np.full((D, K, m), 7), np.full((D, m), 7), None, K, R)
    assert fb.tolist() == [0, 2] and du.tolist() == [2, 0] and ns.tolist() == [[5, 0], [5, 0]]
    assert np.array_equal(rows[R:], det[K:K + R]) and (ow == 2).all()


@pytest.mark.parametrize("seed", range(4))
def test_depth_1_is_the_depth_1_selection(seed):
    rng = np.random.default_rng(seed)
    m, K, R = 6, 9, 4
    src, det = _labelled(m, K)
    src[2, 0] = 1 << 19
    w = rng.integers(0, 3, m * K).astype(np.uint32)
    hyp, actual = rng.integers(0, 2, (K, m)), rng.integers(0, 2, m)
    hyp[:, 4] = 1 - actual[4]   # a root without a survivor
    for valid in (None, rng.integers(0, 2, m).astype(np.uint8)):
        a = select_ref(src, det, w, hyp, actual, valid, K, R)
        b = select_depth_ref(src, det, w, hyp[None], actual[None], None if valid is None else valid[None], K, R)
        assert all(np.array_equal(x, y) for x, y in zip(a, (b[0], b[1], b[2][0], b[4])))
        assert np.array_equal(b[3], (a[3] == 0).astype(np.int32))


# ---- alive tracking against games on the CPU oracle ---------------------------------------------------------------------------------
def _careful_uid(cfg, row, legal, rng):
    """A random legal move that never misplays (the mover's cards are read off the row), so that games run the deck out. (With
    two players nobody moves twice once the deck is empty, so a shrunken hand never meets a stored entry in play: the hand-worked
    cases cover it.)"""
    seat, w1, H, R = (int(row[0]) >> 13) & 7, int(row[1]), cfg.hand_size, cfg.ranks
    hand = int(row[10 + seat])
    ok = []
    for u in np.flatnonzero(legal):
        if H <= u < 2 * H:
            card = (hand >> (5 * (u - H))) & 31
            if (w1 >> (3 * (card // R))) & 7 != card % R:
                continue
        ok.append(int(u))
    return ok[rng.integers(len(ok))]


def _games():
    """(name, cfg, deck or None, moves or seed)."""
    O = _oracle()
    small, full = O.make_config("Hanabi-Small", 2, 0), O.make_config("Hanabi-Full", 2, 0)
    out = [(f"small script {j}", small, deck, moves) for j, (deck, moves) in enumerate(SMALL_SCRIPTS)]
    out.append(("full script", full, FULL_SCRIPT[0], FULL_SCRIPT[1]))
    out += [(f"full careful {s}", full, None, s) for s in (1, 2)] + [(f"small careful {s}", small, None, s) for s in (1, 2, 3)]
    return out


@pytest.mark.parametrize("game", range(10))
def test_alive_masks_carry_the_current_hand_back_to_every_stored_state(game):
    """Both seats of a 2-player game keep a PartnerHistory of depth 8 as SearchPlayer does (own_move with the move made two plies
    ago, then push of the state the partner moved from). At every turn and for every stored entry, the TRUE current row spliced
    into the stored row with the tracked mask is the stored row word for word — and still is after the alive slots of the stored
    row were overwritten with garbage: the rule reads only the public cards of the old hand. The torch masks are PartnerHistory's,
    the numpy ones the restatement's."""
    import torch

    from hanabi_hip import PartnerHistory, last_move_uid, make_config

    O = _oracle()
    name, cfg, deck, script = _games()[game]
    H, D = cfg.hand_size, 8
    env = O.OracleEnv(cfg, 1, seed=7 if deck is None else 1, decks=None if deck is None else np.asarray(deck, np.uint8)[None])
    rng = np.random.default_rng(script if deck is None else 0)
    hcfg = make_config("Hanabi-Small" if cfg.colors == 2 else "Hanabi-Full", 2, 0)
    hist = [PartnerHistory(hcfg, 1, D, "cpu") for _ in range(2)]
    ref = [[] for _ in range(2)]        # per seat: [(stored row, alive mask)], newest first
    mine = [None, None]                 # the move each seat made two plies ago
    legal = env.observe()["legal"][0]
    states, kinds, checked, dead_seen, plies = [env.export_state()[0].copy()], set(), 0, False, 0
    for t in range(200):
        row = states[-1]
        if (int(row[0]) >> 19) & 3:
            break
        me = (int(row[0]) >> 13) & 7
        if t >= 1:   # the partner moved from states[-2]
            prev = states[-2]
            if mine[me] is not None:
                hist[me].own_move(torch.tensor([mine[me]]))
                ref[me] = [(r, own_move_ref(a, mine[me], H)) for r, a in ref[me]]
            uid_prev = int(last_move_uid(hcfg, torch.as_tensor(row[None].astype(np.int64)))[0])
            hist[me].push(torch.as_tensor(prev[None].astype(np.uint32).view(np.int32)), [uid_prev], t, [1], seat=me)
            ref[me] = ([(prev.copy(), occupied_mask(prev[10 + me]))] + ref[me])[:D]
            assert hist[me].filled == len(ref[me]) and hist[me].draws[:len(ref[me])] == list(range(t, t - 2 * len(ref[me]), -2))
            for d, (stored, alive) in enumerate(ref[me]):
                assert int(hist[me].alive[d, 0]) == alive and int(hist[me].valid[d, 0]) == 1
                assert np.array_equal(hist[me].prev_rows[d, 0].numpy().view(np.uint32), stored.astype(np.uint32))
                got = splice_alive_ref(stored[None], np.array([alive], np.uint8), row[None], me, 1)[0]
                assert np.array_equal(got, stored.astype(np.uint32)), (name, t, d)
                junk = stored.copy()
                hand = int(junk[10 + me])
                for s in range(5):
                    if (alive >> s) & 1 and (hand >> (5 * s)) & 31 != 31:
                        hand = (hand & ~(31 << (5 * s))) | (((7 * s + t) % 30) << (5 * s))
                junk[10 + me] = hand
                assert np.array_equal(splice_alive_ref(junk[None], np.array([alive], np.uint8), row[None], me, 1)[0], stored.astype(np.uint32))
                checked += 1
                dead_seen |= alive != occupied_mask(stored[10 + me])
        if deck is None:
            uid = _careful_uid(cfg, row, legal, rng)
        elif t < len(script):
            uid = script[t]
        else:
            break
        mine[me] = uid
        kinds.add(0 if uid < H else 1 if uid < 2 * H else 2 if uid < 2 * H + cfg.colors else 3)
        legal = env.step(np.asarray([uid], np.int32))["legal"][0]
        assert env.illegal_count() == 0
        states.append(env.export_state()[0].copy())
        plies += 1
    print(name, "plies", plies, "entries checked", checked)
    assert checked > plies and dead_seen
    if deck is None or cfg.colors == 5:
        assert kinds == {0, 1, 2, 3}
    if cfg.colors == 5:
        assert plies >= 30


# ---- exactness by enumeration ---------------------------------------------------------------------------------------------------------
class Scene2:
    """A Small 2-player game: `moves` on `deck`, the partner's rule-list move a_old from S_old, my move `mine`, the partner's
    rule-list move a_new from S_new; I am to act in S. moves_under(hand) = what the partner's rule list plays in S_new and in
    S_old had I held `hand` NOW, and the hands I would have held then — the script replayed on a deck with my current cards and
    the undealt ones swapped (a hand in the V0 support answers every hint as the real one did, so the replay is legal; the cards
    I gave up since are public and stay where they are)."""

    def __init__(self, deck, moves, mine):
        O = _oracle()
        self.cfg = O.make_config("Hanabi-Small", 2, 0)
        self.deck, self.moves, self.mine = list(deck), list(moves), int(mine)
        env = _replay(self.cfg, deck, moves)
        self.old_row = env.export_state()[0].copy()
        self.partner = (int(self.old_row[0]) >> 13) & 7
        self.seat = 1 - self.partner
        self.a_old = int(env.rule_act(_rules(), 1, 1)[0][0])
        env.step(np.asarray([self.a_old], np.int32))
        self.ok = env.illegal_count() == 0 and (int(env.export_state()[0, 0]) >> 19) & 3 == 0
        self.ok = self.ok and bool(env.observe()["legal"][0][self.mine])
        if not self.ok:
            return
        env.step(np.asarray([self.mine], np.int32))
        self.new_row = env.export_state()[0].copy()
        self.ok = env.illegal_count() == 0 and (int(self.new_row[0]) >> 19) & 3 == 0
        if not self.ok:
            return
        self.a_new = int(env.rule_act(_rules(), 1, 1)[0][0])
        env.step(np.asarray([self.a_new], np.int32))
        self.row = env.export_state()[0].copy()
        self.ok = env.illegal_count() == 0 and (int(self.row[0]) >> 19) & 3 == 0
        hands, pos = _hand_positions(self.cfg, self.moves + [self.a_old, self.mine, self.a_new])
        self.my_pos, self.undealt = hands[self.seat], list(range(pos, len(deck)))
        # the masks as PartnerHistory keeps them: S_old pushed with every slot alive, my move, S_new pushed
        self.alive = [occupied_mask(self.new_row[10 + self.seat]),
                      own_move_ref(occupied_mask(self.old_row[10 + self.seat]), self.mine, self.cfg.hand_size)]
        self._cache = {}

    def _same_but_my_hand(self, got, want):
        same = np.ones(len(got), bool)
        same[10 + self.seat] = False
        same[10 + 3 * self.cfg.players:] = False
        return np.array_equal(got[same], want[same])

    def moves_under(self, hand):
        """-> ((move in S_new, move in S_old), (my hand in S_new, my hand in S_old))."""
        if hand not in self._cache:
            pool = [self.deck[q] for q in self.my_pos + self.undealt]
            deck = list(self.deck)
            for q, c in zip(self.my_pos, hand):
                pool.remove(c)
                deck[q] = c
            for q, c in zip(self.undealt, pool):
                deck[q] = c
            env = _replay(self.cfg, deck, self.moves)
            got = env.export_state()[0]
            assert self._same_but_my_hand(got, self.old_row), "the replay did not end in S_old"
            m_old, h_old = int(env.rule_act(_rules(), 1, 1)[0][0]), hand_types(self.cfg, got, self.seat)
            env.step(np.asarray([self.a_old], np.int32))
            env.step(np.asarray([self.mine], np.int32))
            assert env.illegal_count() == 0
            got = env.export_state()[0]
            assert self._same_but_my_hand(got, self.new_row), "the replay did not end in S_new"
            self._cache[hand] = ((int(env.rule_act(_rules(), 1, 1)[0][0]), m_old), (hand_types(self.cfg, got, self.seat), h_old))
        return self._cache[hand]

    def posteriors(self):
        """(V0 prior, posterior given the last move, posterior given the last two) over the hands of the V0 support; a posterior
        is None where no hand is kept."""
        exact = enumerate_hands(self.cfg, self.row, self.seat)
        out = [{h: t for h, (t, _, _) in exact.items()}]
        for depth in (1, 2):
            want = (self.a_new, self.a_old)[:depth]
            out.append({h: (t if self.moves_under(h)[0][:depth] == want else 0) for h, (t, _, _) in exact.items()})
        return [None if not sum(p.values()) else {h: v / sum(p.values()) for h, v in p.items()} for p in out]


# (script of tests/test_search_cpu.SMALL_SCRIPTS, moves of it played before the partner's older rule-list move, my move between
# the partner's two, whether the older move tells more than the newer alone): found by a search over all prefixes and all my
# legal moves for scenes whose depth-2 posterior is a proper, non-empty part of the V0 support. In the first three it is also a
# proper part of the depth-1 posterior (my move: a discard; a play, after which the newer move alone tells nothing; a hint); in
# the last (a play) the older move adds nothing to what the newer tells.
SCENES2 = [(0, 11, 0, True), (1, 8, 3, True), (3, 18, 6, True), (3, 15, 3, False)]
R_EX, OVERSAMPLE_EX, CALLS_EX = 4, 4, 300


@pytest.mark.parametrize("script,n_moves,mine,proper", SCENES2)
def test_depth_2_survivors_are_the_exact_posterior_by_enumeration(script, n_moves, mine, proper):
    """The restated pipeline at depth 2 (determinize once, splice into both stored states with the tracked masks, the partner's
    move in each by the CPU rule oracle, select) against the exact posterior given both moves — uniform over the physical
    assignments in the V0 support under which the partner's rule list plays a_old in S_old and a_new in S_new — within 6 sigma
    of the binomial deviation per hand. Where the second move tells more than the first, the depth-1 survivors miss that bound."""
    deck, moves = SMALL_SCRIPTS[script]
    sc = Scene2(deck, moves[:n_moves], mine)
    assert sc.ok and (int(sc.row[0]) >> 13) & 7 == sc.seat
    prior, post1, post2 = sc.posteriors()
    true_hand = hand_types(sc.cfg, sc.row, sc.seat)
    assert post2 is not None and post2[true_hand] > 0 and sc.moves_under(true_hand)[0] == (sc.a_new, sc.a_old)
    keep1, keep2 = {h for h, v in post1.items() if v > 0}, {h for h, v in post2.items() if v > 0}
    assert keep2 <= keep1 and 0 < len(keep2) < len(prior), "the two moves tell the observer nothing about its hand"
    assert (keep2 < keep1) == bool(proper)
    K = R_EX * OVERSAMPLE_EX
    actual = np.array([[sc.a_new], [sc.a_old]])
    stored = [sc.new_row, sc.old_row]
    deep, shallow, n_deep, n_shallow = {}, {}, 0, 0
    for call in range(CALLS_EX):
        det, w = determinize_ref(sc.cfg, sc.row[None], sc.seat, K, 11, 3, first_row_id=call * K)
        hyp = np.empty((2, K, 1), np.int64)
        for d in range(2):
            hyp_rows = splice_alive_ref(stored[d][None], np.array([sc.alive[d]], np.uint8), det, sc.seat, K)
            for k in range(K):
                mv, hands = sc.moves_under(hand_types(sc.cfg, det[k], sc.seat))
                # what the spliced row shows the partner is the hand the candidate would have been at that time
                assert hand_types(sc.cfg, hyp_rows[k], sc.seat) == hands[d]
                hyp[d, k, 0] = mv[d]
        rows, ow, ns, du, fb = select_depth_ref(sc.row[None], det, w, hyp, actual, None, K, R_EX)
        if du[0] == 2:   # (a shallower depth is a fallback, not the depth-2 posterior)
            for j in range(R_EX):
                if ow[j]:
                    h = hand_types(sc.cfg, rows[j], sc.seat)
                    deep[h] = deep.get(h, 0) + 1
                    n_deep += 1
        rows1, ow1, _, fb1 = select_ref(sc.row[None], det, w, hyp[0], actual[0], None, K, R_EX)
        if fb1[0] == 0:
            for j in range(R_EX):
                if ow1[j]:
                    h = hand_types(sc.cfg, rows1[j], sc.seat)
                    shallow[h] = shallow.get(h, 0) + 1
                    n_shallow += 1
    assert n_deep > 500 and set(deep) <= keep2
    assert min(v for v in post2.values() if v > 0) * n_deep >= 20   # every kept hand is drawn often enough for the bound to bite
    assert not _violations(deep, n_deep, post2), _violations(deep, n_deep, post2)
    assert not _violations(shallow, n_shallow, post1)               # (depth 1 is the depth-1 posterior)
    if proper:
        assert _violations(shallow, n_shallow, post2), "the depth-1 survivors pass: the test cannot see the second predicate"


# ---- declarations and argument validation ---------------------------------------------------------------------------------------------
def test_new_names_are_exported_and_declared():
    import os

    import hanabi_hip
    from hanabi_hip import _capi

    for name in ("PartnerHistory", "belief_splice_alive", "belief_select_depth"):
        assert hasattr(hanabi_hip, name) and name in hanabi_hip.__all__
    assert "hb_belief_splice_alive" in _capi.SIGNATURES and "hb_belief_select_depth" in _capi.SIGNATURES
    L = hanabi_hip.lib()
    assert L.hb_belief_splice_alive and L.hb_belief_select_depth
    assert L.hb_abi_version() == 1
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "hanabi_hip.h")).read()
    assert "int hb_belief_splice_alive(const hb_config* cfg" in header and "int hb_belief_select_depth(const hb_config* cfg" in header
    assert "depth_used" in hanabi_hip.SearchPlayer.COUNTERS and hanabi_hip.SearchPlayer.COUNTERS[-1] == "depth_used"


def test_argument_validation_needs_no_gpu():
    import hanabi_hip

    L = hanabi_hip.lib()
    cfg = hanabi_hip.make_config()
    ref, one = C.byref(cfg), C.c_void_p(16)
    err = lambda: L.hb_last_error()
    bad_cfg = hanabi_hip.HbConfig(6, 5, 5, 5, 8, 3, 0)
    assert L.hb_belief_splice_alive(None, one, one, one, 4, 0, 8, one, None) < 0 and b"null" in err()
    for bad in (0, 2, 3):   # (alive may be NULL)
        p = [one] * 4
        p[bad] = None
        assert L.hb_belief_splice_alive(ref, p[0], p[1], p[2], 4, 0, 8, p[3], None) < 0 and b"null" in err()
    assert L.hb_belief_splice_alive(ref, one, one, one, 4, -1, 8, one, None) < 0 and b"seat" in err()
    assert L.hb_belief_splice_alive(ref, one, one, one, 4, 2, 8, one, None) < 0 and b"seat" in err()
    assert L.hb_belief_splice_alive(ref, one, one, one, 4, 0, 0, one, None) < 0 and b"n_cand" in err()
    assert L.hb_belief_splice_alive(ref, one, one, one, -1, 0, 8, one, None) < 0
    assert L.hb_belief_splice_alive(ref, one, one, one, 1 << 20, 0, 64, one, None) < 0 and b"2^31" in err()
    assert L.hb_belief_splice_alive(ref, one, one, one, 0, 0, 8, one, None) == 0
    assert L.hb_belief_splice_alive(ref, one, None, one, 0, 0, 8, one, None) == 0
    assert L.hb_belief_splice_alive(C.byref(bad_cfg), one, one, one, 4, 0, 8, one, None) < 0 and b"players" in err()

    def select(ptrs, m=4, k=8, r=3, d=2, cfg_ref=ref):
        p = list(ptrs)
        return L.hb_belief_select_depth(cfg_ref, p[0], p[1], p[2], p[3], p[4], p[5], m, k, r, d, p[6], p[7], p[8], p[9], p[10], None)

    assert select([one] * 11, cfg_ref=None) < 0 and b"null" in err()
    for bad in range(11):
        if bad == 5:   # valid may be NULL
            continue
        p = [one] * 11
        p[bad] = None
        assert select(p) < 0 and b"null" in err()
    assert select([one] * 11, r=0) < 0 and b"replicas" in err()
    assert select([one] * 11, k=2, r=3) < 0 and b"n_cand" in err()
    assert select([one] * 11, d=0) < 0 and b"depth" in err()
    assert select([one] * 11, d=9) < 0 and b"depth" in err()
    assert select([one] * 11, m=-1) < 0
    assert select([one] * 11, m=1 << 20, k=64, r=3) < 0 and b"2^31" in err()
    assert select([one] * 11, m=0) == 0 and select([one] * 11, m=0, d=8) == 0
    assert select([one] * 5 + [None] + [one] * 5, m=0) == 0
    assert select([one] * 11, cfg_ref=C.byref(bad_cfg)) < 0 and b"players" in err()


class _Agent:
    def eval_moves(self, *a, **k):
        raise AssertionError("not called")


def test_python_arguments_are_checked():
    import torch

    import hanabi_hip
    from hanabi_hip import PartnerHistory, SearchPlayer

    cfg = hanabi_hip.make_config()
    for depth in (0, 9):
        with pytest.raises(ValueError, match="depth"):
            PartnerHistory(cfg, 4, depth, "cpu")
        with pytest.raises(ValueError, match="depth"):
            SearchPlayer([_Agent(), _Agent()], 0, condition=True, depth=depth)
    with pytest.raises(ValueError, match="condition=True"):
        SearchPlayer([_Agent(), _Agent()], 0, depth=2)
    sp = SearchPlayer([_Agent(), _Agent()], 1, condition=True, depth=3)
    assert sp.depth == 3 and sp.depth_used == 0 and SearchPlayer([_Agent(), _Agent()], 0).depth == 1
    assert sp.depth_stats() == dict(reached=[0, 0, 0], survivors=[0, 0, 0], used=[0, 0, 0], shallow=[0, 0, 0])
    with pytest.raises(ValueError, match="m must be"):
        PartnerHistory(cfg, 0, 2, "cpu")
    h = PartnerHistory(cfg, 4, 2, "cpu", partner_seed=7, first_game_id=100)
    assert h.prev_rows.shape == (2, 4, 32) and h.moves.shape == h.alive.shape == h.valid.shape == (2, 4)
    assert (h.partner_seed, h.first_game_id, h.filled, h.draws) == (7, 100, 0, [0, 0]) and not h.valid.any()
    rows = torch.zeros((4, 32), dtype=torch.int32)
    with pytest.raises(ValueError, match="previous rows"):
        h.push(rows[:3], [0] * 4, 1, [1] * 4)
    with pytest.raises(ValueError, match="moves and valid"):
        h.push(rows, [0] * 3, 1, [1] * 4)
    with pytest.raises(ValueError, match="seat"):
        h.push(rows, [0] * 4, 1, [1] * 4, seat=2)
    with pytest.raises(ValueError, match="uids"):
        h.own_move([0] * 3)
    h.push(rows, [3, 4, 5, 6], 5, [1, 0, 1, 1])
    h.push(rows, [7, 8, 9, 10], 7, [1, 1, 1, 1])
    h.push(rows, [1, 1, 1, 1], 9, [0, 1, 1, 1])   # the oldest entry is dropped
    assert h.moves.tolist() == [[1, 1, 1, 1], [7, 8, 9, 10]] and h.valid.tolist() == [[0, 1, 1, 1], [1, 1, 1, 1]]
    assert h.draws == [9, 7] and h.filled == 2
    h.clear()
    assert not h.valid.any() and h.filled == 0 and h.draws == [0, 0]
