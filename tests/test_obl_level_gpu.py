"""Off-belief learning levels 2+ on the GPU (hanabi_hip.obl, PartnerHistory.advance, hb_belief_history_step): the kernel against
`advance` on CPU copies bit for bit, the session's partner histories through re-deals against histories rebuilt on the CPU with
the torch methods, one level-2 step against sample_history called by hand, what conditioning means, the counters, the real game
against SelfPlaySession's, the unchanged default, a short level-2 training run and the refusals."""
import numpy as np
import pytest

from search_util import _mid_game_env

pytestmark = pytest.mark.gpu

CAP = 256
BELIEF_SEED = 5


# ---- the kernel ----------------------------------------------------------------------------------------------------------------------
def _guarded(shape, dtype, guard, fill):
    """(buffer, view): a contiguous tensor of `shape` with `guard` sentinel elements before and after it."""
    import torch

    n = int(np.prod(shape))
    buf = torch.full((n + 2 * guard,), fill, dtype=dtype, device="cuda")
    return buf, buf[guard:guard + n].view(shape)


@pytest.mark.parametrize("game,players,m", [(g, p, m) for g, p in (("Hanabi-Full", 2), ("Hanabi-Small", 2), ("Hanabi-Full", 3))
                                            for m in (1, 63, 64, 65, 200)] + [("Hanabi-Full", 5, 65)])
def test_history_step_equals_advance_on_the_cpu(game, players, m):
    """12 calls per depth on the rows of a real game (random legal moves, no re-deal: games finish on the way), each part present
    or absent by a seeded pattern that covers all eight combinations; all four tensors compared after every call. The history
    starts from random bytes (alive bits 5-7 and the bits of empty slots among them). Two layouts per depth: every tensor 4
    sentinel elements into its buffer (rows 16-byte aligned: the 16-byte items) and 3 (the word-by-word form)."""
    import torch

    from hanabi_hip import PartnerHistory

    calls = 12
    env = _mid_game_env(game, players, m, 2 if game == "Hanabi-Small" else 6, seed=5 + m)
    cfg, SW, H = env.cfg, env.state_words, env.cfg.hand_size
    assert SW == (48 if players == 5 else 32) and H == (2 if game == "Hanabi-Small" else 4 if players == 5 else 5)
    rng = np.random.default_rng(1000 * players + m)
    # the inputs of every call, from the game: (seat, own or None, reset or None, cur or None, prev or None, draw)
    exports, inputs = [env.export_state()], []
    pattern = list(rng.permutation(8)) + list(rng.integers(0, 8, calls - 8))
    for k in range(calls):
        own = env.random_legal_actions(seed=77, draw=k).cpu()   # plays, discards and hints of the right range
        own[torch.as_tensor(rng.random(m) < 0.1)] = -1
        own[torch.as_tensor(rng.random(m) < 0.1)] = env.num_actions + 3
        env.step(env.random_legal_actions(seed=78, draw=k))
        exports.append(env.export_state())
        reset = torch.as_tensor((rng.random(m) < 0.25) * rng.integers(1, 256, m)).to(torch.uint8)
        bits = int(pattern[k])
        inputs.append((int(rng.integers(players)), own if bits & 1 else None, reset if bits & 2 else None,
                       exports[-1].cpu() if bits & 4 else None, exports[-2].cpu() if bits & 4 else None, 2 * k + 1))
    assert sorted(set(int(b) for b in pattern)) == list(range(8))
    finished = (((exports[-1][:, 0] >> 19) & 3) != 0).sum().item()
    print(game, players, m, "finished games at the end:", finished)
    for depth in (1, 2, 8):
        start = dict(prev_rows=torch.as_tensor(rng.integers(-2 ** 31, 2 ** 31, (depth, m, SW)).astype(np.int32)),
                     moves=torch.as_tensor(rng.integers(-1, env.num_actions, (depth, m)).astype(np.int32)),
                     alive=torch.as_tensor(rng.integers(0, 256, (depth, m)).astype(np.uint8)),
                     valid=torch.as_tensor(rng.integers(0, 2, (depth, m)).astype(np.uint8)))
        ref = PartnerHistory(cfg, m, depth, "cpu")
        for name, t in start.items():
            getattr(ref, name).copy_(t)
        want = []
        for seat, own, reset, cur, prev, draw in inputs:
            ref.advance(own_moves=own, reset=reset, cur_rows=cur, prev_rows=prev, seat=seat, draw=draw)
            want.append({name: getattr(ref, name).clone() for name in start} | dict(draws=list(ref.draws), filled=ref.filled))
        for guard in (4, 3):
            h = PartnerHistory(cfg, m, depth, "cuda")
            bufs = {}
            for name, t in start.items():
                fill = 0x5A if t.dtype == torch.uint8 else 0x5A5A5A5A
                bufs[name], view = _guarded(t.shape, t.dtype, guard, fill)
                view.copy_(t)
                setattr(h, name, view)
            assert (h.prev_rows.data_ptr() % 16 == 0) == (guard == 4)
            cuda = lambda x: None if x is None else x.cuda()
            for k, (seat, own, reset, cur, prev, draw) in enumerate(inputs):
                h.advance(own_moves=cuda(own), reset=cuda(reset), cur_rows=cuda(cur), prev_rows=cuda(prev), seat=seat, draw=draw)
                for name in start:
                    assert torch.equal(getattr(h, name).cpu(), want[k][name]), (name, depth, guard, k)
                assert (h.draws, h.filled) == (want[k]["draws"], want[k]["filled"])
            for name, buf in bufs.items():   # the sentinels on both sides
                fill = 0x5A if buf.dtype == torch.uint8 else 0x5A5A5A5A
                assert bool((buf[:guard] == fill).all()) and bool((buf[-guard:] == fill).all()), (name, depth, guard)


# ---- the session's histories ---------------------------------------------------------------------------------------------------------
def _params(**kw):
    from hanabi_agents.rlax_dqn import RlaxRainbowParams

    base = dict(train_batch_size=64, experience_buffer_size=CAP, compute_dtype="bfloat16", packed_obs=True, layers=[512],
                mask_terminal=True)
    base.update(kw)
    return RlaxRainbowParams(**base)


def _dqn(env, seed, **kw):
    from hanabi_agents.rlax_dqn import ActionSpec, DQNAgent, ObservationSpec

    return DQNAgent(ObservationSpec((env.n, env.obs_len)), ActionSpec(env.num_actions), _params(seed=seed, **kw), device="cuda")


def _piers(seed):
    from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR

    return RulebasedAgent(PR.piers_rules, seed=seed)


def _valid_rule(cur, prev, seat):
    """The issue's rule for a pushed entry, in numpy on uint32 rows: cur running, a last move recorded in word 2, its mover not
    the observer, prev running with that mover to act."""
    run = lambda r: ((r[:, 0] >> 19) & 3) == 0
    mover = (cur[:, 2] >> 1) & 7
    return (run(cur) & ((cur[:, 2] & 1) != 0) & (mover != seat) & run(prev) & (((prev[:, 0] >> 13) & 7) == mover)).astype(np.uint8)


class _Shadow:
    """Both observers' histories of a 2-player session, rebuilt on the CPU with PartnerHistory's torch methods from what the test
    records around every step (the export before it, the moves and the terminal flags after it): independent of advance()."""

    def __init__(self, cfg, n, depth):
        from hanabi_hip import PartnerHistory

        self.cfg, self.hist = cfg, [PartnerHistory(cfg, n, depth, "cpu") for _ in range(2)]
        self.rows, self.moves, self.term = [], [], []

    def before_step(self, t, rows):
        """The turn of seat t % 2's history at step t; rows = the export of step t."""
        import torch

        from hanabi_hip import last_move_uid

        self.rows.append(rows.cpu())
        if t == 0:
            return
        h, seat = self.hist[t % 2], t % 2
        if t >= 2:
            h.own_move(self.moves[t - 2])
        gone = self.term[t - 1] != 0
        if t >= 2:
            gone = gone | (self.term[t - 2] != 0)
        h.valid[:, gone] = 0
        h.alive[:, gone] = 0
        cur, prev = self.rows[t], self.rows[t - 1]
        valid = _valid_rule(cur.numpy().view(np.uint32), prev.numpy().view(np.uint32), seat)
        h.push(prev, last_move_uid(self.cfg, cur), t - 1, torch.as_tensor(valid), seat=seat)

    def after_step(self, moves, term):
        self.moves.append(moves.cpu().clone())
        self.term.append(term.cpu().clone())


def _same_history(h, ref):
    import torch

    for name in ("prev_rows", "moves", "alive", "valid"):
        if not torch.equal(getattr(h, name).cpu(), getattr(ref, name)):
            return False
    return (h.draws, h.filled) == (ref.draws, ref.filled)


def _deck_layout(cfg, deck_size):
    """(first deck word, words the deck bytes take)."""
    return 10 + 3 * cfg.players, (deck_size + 3) // 4


def test_histories_through_redeals_one_step_by_hand_and_what_conditioning_means():
    """Small, 2 players, 200 games, depth 3, oversample 4, belief policy [Piers, Piers], 120 steps without training; the live
    agents move uniformly at random (epsilon = 1), so that games of every length end on both seats' moves.
    * Every step: both observers' histories equal the CPU rebuild (_Shadow).
    * Steps 40 .. 47: the session's fictitious rows and weights equal ConditionedDeterminizer.sample_history called directly with
      the rebuilt history (moved to the GPU) and the issue's arguments, and the scratch env imported exactly those rows.
    * The same steps: for every row with fallback 0 and depth_used = D, the chosen fictitious hand spliced into the state of each
      of the partner's last D moves makes the belief policy play the move the partner really made; and the fictitious row
      differs from the real one in the observer's hand word and the undealt deck bytes only.
    * The counters add up to the rows branched."""
    import torch

    import hanabi_hip
    from hanabi_hip import ConditionedDeterminizer, OffBeliefSession, PartnerHistory, belief_splice_alive

    n, depth, ov, steps = 200, 3, 4, 120
    env = hanabi_hip.HanabiEnv("Hanabi-Small", 2, n_games=n, seed=21, first_game_id=1000, packed=True)
    cfg = env.cfg
    agents = [_dqn(env, seed=s, epsilon=1.0) for s in (1, 2)]
    belief = [_piers(41), _piers(42)]
    sess = OffBeliefSession(env, agents, belief_seed=BELIEF_SEED, belief_policy=belief, depth=depth, oversample=ov)
    assert sorted(sess.histories) == [0, 1]
    shadow = _Shadow(cfg, n, depth)
    imported = []
    orig_import = sess.scratch.import_state

    def spy(rows):
        orig_import(rows)
        imported.append(sess.scratch.export_state())

    sess.scratch.import_state = spy
    by_hand = ConditionedDeterminizer(config=cfg)
    probe = hanabi_hip.HanabiEnv(config=cfg, n_games=n, first_game_id=env.first_game_id, packed=True)
    hyp = torch.empty(n, dtype=torch.int32, device="cuda")
    D_cards = env.deck_size
    w_deck, n_deck = _deck_layout(cfg, D_cards)
    seen = dict(own_end=[False, False], partner_end=[False, False], full=[False, False], cut=[False, False], none=[False, False])
    checked_rows, forwards = 0, 0
    for t in range(steps):
        seat = t % 2
        rows = env.export_state()
        shadow.before_step(t, rows)
        ref = shadow.hist[seat]
        want = None
        if 40 <= t < 48:
            on_gpu = PartnerHistory(cfg, n, depth, "cuda")
            for name in ("prev_rows", "moves", "alive", "valid"):
                getattr(on_gpu, name).copy_(getattr(ref, name))
            on_gpu.draws, on_gpu.filled = list(ref.draws), ref.filled
            want = by_hand.sample_history(rows, on_gpu, belief[1 - seat], seat, 1, ov, seed=BELIEF_SEED, draw=t, partner_seed=BELIEF_SEED,
                                          first_game_id=env.first_game_id, first_row_id=env.first_game_id)
        forwards += min(depth, ref.filled) * ov
        sess.step(train=False)
        shadow.after_step(sess.last_actions[seat], env.terminal)
        assert _same_history(sess.histories[seat], ref), t
        # what the run contains, observer by observer
        term = shadow.term[t].numpy() != 0
        seen["own_end"][seat] |= bool(term.any())
        seen["partner_end"][1 - seat] |= bool(term.any())
        valid = ref.valid.numpy()
        if ref.filled == depth:
            seen["full"][seat] |= bool(valid.all(0).any())
            seen["cut"][seat] |= bool(((valid[0] == 1) & (valid[depth - 1] == 0)).any())
            seen["none"][seat] |= bool((valid[0] == 0).any())
        assert (np.diff(valid.astype(np.int8), axis=0) <= 0).all()   # (2 players, auto-reset: a chain is a prefix of the stack)
        if want is None:
            continue
        # ---- one step by hand
        w_rows, w_w, w_surv, w_used, w_fb = want.rows, want.weights, want.n_surv, want.depth_used, want.fallback
        assert torch.equal(sess._det_rows, w_rows) and torch.equal(sess._det_w.long() & 0xFFFFFFFF, w_w)
        n_surv, used, fb = sess.last_belief
        assert torch.equal(n_surv, w_surv) and torch.equal(used, w_used) and torch.equal(fb, w_fb)
        assert torch.equal(imported[-1], sess._det_rows)
        # ---- what conditioning means
        h = sess.histories[seat]
        fict = sess._det_rows
        used_c, fb_c = used.cpu().numpy(), fb.cpu().numpy()
        for d in range(depth):
            pick = torch.as_tensor((fb_c == 0) & (used_c > d)).cuda()
            if not bool(pick.any()):
                continue
            spliced = belief_splice_alive(cfg, h.prev_rows[d].contiguous(), h.alive[d].contiguous(), fict, seat, 1)[0]
            # (rows that are not checked must still be states the policy can run on: the real current row is one)
            probe.import_state(torch.where(pick.view(n, 1), spliced, rows))
            belief[1 - seat].eval_moves(probe, BELIEF_SEED, h.draws[d], hyp)
            assert torch.equal(hyp[pick], h.moves[d][pick]), (t, d)
            checked_rows += int(pick.sum())
        assert (used_c[fb_c == 0] >= 1).all() and (used_c[fb_c != 0] == 0).all()
        real, fic = rows.cpu().numpy().view(np.uint32), fict.cpu().numpy().view(np.uint32)
        other = [j for j in range(env.state_words) if j != 10 + seat and not w_deck <= j < w_deck + n_deck]
        assert np.array_equal(real[:, other], fic[:, other])
        dealt = D_cards - (real[:, 0] & 63).astype(np.int64)     # deck bytes below this position are public
        rb = real[:, w_deck:w_deck + n_deck].copy().view(np.uint8).reshape(n, -1)[:, :D_cards]
        fb_bytes = fic[:, w_deck:w_deck + n_deck].copy().view(np.uint8).reshape(n, -1)[:, :D_cards]
        public = np.arange(D_cards)[None, :] < dealt[:, None]
        assert np.array_equal(rb[public], fb_bytes[public])
        assert (real[:, 10 + seat] != fic[:, 10 + seat]).any()
    sess.flush()
    torch.cuda.synchronize()
    print("run contains", seen, "rows checked for conditioning", checked_rows)
    for what in ("own_end", "partner_end", "full", "cut", "none"):
        assert all(seen[what]), what
    assert checked_rows > 0
    # ---- the counters
    branched = n * steps   # every step is a branch step, every game of an auto-reset env is running
    c = {k: getattr(sess, k) for k in OffBeliefSession.LEVEL_COUNTERS}
    print(c, "belief_forwards", sess.belief_forwards)
    assert c["conditioned_rows"] + c["fallback_rows"] + c["unconditioned_rows"] == branched == sess.branch_steps // 2
    assert c["conditioned_rows"] > 0 and c["unconditioned_rows"] > 0
    assert c["conditioned_rows"] <= c["survivors"] <= ov * c["conditioned_rows"]
    assert c["conditioned_rows"] <= c["depth_used_sum"] <= depth * c["conditioned_rows"]
    assert sess.belief_forwards == forwards == sum(min(depth, (t + t % 2) // 2) * ov for t in range(steps))
    assert env.illegal_count() == 0 and sess.scratch.illegal_count() == 0 and sess.dead_rows == 0


# ---- the real game, and the default ------------------------------------------------------------------------------------------------------
def test_the_real_game_is_selfplay_s_with_a_belief_policy():
    import torch

    import hanabi_hip
    from hanabi_hip import OffBeliefSession
    from hanabi_hip.selfplay import SelfPlaySession

    def run(make):
        torch.manual_seed(0)
        env = hanabi_hip.HanabiEnv("Hanabi-Full", 2, n_games=256, seed=7, packed=True)
        agents = [_dqn(env, seed=s, experience_buffer_size=8192) for s in (1, 2)]
        sess = make(env, agents)
        acts = []
        for _ in range(40):
            sess.step(train=False)
            acts.append(sess.last_actions[(sess.t - 1) % 2].clone())
        sess.flush()
        torch.cuda.synchronize()
        return torch.stack(acts), env.export_state(), [a._draws for a in agents], sess

    a_obl, rows_obl, draws_obl, obl = run(lambda e, a: OffBeliefSession(e, a, belief_policy=[_piers(1), _piers(2)], depth=2, oversample=3))
    a_sp, rows_sp, draws_sp, sp = run(SelfPlaySession)
    assert torch.equal(a_obl, a_sp) and torch.equal(rows_obl, rows_sp)
    assert draws_obl == draws_sp == [20, 20]
    assert obl.env_steps == sp.env_steps == 40 * 256 and obl.branch_steps == 40 * 256 * 2
    assert obl.episodes == sp.episodes and obl.grad_steps == sp.grad_steps == 0
    assert obl.belief_forwards == sum(min(2, (t + t % 2) // 2) * 3 for t in range(40))
    assert obl.conditioned_rows + obl.fallback_rows + obl.unconditioned_rows == 40 * 256


def test_no_belief_policy_is_level_1_unchanged():
    import torch

    import hanabi_hip
    from hanabi_hip import OffBeliefSession

    def run(**kw):
        env = hanabi_hip.HanabiEnv("Hanabi-Small", 2, n_games=128, seed=3, packed=True)
        agents = [_dqn(env, seed=s, experience_buffer_size=1024) for s in (1, 2)]
        sess = OffBeliefSession(env, agents, **kw)
        for _ in range(10):
            sess.step(train=False)
        sess.flush()
        torch.cuda.synchronize()
        return sess, [[t.clone() for t in (b._obs_tm1_buf, b._obs_t_buf, b._act_tm1_buf, b._lms_t_buf, b._rew_t_buf, b._terminal_t_buf)]
                      for b in (a.experience for a in agents)]

    plain, rings = run()
    explicit, rings2 = run(belief_policy=None, depth=1, oversample=4)
    for a, b in zip(rings, rings2):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    assert plain.agents[0].experience.size == 128 * 5
    for s in (plain, explicit):
        assert s.belief_policy is None and s.belief_forwards == 0
        assert (s.conditioned_rows, s.fallback_rows, s.unconditioned_rows, s.survivors, s.depth_used_sum) == (0, 0, 0, 0, 0)


# ---- training ----------------------------------------------------------------------------------------------------------------------------
def test_training_smoke_at_level_2_and_frozen_copy():
    import torch

    import hanabi_hip
    from hanabi_hip import OffBeliefSession
    from hanabi_hip.obl import frozen_copy

    n, steps = 256, 150
    env = hanabi_hip.HanabiEnv("Hanabi-Small", 2, n_games=n, seed=11, packed=True)
    agents = [_dqn(env, seed=s, experience_buffer_size=32768, use_priority=True) for s in (1, 2)]
    frozen = [frozen_copy(a) for a in agents]
    batch = (env, (env.net_obs.clone(), env.legal.clone()))
    greedy = lambda a: a.eval_moves(batch, 3, 0, torch.empty(n, dtype=torch.int32, device="cuda")).clone()
    for a, f in zip(agents, frozen):
        assert f is not a and f.params.seed == a.params.seed and f.experience.capacity <= 64
        assert torch.equal(greedy(a), greedy(f))
        for (k, x), (_, y) in zip(a.online.state_dict().items(), f.online.state_dict().items()):
            assert torch.equal(x, y) and x.data_ptr() != y.data_ptr(), k
    before = [greedy(f) for f in frozen]
    w0 = [torch.cat([p.detach().reshape(-1) for p in a.online.parameters()]).clone() for a in agents]
    sess = OffBeliefSession(env, agents, belief_policy=frozen, depth=2)
    sess.run(steps)
    torch.cuda.synchronize()
    assert sess.grad_steps > 0 and sess.env_steps == n * steps and sess.branch_steps == n * steps * 2 and sess.dead_rows == 0
    assert env.illegal_count() == 0 and sess.scratch.illegal_count() == 0
    assert sess.conditioned_rows > 0 and sess.belief_forwards > 0
    assert sess.conditioned_rows + sess.fallback_rows + sess.unconditioned_rows == n * steps
    for a, f, start, moves in zip(agents, frozen, w0, before):
        w = torch.cat([p.detach().reshape(-1) for p in a.online.parameters()])
        assert torch.isfinite(w).all() and not torch.equal(w, start)
        # the copy stayed where it was: its weights are the original's first ones, its moves the same
        assert torch.equal(torch.cat([p.detach().reshape(-1) for p in f.online.parameters()]), start)
        assert torch.equal(greedy(f), moves) and f.experience.size == 0 and f._draws == 0
        buf = a.experience
        assert buf.size == n * (steps // 2)
        assert torch.isfinite(buf._rew_t_buf[:buf.size]).all()
        ended = buf._terminal_t_buf[:buf.size, 0]
        assert ended.any() and not ended.all()
        assert not buf._obs_t_buf[:buf.size][ended].any() and not buf._lms_t_buf[:buf.size][ended].any()
        assert buf._lms_t_buf[:buf.size][~ended].any(1).all()
        # every row of the ring has a leaf, and the root is their sum: fp32 pairwise sums over log2(capacity) = 15 levels, each
        # within 2^-24 relative of the exact sum of positive terms
        nodes = buf.sum_tree.nodes().double()
        leaves = nodes[buf.capacity:]
        assert torch.isfinite(leaves).all() and (leaves[:buf.size] > 0).all() and not leaves[buf.size:].any()
        total = float(buf.sum_tree.total_dev().item())
        assert abs(total - float(leaves.sum())) <= 15 * 2.0 ** -24 * float(leaves.sum())
    assert np.isfinite(sess.mean_score()) and sess.episodes > 0


def test_a_loaded_checkpoint_clears_the_histories():
    import torch

    import hanabi_hip
    from hanabi_hip import OffBeliefSession

    env = hanabi_hip.HanabiEnv("Hanabi-Small", 2, n_games=64, seed=2, packed=True)
    sess = OffBeliefSession(env, [_dqn(env, seed=1), _dqn(env, seed=2)], belief_policy=[_piers(1), _piers(2)], depth=2)
    for _ in range(6):
        sess.step(train=False)
    sd = sess.checkpoint_state(include_replay=False)
    assert all(h.filled == 2 and bool(h.valid.any()) for h in sess.histories.values())
    sess.load_checkpoint_state(sd)
    assert all(h.filled == 0 and not bool(h.valid.any()) and not bool(h.alive.any()) for h in sess.histories.values())
    before = sess.unconditioned_rows
    sess.step(train=False)   # the first step after a load has nothing to condition on
    torch.cuda.synchronize()
    assert sess.unconditioned_rows - before == 64 and all(h.filled == 0 for h in sess.histories.values())
    sess.step(train=False)
    assert sess.histories[1].filled == 1


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    import hanabi_hip
    from hanabi_hip import OffBeliefSession

    env = hanabi_hip.HanabiEnv("Hanabi-Small", 2, n_games=128, seed=1, packed=True)
    good, other, piers = _dqn(env, seed=1), _dqn(env, seed=2), _piers(1)
    frozen = [_piers(2), _piers(3)]
    for kw in (dict(depth=2), dict(oversample=8), dict(depth=0)):
        with pytest.raises(ValueError, match="belong to a belief policy"):
            OffBeliefSession(env, [good, other], **kw)
    env3 = hanabi_hip.HanabiEnv("Hanabi-Small", 3, n_games=128, seed=1, packed=True)
    with pytest.raises(ValueError, match="2 players"):
        OffBeliefSession(env3, [_dqn(env3, seed=s) for s in (1, 2, 3)], belief_policy=[_piers(1), _piers(2), _piers(3)])
    for bad in ([frozen[0]], frozen + [_piers(4)], []):
        with pytest.raises(ValueError, match="one entry per seat"):
            OffBeliefSession(env, [good, other], belief_policy=bad)
    with pytest.raises(ValueError, match=r"belief_policy\[1\] is None"):
        OffBeliefSession(env, [good, other], belief_policy=[frozen[0], None])
    with pytest.raises(ValueError, match=r"belief_policy\[0\] is None"):
        OffBeliefSession(env, [good, other], belief_policy=[None, frozen[1]])
    with pytest.raises(TypeError, match="eval_moves"):
        OffBeliefSession(env, [good, other], belief_policy=[frozen[0], object()])
    with pytest.raises(ValueError, match="own agents"):
        OffBeliefSession(env, [good, other], belief_policy=[good, frozen[1]])
    with pytest.raises(ValueError, match="own agents"):
        OffBeliefSession(env, [good, piers], train_seats=[0], belief_policy=[None, piers])
    for depth in (0, 9):
        with pytest.raises(ValueError, match="depth"):
            OffBeliefSession(env, [good, other], belief_policy=frozen, depth=depth)
    with pytest.raises(ValueError, match="oversample"):
        OffBeliefSession(env, [good, other], belief_policy=frozen, oversample=0)
    # a seat nobody conditions on needs no entry: seat 0 alone is trained, on the belief over seat 1's moves
    sess = OffBeliefSession(env, [good, piers], train_seats=[0], belief_policy=[None, frozen[1]], depth=8, oversample=1)
    assert sorted(sess.histories) == [0] and sess.depth == 8 and sess.oversample == 1
