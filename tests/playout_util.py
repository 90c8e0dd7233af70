"""The expectation of hb_rule_playout that passes through no GPU code (tests/test_playout_cpu.py, tests/test_playout_gpu.py).

`oracle_playout` plays rule-list teams to the end on the CPU oracle: `OracleEnv.rule_act(rules, seed, t + 1)` and
`OracleEnv.step` per turn, with hb_eval_tally's bookkeeping (include/hanabi_hip.h) restated in numpy. Deals are those of the
oracle env of `seed` (the HIP env deals the same: deck(g) = Philox(seed, game id, episode 1))."""
import functools

import numpy as np

from oracle import oracle_py as O

DEAL_SEED = 7


def rules_of(rule_list):
    return [(r.kind, r.arg, r.threshold) for r in rule_list]


def teams():
    """name -> function(P) -> one rule list per seat (Ruleset rules)."""
    from hanabi_agents.rule_based import Ruleset, predefined_rules as PR

    everything = [Ruleset.hail_mary, Ruleset.play_if_certain, Ruleset.play_safe_card, Ruleset.play_probably_safe_factory(0.8, True),
                  Ruleset.discard_probably_useless_factory(0.9), Ruleset.tell_anyone_useless_card, Ruleset.tell_dispensable_factory(5),
                  Ruleset.tell_playable_card, Ruleset.tell_most_information, Ruleset.tell_unknown, Ruleset.osawa_discard,
                  Ruleset.discard_randomly]   # tests/test_rule_agents.py's list: the probability rules
    mixed = [PR.piers_rules, PR.iggi_rules, PR.outer_rules, PR.flawed_rules, PR.piers_rules]
    return dict(piers=lambda P: [PR.piers_rules] * P, flawed=lambda P: [PR.flawed_rules] * P, mixed=lambda P: mixed[:P],
                everything=lambda P: [everything] * P)


def oracle_playout(game, players, team_rules, seed, n, max_turns=None, first_moves=None, deal_seed=DEAL_SEED, first_game_id=0):
    """Play `n` games of `game` / `players` dealt by the oracle env of `deal_seed`, seat p following team_rules[p] (a list of
    (kind, arg, threshold)), agents' Philox seed `seed`, for max_turns turns (default: the bound no game exceeds).
    Returns a dict: rows0 / rows [n, SW] uint32 before / after, done [n] uint8, final_score [n] int8, length [n] int16, counters
    [2 + B + 5 P] int64 (hb_eval_tally's layout), actions [max_turns, n] int32 (-1 from a game's end on), illegal, max_len,
    status [n] (row status: 0 running, 1 out of lives, 2 perfect, 3 out of cards)."""
    cfg = O.make_config(game, players, 0)
    env = O.OracleEnv(cfg, n, seed=deal_seed, first_game_id=first_game_id)
    P, C_, R, H, A = players, cfg.colors, cfg.ranks, cfg.hand_size, env.num_actions
    draws = env.deck_size - P * H
    bound = draws + (cfg.max_info + draws + C_) + P
    T = bound if max_turns is None else int(max_turns)
    assert 1 <= T <= bound
    B = C_ * R + 1
    rows0 = env.export_state()
    done = np.zeros(n, np.uint8)
    final_score = np.zeros(n, np.int8)
    length = np.zeros(n, np.int16)
    counters = np.zeros(2 + B + 5 * P, np.int64)
    counters[0] = n
    actions = np.full((T, n), -1, np.int32)
    illegal0 = env.illegal_count()
    for t in range(T):
        live = (done & 0x80) == 0
        if not live.any():
            break
        seat = t % P
        if t == 0 and first_moves is not None:
            act = np.asarray(first_moves, np.int32)
        else:
            act, _ = env.rule_act(team_rules[seat], seed, t + 1)
        out = env.step(act)
        # hb_eval_tally(seat, t), games still live only
        ok = live & (act >= 0) & (act < A)
        kind = np.where(act < H, 0, np.where(act < 2 * H, 1, np.where(act < 2 * H + (P - 1) * C_, 2, 3)))
        for k in range(4):
            counters[2 + B + 4 * seat + k] += int((ok & (kind == k)).sum())
        misplay = ok & (kind == 1) & (out["reward"] <= 0)
        counters[2 + B + 4 * P + seat] += int(misplay.sum())
        lost = (done & 0x7F).astype(np.int64) + misplay
        ended = live & (out["terminal"] != 0)
        sc = out["score"].astype(np.int64)
        np.add.at(counters, 1 + np.clip(sc[ended], 0, B - 1), 1)
        counters[1 + B] += int((ended & (lost >= cfg.max_life)).sum())
        counters[0] -= int(ended.sum())
        final_score[ended] = sc[ended]
        length[ended] = t + 1
        done = np.where(ended, 0x80 | lost, np.where(live & misplay, lost, done)).astype(np.uint8)
        actions[t, live] = act[live]
    rows = env.export_state()
    return dict(rows0=rows0, rows=rows, done=done, final_score=final_score, length=length, counters=counters, actions=actions,
                illegal=env.illegal_count() - illegal0, max_len=int(length.max()), status=((rows[:, 0] >> 19) & 3).astype(np.int64),
                bins=B, players=P)


@functools.lru_cache(maxsize=None)
def expected(game, players, n, team, seed=DEAL_SEED, max_turns=None, first_game_id=0):
    """oracle_playout of a named team (teams()), computed once per case and shared; treat the arrays as read-only."""
    return oracle_playout(game, players, [rules_of(r) for r in teams()[team](players)], seed, n, max_turns=max_turns,
                          first_game_id=first_game_id)
