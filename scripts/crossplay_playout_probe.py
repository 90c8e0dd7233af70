"""What CrossPlay(playout=True) (every chunk of rule-list teams played to the end by one hb_rule_playout_grouped launch) is worth
on one MI355X. A pool of 8 rule lists, the 64 default teams x 4 096 games, Hanabi-Full with 2 and with 5 players, three paths in
one process:
  (a) loop     CrossPlay().run(pool): the turn loop, three launches per turn over all 64 blocks;
  (b) single   a Python loop of 64 Evaluator(playout=True).run(team): one hb_rule_playout launch per team;
  (c) grouped  CrossPlay(playout=True).run(pool): one launch for the 64 teams.
A warm-up run of each, then the three alternated, best of 3 each, every run kept; events around whole run calls. Checks that the
three paths give the same 64 means. Then one RuleSearch generation as a time only: 256 lists x 1 024 games, Hanabi-Full 2p.
Usage: crossplay_playout_probe.py [out.json]   (default profiles/playout/crossplay_playout_probe.json)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hanabi-agents_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from hanabi_agents.rule_based import RulebasedAgent, Ruleset as R, predefined_rules as PR  # noqa: E402
from hanabi_hip import CrossPlay, Evaluator, RuleSearch  # noqa: E402
from hanabi_hip.crossplay import default_teams  # noqa: E402

REPS, N_GAMES, SEED = 3, 4096, 7


def pool_of_8():
    cautious = [R.play_safe_card, R.tell_playable_card_outer, R.osawa_discard, R.tell_unknown, R.discard_oldest_first]
    gambler = [R.play_if_certain, R.play_probably_safe_factory(0.6, True), R.tell_playable_card, R.discard_probably_useless_factory(0.5),
               R.tell_randomly, R.discard_randomly]
    everything = [R.hail_mary, R.play_if_certain, R.play_safe_card, R.play_probably_safe_factory(0.8, True),
                  R.discard_probably_useless_factory(0.9), R.tell_anyone_useless_card, R.tell_dispensable_factory(5), R.tell_playable_card,
                  R.tell_most_information, R.tell_unknown, R.osawa_discard, R.discard_randomly]
    lists = [PR.piers_rules, PR.iggi_rules, PR.outer_rules, PR.flawed_rules, cautious, gambler, everything, [R.legal_random]]
    return [RulebasedAgent(rules, seed=100 + i) for i, rules in enumerate(lists)]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def alternate(paths):
    """Warm every path, then alternate them: {name: (best ms, the REPS runs, the last result)}."""
    for fn in paths.values():
        fn()
    ms, res = {k: [] for k in paths}, {}
    for _ in range(REPS):
        for name, fn in paths.items():
            t, res[name] = timed(fn)
            ms[name].append(round(t, 3))
    return {k: (min(v), v, res[k]) for k, v in ms.items()}


def spread(runs):
    return max(runs) - min(runs)


def crossplay_case(players):
    pool = pool_of_8()
    teams = default_teams(len(pool), players)
    loop, grouped = CrossPlay("Hanabi-Full", players, n_games=N_GAMES, seed=SEED), CrossPlay("Hanabi-Full", players, n_games=N_GAMES,
                                                                                             seed=SEED, playout=True)
    single = Evaluator("Hanabi-Full", players, n_games=N_GAMES, seed=SEED, playout=True)
    out = alternate(dict(loop=lambda: [r.mean for r in loop.run(pool).results],
                         single=lambda: [single.run([pool[i] for i in t]).mean for t in teams],
                         grouped=lambda: [r.mean for r in grouped.run(pool).results]))
    assert loop.last_path == "loop" and grouped.last_path == "playout" and single.last_path == "playout"
    a, b, c = out["loop"], out["single"], out["grouped"]
    worst = max(spread(a[1]), spread(b[1]), spread(c[1]))
    return dict(players=players, pool=len(pool), teams=len(teams), n_games=N_GAMES, chunks=len(grouped.chunks(len(teams))),
                longest_game=max(grouped.last_turns), ms_best=dict(loop=a[0], single=b[0], grouped=c[0]),
                ms_runs=dict(loop=a[1], single=b[1], grouped=c[1]), spread_ms=round(worst, 3),
                loop_over_grouped=round(a[0] / c[0], 2), single_over_grouped=round(b[0] / c[0], 2),
                grouped_beats_loop_by_more_than_the_spread=bool(a[0] - c[0] > worst),
                grouped_no_slower_than_single_within_the_spread=bool(c[0] - b[0] <= worst),
                means_equal=bool(a[2] == b[2] == c[2]), mean_of_means=float(np.mean(c[2])))


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "playout", "crossplay_playout_probe.json")
    out = {}
    for players in (2, 5):
        out[f"crossplay_full_{players}p"] = crossplay_case(players)
        print(json.dumps(out[f"crossplay_full_{players}p"]), flush=True)
        torch.cuda.empty_cache()
    # one RuleSearch generation (a time only): 256 lists scored on 1 024 common deals
    rs = RuleSearch("Hanabi-Full", 2, n_games=1024, seed=SEED, population=256, elite=32)
    rng = np.random.Generator(np.random.PCG64(0))
    lists = [PR.piers_rules, PR.iggi_rules, PR.outer_rules, PR.flawed_rules]
    rs._fill(lists, 4, rng)
    rs.score(lists)
    runs = [round(timed(lambda: rs.score(lists))[0], 3) for _ in range(REPS)]
    out["rule_search_generation"] = dict(lists=len(lists), n_games=1024, game="Hanabi-Full 2p", ms_best=min(runs), ms_runs=runs)
    print(json.dumps(out["rule_search_generation"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
