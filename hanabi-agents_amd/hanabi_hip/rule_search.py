"""Evolutionary search over rule lists, scored on the GPU: a tool on top of `CrossPlay(playout=True)`.

The reference's rule-based agents are priority lists of `Ruleset` rules that somebody searched for. `RuleSearch` is that kind of
search: a population of rule lists, every list scored as a self-play team (the list in every seat) on the SAME deals — one
`CrossPlay(playout=True)` run, which is one hb_rule_playout_grouped launch per chunk of teams —, the best `elite` kept and the
population refilled with their mutants.

    rs = RuleSearch("Hanabi-Small", players=2, n_games=1024, seed=3, population=64, elite=8)
    out = rs.run([predefined_rules.piers_rules], generations=10, rng_seed=0)
    out.best, out.mean, out.history            # the best list, its mean score on the search's deals, the best mean per generation
    rs.validate([out.best], n_games=4096, seed=99)   # on fresh deals: the search overfits its own

A mutation replaces one rule by a rule of the catalogue, swaps two neighbours, inserts a catalogue rule or deletes a rule; a list
keeps between 1 and MAX_RULES rules. Everything random comes from one `numpy.random.Generator(PCG64(rng_seed))`: the same
`rng_seed`, initial lists and scores give the same run. The elite are carried over unchanged and the deals are fixed, so the best
mean of a generation never falls below the one before. Nothing here says how well a found list plays: the means are means over the
search's own deals, `validate` gives the figure on others.
"""
from typing import List, NamedTuple

import numpy as np

from . import _capi as K

MUTATIONS = ("replace", "swap", "insert", "delete")
THRESHOLDS = (0.4, 0.6, 0.8)   # the factory rules' fixed thresholds in the default catalogue
MIN_INFO = (2, 5, 8)           # tell_dispensable_factory's


def default_catalogue():
    """The `Ruleset` rules a mutation draws from: every plain rule, and the factory rules at a few fixed thresholds."""
    from hanabi_agents.rule_based import Ruleset as R

    plain = [R.legal_random, R.discard_oldest_first, R.osawa_discard, R.tell_unknown, R.tell_randomly, R.play_safe_card,
             R.play_if_certain, R.tell_playable_card_outer, R.tell_anyone_useless_card, R.tell_most_information, R.tell_playable_card,
             R.discard_randomly, R.hail_mary]
    made = [R.tell_dispensable_factory(m) for m in MIN_INFO]
    made += [R.play_probably_safe_factory(t, lives) for t in THRESHOLDS for lives in (False, True)]
    made += [R.discard_probably_useless_factory(t) for t in THRESHOLDS]
    return plain + made


class RuleSearchResult(NamedTuple):
    """best: the best rule list of the last generation, mean: its score, history: the best score of every generation (the initial
    population first: generations + 1 entries)."""
    best: list
    mean: float
    history: List[float]


class RuleSearch:
    """game / players / n_games / seed: the deals every list is scored on (CrossPlay's). population: lists per generation, elite:
    how many of the best survive unchanged (1 .. population). catalogue: the rules a mutation draws from (default:
    default_catalogue()). score: a function lists -> one mean per list, instead of the GPU self-play score (for tests and other
    objectives)."""

    def __init__(self, game="Hanabi-Full", players=2, n_games=1024, seed=1, population=64, elite=8, catalogue=None, score=None):
        self.game, self.players, self.n_games, self.seed = game, int(players), int(n_games), int(seed)
        self.population, self.elite = int(population), int(elite)
        if not 1 <= self.elite <= self.population:
            raise ValueError(f"need 1 <= elite <= population, got elite {elite}, population {population}")
        self.catalogue = list(default_catalogue() if catalogue is None else catalogue)
        if not self.catalogue:
            raise ValueError("an empty catalogue")
        self._score = score
        self._crossplays = {}     # (n_games, seed) -> CrossPlay(playout=True)
        self.mutation_counts = dict.fromkeys(MUTATIONS, 0)   # of the last run

    # ---- scoring --------------------------------------------------------------------------------------------------------------
    def selfplay_means(self, lists, n_games, seed):
        """Mean score of every list as a self-play team (the list in every seat) on the `n_games` deals of `seed`: one
        CrossPlay(playout=True) run over len(lists) teams."""
        from hanabi_agents.rule_based import RulebasedAgent

        from .crossplay import CrossPlay

        key = (int(n_games), int(seed))
        cp = self._crossplays.get(key)
        if cp is None:
            cp = self._crossplays[key] = CrossPlay(self.game, self.players, n_games=n_games, seed=seed, playout=True)
        pool = [RulebasedAgent(rules) for rules in lists]
        res = cp.run(pool, teams=[(i,) * self.players for i in range(len(pool))])
        if cp.last_path != "playout":
            raise RuntimeError("rule lists took the turn loop: the playout kernel is missing from this run")
        return [r.mean for r in res.results]

    def score(self, lists):
        lists = [list(x) for x in lists]
        if self._score is not None:
            means = [float(m) for m in self._score(lists)]
            if len(means) != len(lists):
                raise ValueError(f"score returned {len(means)} means for {len(lists)} lists")
            return means
        return self.selfplay_means(lists, self.n_games, self.seed)

    def validate(self, lists, n_games, seed):
        """The self-play means of `lists` on other deals than the search's (which it overfits): `n_games` deals of `seed`."""
        return self.selfplay_means([list(x) for x in lists], n_games, seed)

    # ---- mutation -------------------------------------------------------------------------------------------------------------
    def mutate(self, rules, rng):
        """(mutant, mutation name) of one rule list: a mutation type that the list's length allows, drawn uniformly."""
        rules = list(rules)
        n = len(rules)
        allowed = ["replace"] + (["swap"] if n >= 2 else []) + (["insert"] if n < K.MAX_RULES else []) + (["delete"] if n >= 2 else [])
        kind = allowed[int(rng.integers(len(allowed)))]
        new = self.catalogue[int(rng.integers(len(self.catalogue)))]
        if kind == "replace":
            rules[int(rng.integers(n))] = new
        elif kind == "swap":
            i = int(rng.integers(n - 1))
            rules[i], rules[i + 1] = rules[i + 1], rules[i]
        elif kind == "insert":
            rules.insert(int(rng.integers(n + 1)), new)
        else:
            del rules[int(rng.integers(n))]
        return rules, kind

    # ---- the search -----------------------------------------------------------------------------------------------------------
    def run(self, initial_lists, generations, rng_seed=0):
        """From `initial_lists` (at least one list of 1 .. MAX_RULES rules; more than `population` are cut, fewer are filled with
        mutants), `generations` times: score, keep the `elite` best (ties: the earlier list), refill with mutants of elite
        members drawn uniformly. Returns a RuleSearchResult."""
        rng = np.random.Generator(np.random.PCG64(int(rng_seed)))
        self.mutation_counts = dict.fromkeys(MUTATIONS, 0)
        pop = [list(x) for x in initial_lists][:self.population]
        if not pop:
            raise ValueError("no initial list")
        for rules in pop:
            if not 1 <= len(rules) <= K.MAX_RULES:
                raise ValueError(f"a list has 1..{K.MAX_RULES} rules, got {len(rules)}")
        self._fill(pop, len(pop), rng)
        history = []
        for g in range(int(generations) + 1):
            means = self.score(pop)
            order = sorted(range(len(pop)), key=lambda i: (-means[i], i))
            pop, means = [pop[i] for i in order], [means[i] for i in order]
            history.append(means[0])
            if g == int(generations):
                break
            pop = pop[:self.elite]
            self._fill(pop, len(pop), rng)
        return RuleSearchResult(pop[0], means[0], history)

    def _fill(self, pop, parents, rng):
        """Append mutants of pop[:parents] until the population is full."""
        while len(pop) < self.population:
            child, kind = self.mutate(pop[int(rng.integers(parents))], rng)
            self.mutation_counts[kind] += 1
            pop.append(child)
