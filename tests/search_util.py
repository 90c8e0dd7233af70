"""Helpers shared by the GPU tests of hanabi_hip.search (tests/test_search_gpu.py, test_search_confirm_gpu.py,
test_search_belief_gpu.py): roots a few moves into a game, the blueprint teams, and tensors as unsigned numpy words."""
import numpy as np


def _u32(t):
    return t.cpu().numpy().view(np.uint32) if t.dtype.itemsize == 4 else t.cpu().numpy()


def _mid_game_env(game, players, n, turns, seed=3):
    """A non-resetting env after `turns` random legal moves per game (hints included; some games may have ended)."""
    import hanabi_hip

    env = hanabi_hip.HanabiEnv(game, players, n_games=n, seed=seed, auto_reset=False, packed=True)
    for t in range(turns):
        env.step(env.random_legal_actions(seed=seed + 1, draw=t))
    return env


def _dqn(env_like, dtype="bfloat16", seed=1):
    from hanabi_agents.rlax_dqn import ActionSpec, DQNAgent, ObservationSpec, RlaxRainbowParams

    params = RlaxRainbowParams(train_batch_size=128, experience_buffer_size=8192, compute_dtype=dtype, packed_obs=True, layers=[512],
                               seed=seed)
    return DQNAgent(ObservationSpec((1, env_like.obs_len)), ActionSpec(env_like.num_actions), params, device="cuda")


def _team(name, env_like):
    from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR

    if name == "piers_piers":
        return [RulebasedAgent(PR.piers_rules, seed=11), RulebasedAgent(PR.piers_rules, seed=12)]
    if name == "iggi_flawed":
        return [RulebasedAgent(PR.iggi_rules, seed=13), RulebasedAgent(PR.flawed_rules, seed=14)]
    return [_dqn(env_like, seed=5), RulebasedAgent(PR.piers_rules, seed=15)]


def _conditioned_games():
    """The two recorded runs of tests/golden/search_belief_lastmove.json (written by tests/golden/gen_search_belief_golden.py,
    replayed by test_search_belief_gpu.py): Full, 2 players, 16 games of [Piers, Piers] with SearchPlayer(condition=True) in
    (a) seat 0, (b) both seats with a confirming stage. Everything is Philox draws and integer sums -> plain ints."""
    from hanabi_agents.rule_based import RulebasedAgent, predefined_rules as PR
    from hanabi_hip import Evaluator, SearchPlayer

    team = [RulebasedAgent(PR.piers_rules, seed=30), RulebasedAgent(PR.piers_rules, seed=31)]
    ev = Evaluator("Hanabi-Full", 2, n_games=16, seed=7, record_actions=True)
    kw = dict(replicas=3, seed=2, z=1.0, condition=True, oversample=4)
    one = SearchPlayer(team, 0, **kw)
    both = [SearchPlayer(team, s, confirm_replicas=4, **kw) for s in (0, 1)]
    out = {}
    for name, agents, players in (("seat0", [one, team[1]], [one]), ("both", both, both)):
        res = ev.run(agents)
        out[name] = dict(scores=res.scores.tolist(), lengths=res.lengths.tolist(), actions=res.actions.tolist(), players=[
            {k: int(getattr(p, k)) for k in SearchPlayer.COUNTERS + ("rollouts", "dead_replicas", "replicas_drawn", "searches")}
            for p in players])
    return out
