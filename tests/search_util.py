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
