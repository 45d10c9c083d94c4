"""Twins of the time-limit bootstrap and of the episode statistics (upkie_amd.policies.MlpActorCritic.
bootstrap_time_limits, upkie_amd.episodes.EpisodeStatistics): Stable-Baselines3's Monitor + ``deque(maxlen=window)``
+ ``safe_mean`` in fp64 Python, and the bootstrap formula in float32 numpy. SB3 is not imported."""

from collections import deque

import numpy as np


class MonitorTwin:
    """SB3's Monitor for each of N envs and the ``ep_info_buffer`` deque. ``rewards[i]`` holds the env's raw rewards
    as Python floats, summed with ``sum`` when the episode ends (Monitor.step); ``round(r, 6)`` and ``"t"`` are left
    out, as on the device."""

    def __init__(self, num_envs: int, window: int = 100):
        self.num_envs, self.window = int(num_envs), int(window)
        self.rewards = [[] for _ in range(self.num_envs)]
        self.ep_info_buffer = deque(maxlen=self.window)
        self.total_episodes = 0

    def step(self, reward, terminated=None, truncated=None) -> None:
        reward = np.asarray(reward, dtype=np.float32)
        done = np.zeros(self.num_envs, dtype=bool)
        if terminated is not None:
            done |= np.asarray(terminated, dtype=bool)
        if truncated is not None:
            done |= np.asarray(truncated, dtype=bool)
        for i in range(self.num_envs):  # (in env order: what VecMonitor / collect_rollouts push into the deque)
            self.rewards[i].append(float(reward[i]))
            if done[i]:
                self.ep_info_buffer.append({"r": sum(self.rewards[i]), "l": len(self.rewards[i])})
                self.rewards[i] = []
                self.total_episodes += 1

    def reset(self, mask=None) -> None:
        for i in range(self.num_envs):
            if mask is None or bool(mask[i]):
                self.rewards[i] = []

    def running(self):
        """(returns, lengths) of the running episodes."""
        return np.array([sum(r) for r in self.rewards], dtype=np.float64), np.array([len(r) for r in self.rewards], dtype=np.int64)

    def means(self):
        """(mean return, mean length) as the device computes them: the return sum sequential from the oldest entry, the
        length sum exact; (0, 0) while the ring is empty."""
        if not self.ep_info_buffer:
            return 0.0, 0.0
        n = len(self.ep_info_buffer)
        total = 0.0
        for e in self.ep_info_buffer:
            total += e["r"]
        return total / n, sum(e["l"] for e in self.ep_info_buffer) / n

    def safe_mean(self, key):
        """SB3's ``safe_mean([ep_info[key] for ep_info in ep_info_buffer])``: np.mean (pairwise sums), nan when empty."""
        values = [e[key] for e in self.ep_info_buffer]
        return np.nan if len(values) == 0 else float(np.mean(values))


def bootstrap(reward, value, terminated, truncated, gamma):
    """``rewards[idx] += gamma * terminal_value`` of SB3's collect_rollouts in float32: two roundings, the envs with
    truncated and not terminated only. ``value``: V(final_obs) per env (float32)."""
    reward = np.array(reward, dtype=np.float32, copy=True)
    value = np.asarray(value, dtype=np.float32)
    mask = np.asarray(truncated, dtype=bool) & ~np.asarray(terminated, dtype=bool)
    g = np.float32(gamma)
    reward[mask] = reward[mask] + (g * value[mask]).astype(np.float32)
    return reward
