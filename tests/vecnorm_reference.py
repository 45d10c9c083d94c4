"""fp64 numpy twin of Stable-Baselines3's VecNormalize in training mode, as include/upkie_hip.h states it (what
upkie_amd.normalize.RunningNormalizer computes on the device). Batch moments are numpy's two-pass mean / var of the
float32 data promoted to fp64."""

import numpy as np


class RunningMeanStd:
    """SB3's RunningMeanStd(epsilon=1e-4), fp64 (``count`` may start at 0 for tests of the merge alone)."""

    def __init__(self, shape=(), epsilon: float = 1e-4):
        self.mean = np.zeros(shape, np.float64)
        self.var = np.ones(shape, np.float64)
        self.count = float(epsilon)

    def update(self, x) -> None:
        x = np.asarray(x, dtype=np.float64)
        self.update_from_moments(x.mean(axis=0), x.var(axis=0), x.shape[0])

    def update_from_moments(self, batch_mean, batch_var, batch_count) -> None:
        delta = batch_mean - self.mean
        tot = self.count + batch_count
        new_mean = self.mean + delta * batch_count / tot
        m2 = self.var * self.count + batch_var * batch_count + np.square(delta) * self.count * batch_count / tot
        self.mean, self.var, self.count = new_mean, m2 / tot, tot


class VecNormalizeTwin:
    def __init__(self, num_envs, obs_dim, gamma=0.99, epsilon=1e-8, clip_obs=10.0, clip_reward=10.0, norm_obs=True, norm_reward=True,
                 training=True):
        self.obs_rms = RunningMeanStd((obs_dim,))
        self.ret_rms = RunningMeanStd(())
        self.returns = np.zeros(num_envs, np.float64)
        self.gamma, self.epsilon, self.clip_obs, self.clip_reward = gamma, epsilon, clip_obs, clip_reward
        self.norm_obs, self.norm_reward, self.training = norm_obs, norm_reward, training

    def mirrors(self):
        """(mean, std) rounded to fp32, as the device's mirrors."""
        return self.obs_rms.mean.astype(np.float32), np.sqrt(self.obs_rms.var + self.epsilon).astype(np.float32)

    def normalize_obs(self, obs):
        """In fp32 with the fp32 mirrors (the device's and the MLP policy's expression)."""
        obs = np.asarray(obs, np.float32)
        if not self.norm_obs:
            return obs.copy()
        m, s = self.mirrors()
        c = np.float32(self.clip_obs)
        return np.clip((obs - m) / s, -c, c).astype(np.float32)

    def normalize_obs64(self, obs):
        """SB3's own expression, in fp64."""
        return np.clip((np.asarray(obs, np.float64) - self.obs_rms.mean) / np.sqrt(self.obs_rms.var + self.epsilon), -self.clip_obs, self.clip_obs)

    def normalize_reward(self, reward):
        """In fp64, rounded once to fp32."""
        r = np.asarray(reward, np.float32).astype(np.float64)
        if self.norm_reward:
            r = np.clip(r / np.sqrt(self.ret_rms.var + self.epsilon), -self.clip_reward, self.clip_reward)
        return r.astype(np.float32)

    def reset(self, obs) -> None:
        self.returns[:] = 0.0
        if self.training and self.norm_obs:
            self.obs_rms.update(np.asarray(obs, np.float32))

    def step(self, obs, reward, terminated, truncated):
        """(normalised obs (fp32), normalised reward (fp32), episode starts)."""
        obs = np.asarray(obs, np.float32)
        reward = np.asarray(reward, np.float32)
        dones = np.asarray(terminated, bool) | np.asarray(truncated, bool)
        if self.training and self.norm_obs:
            self.obs_rms.update(obs)
        if self.training:
            self.returns = self.returns * self.gamma + reward.astype(np.float64)
            self.ret_rms.update(self.returns)
        r = self.normalize_reward(reward)
        self.returns[dones] = 0.0
        return self.normalize_obs(obs), r, dones.astype(np.uint8)
