"""Host twins of the agent pipeline (csrc/agent_pipeline.hpp; include/upkie_hip.h states the arithmetic), for
tests/test_agent_pipeline*.py:

* `Twin` -- one env at a time, plain numpy: fp64 for the arithmetic, float32 for what is stored (the state, the
  command, the stack, and the settings dt and alpha, which the library rounds to float32 once); the noise from
  tests/mlp_reference.py's Philox helpers with the pipeline's tag;
* `DequeStack` -- a second, independent statement of the frame stack as an actual ``collections.deque(maxlen=K)`` of
  frames per env (Stable-Baselines3's ``VecFrameStack`` on a flat observation), without noise: it checks the twin's
  index arithmetic.
"""

import collections
import math

import numpy as np

from oracle import oracle as O
from tests import mlp_reference as MR

STREAM_PIPELINE = 5
FINAL_BLOCK = 64
F32 = np.float32


def philox_normal(env: int, call: int, block: int, elem: int, seed: int, tag: int = STREAM_PIPELINE) -> float:
    """Element `elem` of the four normals of Philox block `block` of env `env` at call `call`: `MR.philox_normal`'s
    arithmetic (fp32 uniforms and angle as the kernel forms them, the rest fp64) under another tag."""
    r = O.philox([env & 0xFFFFFFFF, call & 0xFFFFFFFF, 0, (tag << 24) | block], [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF])
    p, i = elem >> 1, elem & 1
    u1 = F32((r[2 * p] >> 8) + 1) * F32(1.0 / 16777216.0)
    u2 = F32(r[2 * p + 1] >> 8) * F32(1.0 / 16777216.0)
    angle = float(F32(MR.TWO_PI_F32 * u2))
    radius = math.sqrt(-2.0 * math.log(float(u1)))
    return radius * (math.cos(angle) if i == 0 else math.sin(angle))


class Twin:
    """The pipeline of ONE env (index `env`: the key of its noise). State: ``prev_command`` [A] float32, ``stack``
    [K, F] float32 (oldest frame first), ``calls`` (int). `shape_action`, `observe` and `reset` are the library's."""

    def __init__(self, env, obs_dim, low, high, dt, stack=8, action_in_observation=True, integrate_action=False, action_noise=None,
                 action_lag=None, observation_noise=None, seed=0):
        self.env, self.D, self.K, self.seed = int(env), int(obs_dim), int(stack), int(seed)
        self.low, self.high = np.asarray(low, dtype=F32).astype(np.float64), np.asarray(high, dtype=F32).astype(np.float64)
        self.A = len(self.low)
        self.in_obs, self.integrate = bool(action_in_observation), bool(integrate_action)
        self.F = self.D + (self.A if self.in_obs else 0)
        self.dt = float(F32(dt))
        self.alpha = None if action_lag is None else float(F32(float(dt) / float(action_lag)))
        widen = lambda s, n: None if s is None else np.broadcast_to(np.asarray(s, dtype=F32), (n,)).astype(np.float64)  # noqa: E731
        self.sigma_a, self.sigma_o = widen(action_noise, self.A), widen(observation_noise, self.D)
        self.prev_command = np.zeros(self.A, dtype=F32)
        self.command = np.zeros(self.A, dtype=F32)
        self.stack = np.zeros((self.K, self.F), dtype=F32)
        self.final = None  # the last stacked terminal observation [K, F]
        self.calls = 0
        self.last_z = None  # the draws of the last shape_action [A] (None without noise)

    # ---- the exact (fp64) value of one shape_action from the stored state; float32 only at the end
    def shape_action_exact(self, action, prev=None, call=None):
        a = np.asarray(action, dtype=F32).astype(np.float64)
        p = (self.prev_command if prev is None else np.asarray(prev, dtype=F32)).astype(np.float64)
        u = a.copy()
        if self.integrate:
            u = np.clip(p + a * self.dt, self.low, self.high)
        z = None
        if self.sigma_a is not None:
            c = self.calls if call is None else int(call)
            z = np.array([philox_normal(self.env, c, k >> 2, k & 3, self.seed) for k in range(self.A)])
            u = np.clip(u + self.sigma_a * z, self.low, self.high)
        out = u if self.alpha is None else p + self.alpha * (u - p)
        return out, z

    def shape_action(self, action):
        a = np.asarray(action, dtype=F32)
        exact, z = self.shape_action_exact(a)
        self.last_z = z
        c = exact.astype(F32)
        poisoned = ~np.isfinite(a) | ~np.isfinite(c)
        self.command = np.where(poisoned, F32(0), c).astype(F32)
        self.prev_command = np.where(poisoned, self.prev_command, c).astype(F32)
        if self.sigma_a is not None:
            self.calls += 1
        return self.command

    def _frame(self, obs, command, call, block0):
        x = np.asarray(obs, dtype=F32).astype(np.float64)
        if self.sigma_o is not None:
            z = np.array([philox_normal(self.env, call, block0 + (d >> 2), d & 3, self.seed) for d in range(self.D)])
            x = x + self.sigma_o * z
        parts = [x.astype(F32)] + ([np.asarray(command, dtype=F32)] if self.in_obs else [])
        return np.concatenate(parts)

    def _restart(self, obs, call):
        self.stack[:] = 0
        self.stack[self.K - 1] = self._frame(obs, np.zeros(self.A, dtype=F32), call, 0)
        self.prev_command[:] = 0

    def observe(self, next_obs, done, final_obs=None):
        call = self.calls
        if not done:
            self.stack[: self.K - 1] = self.stack[1:].copy()
            self.stack[self.K - 1] = self._frame(next_obs, self.command, call, 0)
        else:
            if final_obs is not None:
                self.final = np.concatenate([self.stack[1:], self._frame(final_obs, self.command, call, FINAL_BLOCK)[None]], axis=0)
            self._restart(next_obs, call)
        if self.sigma_o is not None:
            self.calls += 1
        return self.stack.reshape(-1)

    def reset(self, obs):
        self._restart(obs, self.calls)
        if self.sigma_o is not None:
            self.calls += 1
        return self.stack.reshape(-1)


class DequeStack:
    """``VecFrameStack`` of one env as a deque of its last K frames (no noise): a restart fills it with zero frames and
    appends the first frame; a step appends; the terminal observation is the deque of the ended episode with the frame
    of the terminal observation appended."""

    def __init__(self, stack, frame_dim):
        self.K, self.F = int(stack), int(frame_dim)
        self.frames = collections.deque([np.zeros(self.F, dtype=F32) for _ in range(self.K)], maxlen=self.K)
        self.final = None

    def restart(self, frame):
        self.frames = collections.deque([np.zeros(self.F, dtype=F32) for _ in range(self.K)], maxlen=self.K)
        self.frames.append(np.asarray(frame, dtype=F32))

    def step(self, frame, done=False, final_frame=None, reset_frame=None):
        if not done:
            self.frames.append(np.asarray(frame, dtype=F32))
            return
        if final_frame is not None:
            ended = collections.deque(self.frames, maxlen=self.K)
            ended.append(np.asarray(final_frame, dtype=F32))
            self.final = np.concatenate(list(ended))
        self.restart(reset_frame)

    def flat(self):
        return np.concatenate(list(self.frames))


def run_batch(twins, actions, next_obs, done, final_obs=None):
    """One step of a list of twins on batch rows: returns (command [N, A], observation [N, K F])."""
    cmd = np.stack([tw.shape_action(actions[e]) for e, tw in enumerate(twins)])
    obs = np.stack([tw.observe(next_obs[e], bool(done[e]), None if final_obs is None else final_obs[e]).copy() for e, tw in enumerate(twins)])
    return cmd, obs
