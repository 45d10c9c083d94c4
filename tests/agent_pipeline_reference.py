"""Host twins of the agent pipeline (csrc/agent_pipeline.hpp; include/upkie_hip.h states the arithmetic), for
tests/test_agent_pipeline*.py:

* `Twin` -- one env at a time, plain numpy: fp64 for the arithmetic, float32 for what is stored (the state, the
  command, the stack, and the settings dt and alpha, which the library rounds to float32 once); the noise from
  tests/mlp_reference.py's Philox helpers with the pipeline's tag;
* `BatchTwin` -- the same for a whole batch at once: vectorised Philox words, the transcendental part of a draw through the
  same scalar `math` calls as `philox_normal`, so that it is `Twin`'s bit for bit (tests/test_agent_pipeline_matrix.py holds
  it there on every row of tests/agent_pipeline_shapes.py); it can also be wrong on purpose (`mutation`), which is how the
  matrix shows that a test would notice;
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


# ---------------------------------------------------------------- the whole batch at once
_M0, _M1, _W0, _W1, _MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF


def philox_words(env, call, block, seed, tag=STREAM_PIPELINE):
    """Philox4x32-10 of counter (env[n], call[n], 0, tag << 24 | block) under `seed`: [N, 4] words (uint64 holding 32 bits)."""
    env, call = np.asarray(env, dtype=np.uint64) & np.uint64(_MASK), np.asarray(call, dtype=np.uint64) & np.uint64(_MASK)
    c = [env.copy(), call.copy(), np.zeros_like(env), np.full_like(env, (tag << 24) | int(block))]
    k0, k1 = seed & _MASK, (seed >> 32) & _MASK
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(_MASK), (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(_MASK)]
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return np.stack(c, axis=-1)


def philox_normals(env, call, count, block0, seed, one_block=False):
    """[N, count] draws: column i is element i & 3 of block block0 + (i >> 2) (of block0 itself with `one_block`), each
    `philox_normal`'s value bit for bit."""
    env = np.asarray(env)
    z = np.zeros((len(env), count))
    for b in range((count + 3) // 4):
        r = philox_words(env, call, block0 + (0 if one_block else b), seed)
        for i in range(4 * b, min(4 * b + 4, count)):
            p, odd = (i & 3) >> 1, i & 1
            u1 = ((r[:, 2 * p] >> np.uint64(8)) + np.uint64(1)).astype(F32) * F32(1.0 / 16777216.0)
            u2 = (r[:, 2 * p + 1] >> np.uint64(8)).astype(F32) * F32(1.0 / 16777216.0)
            angle = (MR.TWO_PI_F32 * u2).astype(F32)
            z[:, i] = [math.sqrt(-2.0 * math.log(float(a))) * (math.sin(float(t)) if odd else math.cos(float(t))) for a, t in zip(u1, angle)]
    return z


MUTATIONS = ("last_observation_column", "last_action", "swapped_terminal_draws", "action_block_zero", "restart_keeps_old_frames",
             "prev_command_zeroed_once")


class BatchTwin:
    """`Twin` for envs ``envs`` (default 0..N-1) at once. State: ``prev_command``, ``command`` [N, A], ``stack``, ``final``
    [N, K, F] float32 (`final` rows of envs that did not end keep what they held, zero at first), ``calls`` [N] (uint32 values
    in int64). ``mutation`` (one of `MUTATIONS`) makes it wrong the way a kernel could be."""

    def __init__(self, num_envs, obs_dim, low, high, dt, stack=8, action_in_observation=True, integrate_action=False, action_noise=None,
                 action_lag=None, observation_noise=None, seed=0, envs=None, mutation=None):
        assert mutation is None or mutation in MUTATIONS
        self.N, self.D, self.K, self.seed, self.mutation = int(num_envs), int(obs_dim), int(stack), int(seed), mutation
        self.envs = np.arange(self.N, dtype=np.int64) if envs is None else np.asarray(envs, dtype=np.int64)
        self.low, self.high = np.asarray(low, dtype=F32).astype(np.float64), np.asarray(high, dtype=F32).astype(np.float64)
        self.A = len(self.low)
        self.in_obs, self.integrate = bool(action_in_observation), bool(integrate_action)
        self.F = self.D + (self.A if self.in_obs else 0)
        self.dt = float(F32(dt))
        self.alpha = None if action_lag is None else float(F32(float(dt) / float(action_lag)))
        widen = lambda s, n: None if s is None else np.broadcast_to(np.asarray(s, dtype=F32), (n,)).astype(np.float64)  # noqa: E731
        self.sigma_a, self.sigma_o = widen(action_noise, self.A), widen(observation_noise, self.D)
        self.prev_command = np.zeros((self.N, self.A), dtype=F32)
        self.command = np.zeros((self.N, self.A), dtype=F32)
        self.stack = np.zeros((self.N, self.K, self.F), dtype=F32)
        self.final = np.zeros((self.N, self.K, self.F), dtype=F32)
        self.calls = np.zeros(self.N, dtype=np.int64)

    def shape_action_exact(self, action, prev=None, calls=None):
        """(the fp64 value of every command word [N, A], the draws [N, A] or None) from `prev` and `calls` (default: the state)."""
        a = np.asarray(action, dtype=F32).astype(np.float64)
        p = (self.prev_command if prev is None else np.asarray(prev, dtype=F32)).astype(np.float64)
        u = np.clip(p + a * self.dt, self.low, self.high) if self.integrate else a.copy()
        z = None
        if self.sigma_a is not None:
            z = philox_normals(self.envs, self.calls if calls is None else calls, self.A, 0, self.seed, one_block=self.mutation == "action_block_zero")
            u = np.clip(u + self.sigma_a * z, self.low, self.high)
        return (u if self.alpha is None else p + self.alpha * (u - p)), z

    def shape_action(self, action):
        a = np.asarray(action, dtype=F32)
        exact, _ = self.shape_action_exact(a)
        with np.errstate(over="ignore", invalid="ignore"):
            c = exact.astype(F32)
        if self.mutation == "last_action":
            c[:, -1] = 0
        poisoned = ~np.isfinite(a) | ~np.isfinite(c)
        self.command = np.where(poisoned, F32(0), c).astype(F32)
        self.prev_command = np.where(poisoned, self.prev_command, c).astype(F32)
        if self.sigma_a is not None:
            self.calls = (self.calls + 1) & _MASK
        return self.command

    def frame_exact(self, obs, calls, terminal=False):
        """(the fp64 value of the D observation columns of a frame [N, D], the draws or None)."""
        x = np.asarray(obs, dtype=F32).astype(np.float64)
        z = None
        if self.sigma_o is not None:
            if self.mutation == "swapped_terminal_draws":
                terminal = not terminal
            z = philox_normals(self.envs, calls, self.D, FINAL_BLOCK if terminal else 0, self.seed)
            x = x + self.sigma_o * z
        if self.mutation == "last_observation_column":
            x[:, -1] = 0
        return x, z

    def _frame(self, obs, command, calls, terminal=False):
        x = self.frame_exact(obs, calls, terminal)[0].astype(F32)
        return np.concatenate([x, np.asarray(command, dtype=F32)], axis=1) if self.in_obs else x

    def observe(self, next_obs, done, final_obs=None):
        done = np.asarray(done, dtype=bool)
        calls = self.calls
        new = self._frame(next_obs, np.where(done[:, None], F32(0), self.command), calls)
        moved = np.concatenate([self.stack[:, 1:], new[:, None]], axis=1)
        if final_obs is not None and done.any():
            last = self._frame(final_obs, self.command, calls, terminal=True)
            self.final[done] = np.concatenate([self.stack[:, 1:], last[:, None]], axis=1)[done]
        if self.mutation != "restart_keeps_old_frames":
            moved[done, : self.K - 1] = 0
        self.stack = moved
        # (the kernel's lane of word w zeroes the words w, w + S, ... of prev_command: "once" stops after the first)
        self.prev_command[done, : self.K * self.F if self.mutation == "prev_command_zeroed_once" else self.A] = 0
        if self.sigma_o is not None:
            self.calls = (self.calls + 1) & _MASK
        return self.stack.reshape(self.N, -1)

    def reset(self, obs, mask=None):
        mask = np.ones(self.N, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
        new = self._frame(obs, np.zeros((self.N, self.A), dtype=F32), self.calls)
        self.stack[mask] = 0
        self.stack[mask, self.K - 1] = new[mask]
        self.prev_command[mask] = 0
        if self.sigma_o is not None:
            self.calls = np.where(mask, (self.calls + 1) & _MASK, self.calls)
        return self.stack.reshape(self.N, -1)
