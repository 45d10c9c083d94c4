"""What an agent wraps around the env before PPO sees it, on the device: the policy's output shaped into the command
the env receives (integrated, noised, passed through a first-order lag), and the observation the policy reads (noised,
the command appended, the last ``stack`` frames stacked as Stable-Baselines3's ``VecFrameStack``).

As torch ops the frame stack with its per-env restart and its stacked terminal observation is a roll, two masked writes
and a concatenation per step, the noise is two generator calls that are not keyed per env, and the whole chain is some
fifteen launches. `AgentPipeline` is two launches per rollout step (``upkie_pipeline_shape_action``,
``upkie_pipeline_observe``: csrc/agent_pipeline.hpp; include/upkie_hip.h states the arithmetic) with all of its state
on the device."""

import ctypes as C
import math
from typing import Optional, Sequence

import torch

from . import lib
from .exceptions import UpkieRuntimeError
from .launch import check, device_tensor, end_flags, launcher, ptr

# enum UpkiePipelineFlag
ACTION_IN_OBSERVATION, INTEGRATE_ACTION, ACTION_NOISE, ACTION_LAG, OBSERVATION_NOISE = 1, 2, 4, 8, 16
MAX_WORDS = 256  # the obs_dim cap of the MLP policy, which reads the stack


def _floats(values, n: int, what: str):
    if isinstance(values, torch.Tensor):
        values = values.detach().cpu().reshape(-1).tolist()
    elif not isinstance(values, (list, tuple)):
        try:
            values = list(values)
        except TypeError:
            values = [values]
    values = [float(v) for v in values]
    if len(values) == 1 and n > 1:
        values = values * n
    if len(values) != n:
        raise ValueError(f"{what} needs {n} values, got {len(values)}")
    return values


class AgentPipeline:
    """Action shaping, noise and frame stacking for ``num_envs`` envs with ``[num_envs, obs_dim]`` float32 observations
    and ``len(action_low)`` actions.

    ``shape_action(env_action)`` (between ``policy.act`` and ``env.step``) turns the policy's clamped output into
    `command`, each stage only if switched on: ``integrate_action``: ``u = clip(prev_command + a * dt, low, high)``;
    ``action_noise`` (per-action sigma): ``u = clip(u + sigma * z, low, high)``; ``action_lag`` (a time constant in
    seconds): ``c = prev_command + (dt / action_lag) * (u - prev_command)``, `upkie_amd.utils.filters.low_pass_filter`
    (``dt / action_lag >= 0.5`` is refused, as there). ``prev_command = c``. A non-finite word gives the neutral
    command 0 and is not stored.

    ``observe(next_obs, terminated, truncated, final_obs)`` (after ``env.step``) builds the frame ``next_obs +
    observation_noise * z`` followed by the command (``action_in_observation``) and pushes it into `observation`
    ``[num_envs, stack * F]``, oldest frame first. For an env that ended (same-step autoreset: ``next_obs`` is the
    reset observation) it does what ``VecFrameStack`` does: `final_observation` gets the old stack shifted, with the
    frame of ``final_obs`` (noised, followed by the command just applied) last; then the stack is zeroed, the frame of
    the reset observation with a zero command takes the last slot, and ``prev_command`` is zeroed. The
    `final_observation` rows of envs that did not end keep what they held: the time-limit bootstrap reads truncated
    rows only. ``final_obs=None``: the restart alone. ``reset(obs, mask)`` is that restart for the masked envs.

    Noise is Philox4x32-10 keyed (env, the env's call counter `calls`, a stream tag of its own, block) under ``seed``:
    the draws of env e at call c do not depend on the batch size and a saved counter resumes them. With every sigma
    None no random number is drawn and the counters do not move. In a sharded run build one pipeline per process with
    a seed per rank (the key is the local env index).

    All state (`prev_command`, `observation`, `calls`) and the outputs (`command`, `final_observation`) are allocated
    at construction; a call allocates nothing and has no host argument that changes between steps, so it can be
    captured in a hipGraph (`GraphedLoop`). Device only: there is no CPU fallback."""

    def __init__(self, num_envs: int, obs_dim: int, action_low: Sequence[float], action_high: Sequence[float], dt: float, stack: int = 8,
                 action_in_observation: bool = True, integrate_action: bool = False, action_noise=None, action_lag: Optional[float] = None,
                 observation_noise=None, seed: int = 0, device="cuda:0"):
        self.num_envs, self.obs_dim, self.stack = int(num_envs), int(obs_dim), int(stack)
        low = _floats(action_low, len(action_low) if hasattr(action_low, "__len__") else 1, "action_low")
        self.act_dim = len(low)
        high = _floats(action_high, self.act_dim, "action_high")
        self.action_in_observation, self.integrate_action = bool(action_in_observation), bool(integrate_action)
        self.frame_dim = self.obs_dim + (self.act_dim if self.action_in_observation else 0)
        self.stacked_dim = self.stack * self.frame_dim
        if self.num_envs < 1:
            raise ValueError("num_envs must be positive")
        if self.stack < 1:
            raise ValueError("stack must be at least 1")
        if not 1 <= self.act_dim <= 64:
            raise ValueError("act_dim must be in 1-64")
        if self.obs_dim < 1 or self.stacked_dim > MAX_WORDS:
            raise ValueError(f"obs_dim must be positive and stack * frame at most {MAX_WORDS} words (the policy's obs_dim cap), got "
                             f"{self.stack} x {self.frame_dim}")
        self.dt = float(dt)
        if not (self.dt > 0.0 and math.isfinite(self.dt)):
            raise ValueError("dt must be positive and finite")
        if any(not lo <= hi for lo, hi in zip(low, high)):
            raise ValueError("action bounds need low <= high")
        self.action_lag = None if action_lag is None else float(action_lag)
        if self.action_lag is not None and not (self.action_lag > 0.0 and self.dt / self.action_lag < 0.5):
            raise ValueError("action_lag: low_pass_filter needs dt / action_lag < 0.5 (Nyquist-Shannon sampling theorem)")
        sigma_a = None if action_noise is None else _floats(action_noise, self.act_dim, "action_noise")
        sigma_o = None if observation_noise is None else _floats(observation_noise, self.obs_dim, "observation_noise")
        for name, sig in (("action_noise", sigma_a), ("observation_noise", sigma_o)):
            if sig is not None and any(not (s >= 0.0 and math.isfinite(s)) for s in sig):
                raise ValueError(f"{name} sigmas must be non-negative and finite")
        self.action_low, self.action_high, self.action_noise, self.observation_noise = low, high, sigma_a, sigma_o
        self.flags = ((ACTION_IN_OBSERVATION if self.action_in_observation else 0) | (INTEGRATE_ACTION if self.integrate_action else 0)
                      | (ACTION_NOISE if sigma_a is not None else 0) | (ACTION_LAG if self.action_lag is not None else 0)
                      | (OBSERVATION_NOISE if sigma_o is not None else 0))
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise UpkieRuntimeError("AgentPipeline runs on the HIP device only (there is no CPU fallback): give device='cuda:0'")
        self._lib = lib.load()
        lib.require(self._lib, "upkie_pipeline_observe")
        self._launcher = launcher(self.device)
        self.params = torch.from_numpy(self.packed_params()).to(self.device)
        N, A, S = self.num_envs, self.act_dim, self.stacked_dim
        f32 = dict(dtype=torch.float32, device=self.device)
        self.prev_command = torch.zeros(N, A, **f32)
        self.command = torch.zeros(N, A, **f32)
        self.observation = torch.zeros(N, S, **f32)
        self.final_observation = torch.zeros(N, S, **f32)
        self.calls = torch.zeros(N, dtype=torch.int32, device=self.device)  # (uint32 words)

    def packed_params(self):
        """The ``params`` words of the library (low, high, action sigma, observation sigma), checked and packed by
        ``upkie_pipeline_params`` (host only)."""
        import numpy as np

        library = lib.load()
        arr = lambda v: None if v is None else (C.c_float * len(v))(*v)  # noqa: E731
        out = np.zeros(3 * self.act_dim + self.obs_dim, dtype=np.float32)
        words = int(library.upkie_pipeline_params(self.obs_dim, self.act_dim, arr(self.action_low), arr(self.action_high), arr(self.action_noise),
                                                  arr(self.observation_noise), out.ctypes.data))
        check(words)
        return out

    def _settings(self):
        return (self.num_envs, self.obs_dim, self.act_dim, self.stack, self.flags, self.dt, self.action_lag or 0.0, self.params.data_ptr(), self.seed)

    def shape_action(self, env_action: torch.Tensor) -> torch.Tensor:
        """``env_action`` [N, A] float32 (the policy's clamped output) into `command`, which is returned."""
        a = device_tensor(env_action, "env_action", self.device, (self.num_envs, self.act_dim))
        self._launcher(self._lib.upkie_pipeline_shape_action, *self._settings(), a.data_ptr(), self.prev_command.data_ptr(), self.calls.data_ptr(),
                       self.command.data_ptr())
        return self.command

    def observe(self, next_obs: torch.Tensor, terminated: Optional[torch.Tensor] = None, truncated: Optional[torch.Tensor] = None,
                final_obs: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One env step: ``next_obs`` [N, D] float32, ``terminated`` / ``truncated`` [N] bool or uint8 (None: none ended),
        ``final_obs`` [N, D] (None: no `final_observation`). Returns `observation`."""
        N, D, dev = self.num_envs, self.obs_dim, self.device
        obs = device_tensor(next_obs, "next_obs", dev, (N, D))
        term, trunc = end_flags(terminated, truncated, dev, N)
        final = device_tensor(final_obs, "final_obs", dev, (N, D), required=False)
        self._launcher(self._lib.upkie_pipeline_observe, *self._settings(), obs.data_ptr(), ptr(term), ptr(trunc), ptr(final),
                       self.command.data_ptr(), self.prev_command.data_ptr(), self.calls.data_ptr(), self.observation.data_ptr(),
                       self.final_observation.data_ptr())
        return self.observation

    def reset(self, obs: torch.Tensor, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Restart the envs with ``mask`` set ([N] bool or uint8; None: every env) from ``obs`` [N, D]: a zero stack
        with the frame of ``obs`` (noised, zero command) last, ``prev_command`` zero. Returns `observation`."""
        obs = device_tensor(obs, "obs", self.device, (self.num_envs, self.obs_dim))
        mask = device_tensor(mask, "mask", self.device, (self.num_envs,), (torch.bool, torch.uint8), required=False)
        self._launcher(self._lib.upkie_pipeline_reset, *self._settings(), obs.data_ptr(), ptr(mask), self.prev_command.data_ptr(),
                       self.calls.data_ptr(), self.observation.data_ptr())
        return self.observation

    def state_tensors(self) -> dict:
        """The three tensors the next call reads (what `Ppo.save` carries)."""
        return {"prev_command": self.prev_command, "observation": self.observation, "calls": self.calls}
