"""Stable-Baselines3's ``Monitor`` + ``ep_info_buffer`` for a batch of envs, on the device.

SB3 reports ``rollout/ep_rew_mean`` and ``rollout/ep_len_mean`` from a per-env running sum of the raw reward, the
finished episodes pushed as ``{"r", "l"}`` into a deque of ``maxlen=stats_window_size`` in env order. As torch ops that
is several launches per step and a variable-length gather of the finished envs, i.e. a host synchronisation inside a
graphed rollout. `EpisodeStatistics` is one launch per step (``upkie_episodes_step``, csrc/episodes.hpp;
include/upkie_hip.h states the arithmetic) with all of its state on the device."""

from typing import List, Optional

import torch

from . import lib
from .exceptions import UpkieRuntimeError
from .launch import check, device_tensor, end_flags, launcher, ptr


class EpisodeStatistics:
    """SB3's ``Monitor`` (per-env return and length) and ``ep_info_buffer`` (the last ``window`` finished episodes) for
    ``num_envs`` envs.

    ``step(reward, terminated, truncated)`` adds the step's raw reward to every env's running return (fp64, summed in
    step order as Python's ``sum(Monitor.rewards)``) and one to its length; the envs with ``terminated | truncated``
    finish their episode, which enters the ring in increasing env index (more than ``window`` in one step: only the
    last ``window``, as a deque would keep). ``means`` (device, fp64) is then the mean return and the mean length over
    the ring, summed from the oldest entry to the newest. ``reset(mask)`` discards the running episodes of the masked
    envs (all without a mask) without recording them, as ``Monitor.reset``; the ring is kept.

    Differences from SB3: Monitor's ``round(r, 6)`` is not applied, and there is no ``"t"`` (wall-clock) entry.

    Order inside a rollout step, as in SB3 (Monitor sits under VecNormalize): ``EpisodeStatistics.step`` on the RAW
    reward comes between the two halves of `upkie_amd.agent_step.AgentStep` (after ``env.step`` and the user's reward),
    so before ``RunningNormalizer.step`` into ``buffer.rewards[t]`` and ``policy.bootstrap_time_limits(info["final_obs"],
    terminated, truncated, buffer.rewards[t], buffer.gamma)`` on the normalised slot.

    All state is allocated at construction; a step allocates nothing and has no host argument that changes between
    steps, so it can be captured in a hipGraph (`GraphedLoop`). Statistics are per process (per rank of a sharded
    run), as in SB3."""

    def __init__(self, num_envs: int, window: int = 100, device="cuda:0"):
        self.num_envs, self.window = int(num_envs), int(window)
        if self.num_envs < 1:
            raise ValueError("num_envs must be positive")
        if not 1 <= self.window <= 65536:
            raise ValueError("window must be in 1-65536")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise UpkieRuntimeError("EpisodeStatistics runs on the HIP device only (there is no CPU fallback): give device='cuda:0'")
        self._lib = lib.load()
        lib.require(self._lib, "upkie_episodes_step")
        nbytes = int(self._lib.upkie_episodes_workspace_bytes(self.num_envs))
        check(nbytes)
        self._launcher = launcher(self.device)
        N, W = self.num_envs, self.window
        self.ep_return = torch.zeros(N, dtype=torch.float64, device=self.device)
        self.ep_length = torch.zeros(N, dtype=torch.int32, device=self.device)
        self.ring_return = torch.zeros(W, dtype=torch.float64, device=self.device)
        self.ring_length = torch.zeros(W, dtype=torch.int32, device=self.device)
        self.counters = torch.zeros(3, dtype=torch.int64, device=self.device)  # episodes so far, ring head, ring fill
        self.means = torch.zeros(2, dtype=torch.float64, device=self.device)  # mean return, mean length over the ring
        self.workspace = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)  # (its ticket starts, and stays, at zero)

    def step(self, reward: torch.Tensor, terminated: Optional[torch.Tensor] = None, truncated: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One env step: ``reward`` [N] float32 (the raw reward, before any normalisation), ``terminated`` /
        ``truncated`` [N] bool or uint8 (None: none ended). Returns ``means``."""
        reward = device_tensor(reward, "reward", self.device, (self.num_envs,))
        terminated, truncated = end_flags(terminated, truncated, self.device, self.num_envs)
        self._launcher(self._lib.upkie_episodes_step, self.num_envs, self.window, reward.data_ptr(), ptr(terminated), ptr(truncated),
                       self.ep_return.data_ptr(), self.ep_length.data_ptr(), self.ring_return.data_ptr(), self.ring_length.data_ptr(),
                       self.counters.data_ptr(), self.means.data_ptr(), self.workspace.data_ptr())
        return self.means

    def reset(self, mask: Optional[torch.Tensor] = None) -> None:
        """Discard the running episodes of the envs with ``mask`` set ([N] bool or uint8; None: every env) without
        recording them (``Monitor.reset``). The ring and the means are kept."""
        mask = device_tensor(mask, "mask", self.device, (self.num_envs,), (torch.bool, torch.uint8), required=False)
        self._launcher(self._lib.upkie_episodes_reset, self.num_envs, ptr(mask), self.ep_return.data_ptr(), self.ep_length.data_ptr())

    def state_tensors(self) -> dict:
        """The running episodes, the ring, its counters and its means (what `Ppo.save` carries)."""
        return {"ep_return": self.ep_return, "ep_length": self.ep_length, "ring_return": self.ring_return, "ring_length": self.ring_length,
                "counters": self.counters, "means": self.means}

    # ---- host reads (each synchronises with the device)
    @property
    def total_episodes(self) -> int:
        """Episodes finished since construction."""
        return int(self.counters[0])

    def ep_rew_mean(self) -> Optional[float]:
        """``rollout/ep_rew_mean``: the mean return over the ring, None while it is empty (SB3 does not log it then)."""
        fill = int(self.counters[2])
        return None if fill == 0 else float(self.means[0])

    def ep_len_mean(self) -> Optional[float]:
        """``rollout/ep_len_mean``: the mean length over the ring, None while it is empty."""
        fill = int(self.counters[2])
        return None if fill == 0 else float(self.means[1])

    def ep_info_buffer(self) -> List[dict]:
        """The ring as SB3's ``ep_info_buffer``: ``[{"r": return, "l": length}, ...]``, oldest first."""
        head, fill = (int(x) for x in self.counters[1:].cpu())
        r, l = self.ring_return.cpu().tolist(), self.ring_length.cpu().tolist()
        first = (head - fill) % self.window
        return [{"r": r[(first + k) % self.window], "l": int(l[(first + k) % self.window])} for k in range(fill)]
