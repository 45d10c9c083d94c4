"""The row an asymmetric critic reads: what the simulator knows and the robot will never see.

`AgentPipeline` noises and lags what the policy observes, `EpisodeEvents` pushes the robot and redraws its link inertias
every episode; a value function fed the policy's observation cannot see the push that is acting or the inertias this
episode drew. `PrivilegedObservation` assembles, in one launch per env step (``upkie_privileged_observation``:
csrc/privileged_obs.hpp; include/upkie_hip.h states the row), the concatenation of the raw next observation, the command
the env received, the force the next step applies and the scales of the links the model randomises -- the input of the
critic of an asymmetric `MlpActorCritic` (``Ppo(critic_observation=...)``). The critic is not deployed: evaluation and
the spine never build this row."""

from typing import Optional, Sequence

import torch

from . import abi, lib
from .exceptions import UpkieRuntimeError
from .launch import device_tensor, end_flags, launcher, ptr

SEGMENTS = ("observation", "command", "push_force", "link_scale")
_KINDS = {"observation": abi.PRIVILEGED_OBSERVATION, "command": abi.PRIVILEGED_COMMAND, "push_force": abi.PRIVILEGED_PUSH_FORCE,
          "link_scale": abi.PRIVILEGED_LINK_SCALE}


class PrivilegedObservation:
    """``observation`` ``[N, Dc]`` and ``final_observation`` ``[N, Dc]`` for the envs of ``env``.

    Per env the row is the concatenation, in ``include``'s order, of: ``"observation"``, the raw next observation
    (un-noised, unstacked; the env's ``[N, D]`` block); ``"command"``, the pipeline's current `command` (A words; needs
    ``pipeline``); ``"push_force"``, the force the next step will apply (the 3 words of ``events.force[0, :, n]``;
    needs ``events``); ``"link_scale"``, the `link_scale` of the links the model randomises (needs ``events`` with
    ``inertia_variation > 0``). A segment whose source is absent is refused, not skipped.

    ``step(next_obs, terminated, truncated, final_obs)`` runs after ``events.step`` (`upkie_amd.agent_step.AgentStep`:
    after `apply`) and writes both buffers. Where the episode ended, ``final_observation[n]`` is ``final_obs[n]``
    followed by the non-observation words of the row that was current DURING the ended step -- the old content of
    ``observation[n]``, because by then ``events.step`` has zeroed the force and redrawn the inertias for the next
    episode. Elsewhere ``final_observation[n]`` is the new row. ``reset(obs)`` writes the first rows.

    Both buffers are allocated at construction; a call allocates nothing and has no host argument that changes between
    steps, so it can be captured in a hipGraph. Device only: there is no CPU fallback."""

    def __init__(self, env, events=None, pipeline=None, include: Sequence[str] = SEGMENTS, obs_dim: Optional[int] = None):
        include = tuple(include)
        if not include or len(set(include)) != len(include) or any(name not in SEGMENTS for name in include):
            raise ValueError(f"include must name each of {SEGMENTS} at most once, got {include}")
        self.include = include
        self.env, self.events, self.pipeline = env, events, pipeline
        self.num_envs = int(env.num_envs)
        self.device = torch.device(env.device)
        if self.device.type != "cuda":
            raise UpkieRuntimeError("PrivilegedObservation runs on the HIP device only (there is no CPU fallback): give it an env on 'cuda:0'")
        if obs_dim is None:
            if pipeline is not None:
                obs_dim = pipeline.obs_dim
            else:
                shape = tuple(getattr(getattr(env, "single_observation_space", None), "shape", ()) or ())
                if len(shape) != 1:
                    raise UpkieRuntimeError(f"PrivilegedObservation needs one [num_envs, obs_dim] float32 observation block, the env has {shape}")
                obs_dim = shape[0]
        self.obs_dim = int(obs_dim)
        for stage, what in ((events, "events"), (pipeline, "pipeline")):
            if stage is not None and int(stage.num_envs) != self.num_envs:
                raise ValueError(f"the {what} serve {int(stage.num_envs)} envs, the env has {self.num_envs}")
        self.act_dim = int(pipeline.act_dim) if pipeline is not None else 1
        links = []
        if "command" in include and pipeline is None:
            raise ValueError("include has 'command' but there is no pipeline (the command is the pipeline's)")
        if "push_force" in include and events is None:
            raise ValueError("include has 'push_force' but there are no events (the force is the events')")
        if "link_scale" in include:
            if events is None or events.link_scale is None:
                raise ValueError("include has 'link_scale' but the events draw no inertias (inertia_variation = 0, or no events)")
            model = getattr(env.model, "struct", env.model)  # (the UpkieModel record)
            links = [k for k in range(int(model.num_links)) if int(model.link_randomized[k])]
            if not links:
                raise ValueError("include has 'link_scale' but the model randomises no link")
        counts = {"observation": self.obs_dim, "command": self.act_dim, "push_force": 3, "link_scale": len(links)}
        self.counts = [counts[name] for name in include]
        self.kinds = [_KINDS[name] for name in include]
        self.dim = sum(self.counts)
        if not 1 <= self.dim <= 256:
            raise ValueError(f"the privileged row has {self.dim} words, the critic takes 1-256")
        self._lib = lib.load()
        lib.require(self._lib, "upkie_privileged_observation")
        self._launcher = launcher(self.device)
        i32 = dict(dtype=torch.int32, device=self.device)
        self.links = torch.tensor(links or [0], **i32)
        self._kinds, self._counts = torch.tensor(self.kinds, dtype=torch.int32), torch.tensor(self.counts, dtype=torch.int32)  # (host arrays)
        f32 = dict(dtype=torch.float32, device=self.device)
        self.observation = torch.zeros(self.num_envs, self.dim, **f32)
        self.final_observation = torch.zeros(self.num_envs, self.dim, **f32)

    def segment(self, name: str) -> slice:
        """The columns of segment ``name`` in a row."""
        k = self.include.index(name)
        start = sum(self.counts[:k])
        return slice(start, start + self.counts[k])

    def _launch(self, obs, final_obs, flags, reset: bool) -> None:
        ev, pipe = self.events, self.pipeline
        self._launcher(self._lib.upkie_privileged_observation, self.num_envs, self.obs_dim, self.act_dim, len(self.kinds), self._kinds.data_ptr(),
                       self._counts.data_ptr(), obs.data_ptr(), ptr(final_obs), ptr(pipe.command if pipe is not None else None),
                       ptr(ev.force if ev is not None else None), ptr(ev.link_scale if ev is not None else None), self.links.data_ptr(),
                       ptr(flags[0]), ptr(flags[1]), int(reset), self.observation.data_ptr(), self.final_observation.data_ptr())

    def step(self, next_obs: torch.Tensor, terminated: Optional[torch.Tensor] = None, truncated: Optional[torch.Tensor] = None,
             final_obs: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One env step, after ``events.step``: ``next_obs`` [N, D] float32 (raw), ``terminated`` / ``truncated`` [N] bool
        or uint8 (None: none ended), ``final_obs`` [N, D] (None: ``next_obs`` stands in). Returns `observation`."""
        N, D, dev = self.num_envs, self.obs_dim, self.device
        obs = device_tensor(next_obs, "next_obs", dev, (N, D))
        final = device_tensor(final_obs, "final_obs", dev, (N, D), required=False)
        self._launch(obs, final, end_flags(terminated, truncated, dev, N), False)
        return self.observation

    def reset(self, obs: torch.Tensor, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The first rows of the envs with ``mask`` set ([N] bool or uint8; None: every env) from ``obs`` [N, D] and the
        stages' current state (after their own resets). Returns `observation`."""
        obs = device_tensor(obs, "obs", self.device, (self.num_envs, self.obs_dim))
        mask = device_tensor(mask, "mask", self.device, (self.num_envs,), (torch.bool, torch.uint8), required=False)
        self._launch(obs, None, (mask, None), True)
        return self.observation

    def state_tensors(self) -> dict:
        """The rows the next call reads (what `Ppo.save` carries under ``critic_observation.``)."""
        return {"observation": self.observation, "final_observation": self.final_observation}
