"""What happens to an env between two steps of a rollout, decided on the device: random pushes and a fresh draw of the
link inertias for every episode.

`BatchedSim.sample_pushes` draws one push for every env at once and leaves holding and ending it to a host loop, and
`randomize_inertias` draws once for the life of the handle: neither can live in a captured rollout. `EpisodeEvents` is one
launch per env step (``upkie_sim_episode_events_step``: csrc/episode_events.hpp; include/upkie_hip.h states the
arithmetic) with all of its state on the device; the step kernels are not involved, they read the force buffer and the
inertial records this stage writes as they read any a caller installed."""

import ctypes as C
import math
from typing import Optional

import torch

from . import abi, lib
from .exceptions import UpkieRuntimeError
from .launch import device_tensor, end_flags, ptr


def events_params(push_prob=0.0, push_norm=(0.0, 20.0), push_steps=(1, 1), inertia_variation=0.0) -> abi.UpkieEpisodeEvents:
    """The checked settings as the library reads them (``UpkieEpisodeEvents``); ``ValueError`` on any out of range."""
    try:
        prob, variation = float(push_prob), float(inertia_variation)
        norm_min, norm_max = (float(v) for v in push_norm)
        raw_steps = tuple(push_steps)
        steps_min, steps_max = (int(v) for v in raw_steps)
    except (TypeError, ValueError) as err:
        raise ValueError(f"push_prob and inertia_variation are numbers, push_norm and push_steps pairs (min, max): {err}") from None
    if not 0.0 <= prob <= 1.0:
        raise ValueError(f"push_prob must be in [0, 1], got {push_prob}")
    if not (math.isfinite(norm_min) and math.isfinite(norm_max) and 0.0 <= norm_min <= norm_max):
        raise ValueError(f"push_norm must be finite with 0 <= min <= max, got {tuple(push_norm)}")
    if any(float(v) != int(v) for v in raw_steps) or not 1 <= steps_min <= steps_max <= 65535:
        raise ValueError(f"push_steps must be whole numbers with 1 <= min <= max <= 65535, got {raw_steps}")
    if not 0.0 <= variation < 1.0:
        raise ValueError(f"inertia_variation must be in [0, 1), got {inertia_variation}")
    if prob == 0.0 and variation == 0.0:
        raise ValueError("push_prob and inertia_variation are both 0: nothing to do")
    p = abi.UpkieEpisodeEvents()
    p.push_prob, p.push_norm_min, p.push_norm_max, p.inertia_variation = prob, norm_min, norm_max, variation
    p.push_steps_min, p.push_steps_max = steps_min, steps_max
    return p


class EpisodeEvents:
    """Random pushes and per-episode inertias for the envs of ``env`` (a `upkie_amd.envs.UpkieVecEnv`: its simulation
    handle, model, ``num_envs`` and device).

    ``step(terminated, truncated)`` runs after the env step that produced the two flags and decides the NEXT step, per
    env n and in this order: 1. one Philox block keyed (global env id, ``calls[n]``, a stream tag of its own) under the
    sim's seed, then ``calls[n] += 1``: every env draws at every call, so its schedule depends neither on the batch, nor
    on the sharding, nor on other envs; 2. if the episode ended: ``episodes[n] += 1``, ``remaining[n] = 0`` (a push does
    not outlive its episode) and, with ``inertia_variation > 0``, the env's link factors are drawn as
    `BatchedSim.randomize_inertias` draws them but keyed by ``episodes[n]``, and fused into its inertial records; 3. a
    held force counts down; 4. on a free step (``remaining[n] == 0``) a push starts with probability ``push_prob``: push
    number ``pushes[n]`` of env n as `BatchedSim.sample_pushes` defines it, but with its norm uniform in ``push_norm``,
    on ``push_link``, horizontal, in the world frame, held a number of steps uniform in ``push_steps``; without a start
    the force is zero; 5. a held force is left as it is. ``push_steps=(1, 1)`` is an independent Bernoulli draw per env
    step, ``(20, 20)`` the held pushes of the C5 benchmark schedule, unsynchronised across envs.

    ``reset(mask)`` zeroes the counters and the force of the masked envs (None: all) and, with inertia randomisation,
    gives them the records of episode 0, which are `randomize_inertias`'s.

    Construction installs `force` ``[1, 3, N]`` (``sim.set_external_forces``) and, with ``inertia_variation > 0``,
    `body_inertials` ``[70, N]`` (``sim.set_body_inertials``) in the simulation ONCE, and refuses an env that already
    carries external forces. A later ``env.set_external_forces`` replaces the force buffer: the stage then writes
    pushes that no step reads. The sim's seed and env id offset are read at every call (when a hipGraph is recorded: at
    the recording).

    All state is allocated at construction; a call allocates nothing and has no host argument that changes between
    steps, so it can be captured in a hipGraph. In a sharded run every process builds its own stage: the draws are keyed
    by global env ids. Device only: there is no CPU fallback."""

    def __init__(self, env, push_prob: float = 0.0, push_norm=(0.0, 20.0), push_steps=(1, 1), push_link: str = "torso",
                 inertia_variation: float = 0.0):
        self.params = events_params(push_prob, push_norm, push_steps, inertia_variation)  # (every range, before any device use)
        self.push_prob, self.inertia_variation = self.params.push_prob, self.params.inertia_variation
        self.push_norm = (self.params.push_norm_min, self.params.push_norm_max)
        self.push_steps = (self.params.push_steps_min, self.params.push_steps_max)
        self.threshold = int(math.floor(self.push_prob * 2 ** 24 + 0.5))  # llround: a push starts iff a 24-bit word is below it
        model = env.model
        if push_link not in model.link_names:
            raise ValueError(f"the model has no link named '{push_link}'")
        self.push_link = push_link
        self.env, self.num_envs = env, int(env.num_envs)
        self.device = torch.device(env.device)
        if self.device.type != "cuda":
            raise UpkieRuntimeError("EpisodeEvents runs on the HIP device only (there is no CPU fallback): give it an env on 'cuda:0'")
        sim = self.sim = env.sim
        if getattr(sim, "ext_force", None) is not None:
            raise ValueError("the env already carries external forces: EpisodeEvents installs its own force buffer (remove them first)")
        self._lib = lib.load()
        lib.require(self._lib, "upkie_sim_episode_events_step")
        N, dev = self.num_envs, self.device
        i32 = dict(dtype=torch.int32, device=dev)
        self.calls = torch.zeros(N, **i32)  # (uint32 words)
        self.remaining = torch.zeros(N, **i32)
        self.pushes = torch.zeros(N, **i32)  # (uint32 words)
        self.episodes = torch.zeros(N, **i32)  # (uint32 words)
        self.force = torch.zeros((1, 3, N), dtype=torch.float32, device=dev)
        self.body_inertials = self.link_scale = None
        body, point, _ = model.link_attachment(push_link)
        sim.set_external_forces(self.force, bodies=[int(body)], points=[[float(x) for x in point]], local=[False])
        if self.inertia_variation > 0.0:
            self.body_inertials = torch.zeros((abi.NB * abi.INERTIAL_WORDS, N), dtype=torch.float32, device=dev)
            self.link_scale = torch.ones((abi.MAX_LINKS, N), dtype=torch.float32, device=dev)
            self.reset()  # (the records of episode 0, before the sim is pointed at them)
            sim.set_body_inertials(self.body_inertials)
            sim.link_scale = self.link_scale
        if sim.ext_force.data_ptr() != self.force.data_ptr() or (self.body_inertials is not None and sim.body_inertials.data_ptr() != self.body_inertials.data_ptr()):
            raise UpkieRuntimeError("the simulation did not take the events' own buffers (it copied them)")

    def _state(self):
        return (ptr(self.calls), ptr(self.remaining), ptr(self.pushes), ptr(self.episodes), ptr(self.force), ptr(self.body_inertials),
                ptr(self.link_scale))

    def step(self, terminated: Optional[torch.Tensor] = None, truncated: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One env step is over: ``terminated`` / ``truncated`` [N] bool or uint8 (None: none ended). Returns `force`."""
        term, trunc = end_flags(terminated, truncated, self.device, self.num_envs)
        self.sim._launch(self._lib.upkie_sim_episode_events_step, C.byref(self.params), ptr(term), ptr(trunc), *self._state())
        return self.force

    def reset(self, mask: Optional[torch.Tensor] = None) -> None:
        """Restart the envs with ``mask`` set ([N] bool or uint8; None: every env)."""
        mask = device_tensor(mask, "mask", self.device, (self.num_envs,), (torch.bool, torch.uint8), required=False)
        self.sim._launch(self._lib.upkie_sim_episode_events_reset, C.byref(self.params), ptr(mask), *self._state())

    def state_tensors(self) -> dict:
        """Everything a resumed run needs (what `Ppo.save` carries under ``events.``)."""
        named = {"calls": self.calls, "remaining": self.remaining, "pushes": self.pushes, "episodes": self.episodes, "force": self.force,
                 "body_inertials": self.body_inertials, "link_scale": self.link_scale}
        return {k: v for k, v in named.items() if v is not None}
