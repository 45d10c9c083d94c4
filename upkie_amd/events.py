"""What happens to an env between two steps of a rollout, decided on the device: random pushes and a fresh draw of the
link inertias for every episode.

`BatchedSim.sample_pushes` draws one push for every env at once and leaves holding and ending it to a host loop, and
`randomize_inertias` draws once for the life of the handle: neither can live in a captured rollout. `EpisodeEvents` is one
launch per env step (``upkie_sim_episode_events_step``: csrc/episode_events.hpp; include/upkie_hip.h states the
arithmetic) with all of its state on the device; the step kernels are not involved, they read the force buffer and the
inertial records this stage writes as they read any a caller installed. `PushLevels` and ``live`` are the push
curriculum: a difficulty level per env, decided in the same launch, and the push settings in a device block."""

import ctypes as C
import math
from typing import Optional

import numpy as np
import torch

from . import abi, lib
from .exceptions import UpkieRuntimeError
from .launch import device_tensor, end_flags, ptr

TWO_24 = 16777216.0  # a push starts iff a 24-bit word is below llround(push_prob * 2^24)


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


class PushLevels:
    """The checked settings of the per-env push curriculum (include/upkie_hip.h, "Push curriculum"): ``levels`` = L, the
    top difficulty level (0-255); an env starts at ``start``, goes ``up`` levels when its episode reaches the time limit
    after at least ``min_pushes`` push starts, and ``down`` levels (not below 0) when the robot falls. At level l the
    env's push norms are uniform in ``[norm_min, norm_min + (norm_max - norm_min) * l / L]``; at L, in ``push_norm``.
    ``PushLevels(L, start=L, up=0, down=0)`` holds every env at the top: an evaluation at a fixed difficulty.
    ``ValueError`` on anything out of range."""

    def __init__(self, levels: int, start: int = 0, up: int = 1, down: int = 1, min_pushes: int = 1):
        named = dict(levels=levels, start=start, up=up, down=down, min_pushes=min_pushes)
        for name, value in named.items():
            if isinstance(value, bool) or not isinstance(value, (int, float)) or value != value or float(value) != int(value):
                raise ValueError(f"{name} must be a whole number, got {value!r}")
        levels, start, up, down, min_pushes = (int(v) for v in named.values())
        if not 0 <= levels <= abi.EVENTS_LEVELS_MAX:
            raise ValueError(f"levels must be in 0-{abi.EVENTS_LEVELS_MAX}, got {levels}")
        for name, value in (("start", start), ("up", up), ("down", down)):
            if not 0 <= value <= levels:
                raise ValueError(f"{name} must be in 0-levels (0-{levels}), got {value}")
        if not 0 <= min_pushes < 2 ** 31:
            raise ValueError(f"min_pushes must be in 0-{2 ** 31 - 1}, got {min_pushes}")
        self.levels, self.start, self.up, self.down, self.min_pushes = levels, start, up, down, min_pushes

    def __repr__(self):
        return f"PushLevels(levels={self.levels}, start={self.start}, up={self.up}, down={self.down}, min_pushes={self.min_pushes})"


def settings_words(params: abi.UpkieEpisodeEvents, curriculum: PushLevels) -> torch.Tensor:
    """The device block of the levelled launch as a host tensor of ``abi.EVENTS_SETTINGS_WORDS`` int32 (32-bit words: the
    two norms are float32 bit patterns), from checked settings."""
    words = np.zeros(abi.EVENTS_SETTINGS_WORDS, dtype=np.uint32)
    named = dict(threshold=int(math.floor(params.push_prob * TWO_24 + 0.5)), steps_min=params.push_steps_min,
                 steps_span=params.push_steps_max - params.push_steps_min + 1, levels=curriculum.levels, up=curriculum.up,
                 down=curriculum.down, min_pushes=curriculum.min_pushes)
    for name, value in named.items():
        words[abi.EVENTS_SETTINGS.index(name)] = value
    norms = np.array([params.push_norm_min, params.push_norm_max], dtype=np.float32)
    words[abi.EVENTS_SETTINGS.index("norm_min"):abi.EVENTS_SETTINGS.index("norm_max") + 1] = norms.view(np.uint32)
    return torch.from_numpy(words.view(np.int32).copy())


def settings_values(words: torch.Tensor) -> dict:
    """What a block says: its words by name, the norms as floats, and ``push_prob`` / ``push_steps`` as `set_push` takes
    them (``threshold / 2^24`` gives the threshold back under llround)."""
    raw = words.numpy().view(np.uint32)
    out = {name: int(raw[i]) for i, name in enumerate(abi.EVENTS_SETTINGS)}
    norms = raw[abi.EVENTS_SETTINGS.index("norm_min"):abi.EVENTS_SETTINGS.index("norm_max") + 1].copy().view(np.float32)
    out["norm_min"], out["norm_max"] = float(norms[0]), float(norms[1])
    out["push_prob"] = out["threshold"] / TWO_24
    out["push_steps"] = (out["steps_min"], out["steps_min"] + max(out["steps_span"], 1) - 1)
    return out


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
    by global env ids. Device only: there is no CPU fallback.

    ``curriculum`` (a `PushLevels`) and ``live``: with neither, the object is the one above, launch for launch. With
    either, probability, norm range and hold steps live in the device block `settings` that the launch
    (``upkie_sim_episode_events_step_levels``) reads at every call, so `set_push` (a device copy, outside any capture) is
    followed by a captured rollout at its next replay, and the stage carries `level`, `episode_pushes` and `difficulty`
    ``[N]``: an env's level rises when its episode reaches the time limit under pushes, falls when the robot falls, and
    scales the upper end of that env's push norms (`PushLevels`). ``live=True`` alone is ``PushLevels(0, up=0, down=0)``:
    one level, the norms of ``push_norm``, the bits of the plain stage. A level depends on its env's own history alone:
    there is no reduction and no host decision, and a sharded run exchanges nothing. `set_levels` places envs,
    `level_counts` is the histogram, `log` what `Ppo` records."""

    def __init__(self, env, push_prob: float = 0.0, push_norm=(0.0, 20.0), push_steps=(1, 1), push_link: str = "torso",
                 inertia_variation: float = 0.0, curriculum: Optional[PushLevels] = None, live: bool = False):
        if curriculum is not None and not isinstance(curriculum, PushLevels):
            raise ValueError(f"curriculum must be a PushLevels (or None), got {type(curriculum).__name__}")
        self.curriculum, self.live = curriculum, bool(live)
        self._levels = curriculum if curriculum is not None else (PushLevels(0, up=0, down=0) if live else None)
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
        self.settings = self.level = self.episode_pushes = self.difficulty = None
        if self._levels is not None:
            lib.require(self._lib, "upkie_sim_episode_events_step_levels", "for a push curriculum or live push settings")
            self._block_host = settings_words(self.params, self._levels)  # (set_push's staging words)
            self.settings = self._block_host.to(dev)  # (uint32 and float32 words)
            self.level = torch.full((N,), self._levels.start, **i32)  # (uint32 words)
            self.episode_pushes = torch.zeros(N, **i32)  # (uint32 words)
            self.difficulty = torch.zeros(N, dtype=torch.float32, device=dev)
            self._counts = torch.zeros(abi.EVENTS_LEVELS_MAX + 1, **i32)  # (uint32 words)
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
        if self.inertia_variation > 0.0 or self._levels is not None:
            self.reset()  # (the records of episode 0, before the sim is pointed at them; the start level's difficulty)
        if self.inertia_variation > 0.0:
            sim.set_body_inertials(self.body_inertials)
            sim.link_scale = self.link_scale
        if sim.ext_force.data_ptr() != self.force.data_ptr() or (self.body_inertials is not None and sim.body_inertials.data_ptr() != self.body_inertials.data_ptr()):
            raise UpkieRuntimeError("the simulation did not take the events' own buffers (it copied them)")

    def _state(self):
        return (ptr(self.calls), ptr(self.remaining), ptr(self.pushes), ptr(self.episodes), ptr(self.force), ptr(self.body_inertials),
                ptr(self.link_scale))

    def _level_state(self):
        return (ptr(self.calls), ptr(self.remaining), ptr(self.pushes), ptr(self.episodes), ptr(self.level), ptr(self.episode_pushes),
                ptr(self.difficulty), ptr(self.force), ptr(self.body_inertials), ptr(self.link_scale))

    def step(self, terminated: Optional[torch.Tensor] = None, truncated: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One env step is over: ``terminated`` / ``truncated`` [N] bool or uint8 (None: none ended). Returns `force`."""
        term, trunc = end_flags(terminated, truncated, self.device, self.num_envs)
        if self._levels is not None:
            self.sim._launch(self._lib.upkie_sim_episode_events_step_levels, self.inertia_variation, ptr(self.settings), ptr(term), ptr(trunc),
                             *self._level_state())
            return self.force
        self.sim._launch(self._lib.upkie_sim_episode_events_step, C.byref(self.params), ptr(term), ptr(trunc), *self._state())
        return self.force

    def reset(self, mask: Optional[torch.Tensor] = None) -> None:
        """Restart the envs with ``mask`` set ([N] bool or uint8; None: every env)."""
        mask = device_tensor(mask, "mask", self.device, (self.num_envs,), (torch.bool, torch.uint8), required=False)
        if self._levels is not None:
            self.sim._launch(self._lib.upkie_sim_episode_events_reset_levels, self.inertia_variation, ptr(self.settings), self._levels.start,
                             ptr(mask), *self._level_state())
            return
        self.sim._launch(self._lib.upkie_sim_episode_events_reset, C.byref(self.params), ptr(mask), *self._state())

    def state_tensors(self) -> dict:
        """Everything a resumed run needs (what `Ppo.save` carries under ``events.``)."""
        named = {"calls": self.calls, "remaining": self.remaining, "pushes": self.pushes, "episodes": self.episodes, "force": self.force,
                 "body_inertials": self.body_inertials, "link_scale": self.link_scale, "settings": self.settings, "level": self.level,
                 "episode_pushes": self.episode_pushes, "difficulty": self.difficulty}
        return {k: v for k, v in named.items() if v is not None}

    # ---- the push curriculum and the live settings
    def _need_block(self, what: str) -> None:
        if self._levels is None:
            raise UpkieRuntimeError(f"{what} needs the push settings in a device block: build the EpisodeEvents with live=True or "
                                    "curriculum=PushLevels(...) (without, they are arguments of the launch a captured rollout has recorded)")

    def set_push(self, prob: Optional[float] = None, norm=None, steps=None) -> None:
        """New ``push_prob``, ``push_norm`` (min, max) and / or ``push_steps`` (min, max); None keeps what the block holds
        (read back first: a loaded checkpoint's, say). Checked as at construction, then written with one device copy from
        the staging words: the next call's settings, a captured rollout's included. Call it outside any capture."""
        self._need_block("set_push")
        self._block_host.copy_(self.settings)
        now = settings_values(self._block_host)
        prob = now["push_prob"] if prob is None else prob
        norm = (now["norm_min"], now["norm_max"]) if norm is None else norm
        steps = now["push_steps"] if steps is None else steps
        self.params = events_params(prob, norm, steps, self.inertia_variation)
        self.push_prob, self.push_norm = self.params.push_prob, (self.params.push_norm_min, self.params.push_norm_max)
        self.push_steps = (self.params.push_steps_min, self.params.push_steps_max)
        self.threshold = int(math.floor(self.push_prob * TWO_24 + 0.5))
        kept = PushLevels(now["levels"], 0, now["up"], now["down"], now["min_pushes"])  # (the block's own: not set_push's to change)
        self._block_host.copy_(settings_words(self.params, kept))
        self.settings.copy_(self._block_host)

    def set_levels(self, levels) -> None:
        """Place the envs: one level for all (a whole number in 0-L) or a tensor ``[N]`` of them. `difficulty` follows
        at the next `step`. Call it outside any capture."""
        self._need_block("set_levels")
        top = self._levels.levels
        if isinstance(levels, torch.Tensor):
            if levels.dtype.is_floating_point or levels.dtype == torch.bool or levels.numel() != self.num_envs or levels.dim() != 1:
                raise ValueError(f"levels must be a whole number or an integer tensor [{self.num_envs}]")
            if self.num_envs and not (0 <= int(levels.min()) and int(levels.max()) <= top):
                raise ValueError(f"levels must be in 0-{top}")
            self.level.copy_(levels)
            return
        if isinstance(levels, bool) or not isinstance(levels, (int, float)) or levels != levels or float(levels) != int(levels):
            raise ValueError(f"levels must be a whole number or an integer tensor [{self.num_envs}], got {levels!r}")
        if not 0 <= int(levels) <= top:
            raise ValueError(f"levels must be in 0-{top}, got {levels}")
        self.level.fill_(int(levels))

    def level_counts(self) -> torch.Tensor:
        """``[L + 1]`` int32 on the device: the number of envs at every level (one memset and one launch, integer sums)."""
        self._need_block("level_counts")
        self.sim._launch(self._lib.upkie_sim_episode_events_level_counts, ptr(self.level), ptr(self._counts))
        return self._counts[:self._levels.levels + 1]

    def log(self) -> dict:
        """What a training record says about the pushes: with a curriculum ``push_level_mean`` and ``push_level_top_frac``
        (from `level_counts`), with ``live`` ``push_prob`` and ``push_norm_high`` (from the block); one device-to-host copy
        each. Without either: nothing."""
        out = {}
        if self.curriculum is not None:
            counts = self.level_counts().cpu().tolist()
            total = max(sum(counts), 1)
            out["push_level_mean"] = sum(l * c for l, c in enumerate(counts)) / total
            out["push_level_top_frac"] = counts[-1] / total
        if self.live:
            now = settings_values(self.settings.cpu())
            out["push_prob"], out["push_norm_high"] = now["push_prob"], now["norm_max"]
        return out
