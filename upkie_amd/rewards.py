"""A declarative reward on the device: up to 16 weighted terms evaluated in one launch per rollout step.

The reference leaves the reward to the agent (``reward = 0.0  # to be decided by agents``), and a reward written as a
Python callable of torch ops is a launch per op, sees the observation only, and under same-step autoreset rewards the
RESET observation of an env whose episode has just ended. `RewardTerms` is one launch per step
(``upkie_reward_terms_step``: csrc/reward_terms.hpp; include/upkie_hip.h states the arithmetic): it reads the terminal
observation where an episode ended, taps the applied action, its rate of change and the ``terminated`` flag besides the
observation, and keeps per env and per term the fp64 sum of the running and of the last finished episode, which is
what one watches while tuning the weights (legged_gym's "episode sums")."""

import ctypes as C
import math
from collections import namedtuple
from typing import Mapping, Optional, Sequence, Tuple

import torch

from . import abi, lib
from .exceptions import UpkieRuntimeError
from .launch import check, device_tensor, end_flags, launcher, ptr

Tap = namedtuple("Tap", ("source", "index", "fn", "coef"))
_FNS = {None: abi.REWARD_FN_ID, "id": abi.REWARD_FN_ID, "sin": abi.REWARD_FN_SIN, "cos": abi.REWARD_FN_COS}
SHAPES = {"identity": abi.REWARD_IDENTITY, "abs": abi.REWARD_ABS, "square": abi.REWARD_SQUARE, "exp_abs": abi.REWARD_EXP_ABS,
          "exp_square": abi.REWARD_EXP_SQUARE, "deadband": abi.REWARD_DEADBAND}
_SCALED = ("exp_abs", "exp_square", "deadband")


def _tap(source: int, index: int, coef: float, fn: Optional[str]) -> Tap:
    if fn not in _FNS:
        raise ValueError(f"a tap's fn is None, 'sin' or 'cos', got {fn!r}")
    return Tap(source, int(index), _FNS[fn], float(coef))


def obs(i: int, coef: float = 1.0, fn: Optional[str] = None) -> Tap:
    """``coef * fn(o[i])``: word ``i`` of the raw observation (the terminal one where the episode ended)."""
    return _tap(abi.REWARD_OBS, i, coef, fn)


def act(j: int, coef: float = 1.0, fn: Optional[str] = None) -> Tap:
    """``coef * fn(a[j])``: word ``j`` of the action applied this step."""
    return _tap(abi.REWARD_ACTION, j, coef, fn)


def act_rate(j: int, coef: float = 1.0, fn: Optional[str] = None) -> Tap:
    """``coef * fn((a[j] - previous a[j]) / dt)``; the previous action of an episode's first step is 0."""
    return _tap(abi.REWARD_ACTION_RATE, j, coef, fn)


def one(coef: float = 1.0, fn: Optional[str] = None) -> Tap:
    """``coef * fn(1)``: a constant (an alive bonus)."""
    return _tap(abi.REWARD_ONE, 0, coef, fn)


def terminated(coef: float = 1.0, fn: Optional[str] = None) -> Tap:
    """``coef * fn(1 if terminated else 0)``: a fall penalty that a time limit does not trigger."""
    return _tap(abi.REWARD_TERMINATED, 0, coef, fn)


class Term:
    """``weight * shape(sum of the taps; scale)``. ``shape``: "identity", "abs", "square", "exp_abs"
    (``exp(-|x| / scale)``), "exp_square" (``exp(-(x / scale)^2)``) or "deadband" (``max(|x| - scale, 0)``); the last
    three need ``scale > 0``."""

    def __init__(self, weight: float, shape: str = "identity", scale: Optional[float] = None, taps: Sequence[Tap] = ()):
        self.weight, self.shape, self.scale, self.taps = weight, shape, scale, list(taps)


def pack_terms(obs_dim: int, act_dim: int, dt: float, terms, clip: Optional[Tuple[float, float]] = None) -> bytes:
    """Check ``terms`` (an ordered mapping, or a sequence of pairs, from a name to a `Term`) and pack the term table
    the kernel reads (``upkie_reward_terms_params``; host only, no device needed)."""
    obs_dim, act_dim = int(obs_dim), int(act_dim)
    pairs = list(terms.items()) if isinstance(terms, Mapping) else [(n, t) for n, t in terms]
    if not 1 <= obs_dim <= 256:
        raise ValueError("obs_dim must be in 1-256")
    if not 1 <= act_dim <= 64:
        raise ValueError("act_dim must be in 1-64")
    if not 1 <= len(pairs) <= abi.REWARD_MAX_TERMS:
        raise ValueError(f"a reward has 1-{abi.REWARD_MAX_TERMS} terms, got {len(pairs)}")
    dt = float(dt)
    if not (dt > 0.0 and math.isfinite(dt)):
        raise ValueError("dt must be positive and finite")
    names = [str(n) for n, _ in pairs]
    for name in names:
        if names.count(name) > 1:
            raise ValueError(f"duplicate term name {name!r}")
    low, high = (-math.inf, math.inf) if clip is None else (float(clip[0]), float(clip[1]))
    if not low <= high:
        raise ValueError("clip needs low <= high (and no NaN)")
    shapes, weights, scales, counts, sources, indices, fns, coefs = [], [], [], [], [], [], [], []
    for name, term in pairs:
        if not isinstance(term, Term):
            raise ValueError(f"term {name!r} must be a Term")
        if term.shape not in SHAPES:
            raise ValueError(f"term {name!r}: shape must be one of {', '.join(SHAPES)}, got {term.shape!r}")
        if not math.isfinite(float(term.weight)):
            raise ValueError(f"term {name!r}: the weight must be finite")
        if term.shape in _SCALED and (term.scale is None or not (float(term.scale) > 0.0 and math.isfinite(float(term.scale)))):
            raise ValueError(f"term {name!r}: shape {term.shape!r} needs a positive, finite scale")
        if not 1 <= len(term.taps) <= abi.REWARD_MAX_TAPS:
            raise ValueError(f"term {name!r}: a term has 1-{abi.REWARD_MAX_TAPS} taps, got {len(term.taps)}")
        for tap in term.taps:
            if not isinstance(tap, Tap):
                raise ValueError(f"term {name!r}: taps are built with obs(), act(), act_rate(), one() and terminated()")
            if not math.isfinite(tap.coef):
                raise ValueError(f"term {name!r}: tap coefficients must be finite")
            if tap.source == abi.REWARD_OBS and not 0 <= tap.index < obs_dim:
                raise ValueError(f"term {name!r}: obs({tap.index}) is beyond the observation's {obs_dim} words")
            if tap.source in (abi.REWARD_ACTION, abi.REWARD_ACTION_RATE) and not 0 <= tap.index < act_dim:
                raise ValueError(f"term {name!r}: action word {tap.index} is beyond the action's {act_dim} words")
            sources.append(tap.source), indices.append(tap.index), fns.append(tap.fn), coefs.append(tap.coef)
        shapes.append(SHAPES[term.shape]), weights.append(float(term.weight)), counts.append(len(term.taps))
        scales.append(float(term.scale) if term.shape in _SCALED else 1.0)
    library = lib.load()
    lib.require(library, "upkie_reward_terms_step")
    ints = lambda v: (C.c_int32 * len(v))(*v)  # noqa: E731
    floats = lambda v: (C.c_float * len(v))(*v)  # noqa: E731
    out = C.create_string_buffer(abi.REWARD_PARAMS_BYTES)
    nbytes = int(library.upkie_reward_terms_params(obs_dim, act_dim, len(pairs), dt, ints(shapes), floats(weights), floats(scales), ints(counts),
                                                   ints(sources), ints(indices), ints(fns), floats(coefs), low, high, out))
    check(nbytes)
    if nbytes != abi.REWARD_PARAMS_BYTES:
        raise UpkieRuntimeError(f"the library packs {nbytes} B of reward parameters, upkie_amd/abi.py expects {abi.REWARD_PARAMS_BYTES}: rebuild it")
    return out.raw


class RewardTerms:
    """The reward of ``num_envs`` envs with ``[num_envs, obs_dim]`` float32 raw observations and ``act_dim`` actions:
    ``terms`` maps a name to a `Term`, in the order the terms are summed; ``dt`` is the env step (the rate taps'
    divisor); ``clip=(low, high)`` clamps the reward (not the per-term sums).

    ``step(next_obs, action, terminated, truncated, final_obs)`` returns the step's reward. Where an episode ended it is
    computed from ``final_obs`` (same-step autoreset: ``next_obs`` is then already the reset observation); ``action``
    is what was applied this step, and an episode's first rate is taken against a zero action. `term_sum` ``[K, N]``
    fp64 is every term's sum over the running episode, `term_last` the same of the env's last finished episode,
    `finished` ``[N]`` the episodes an env has finished; `term_means` reports them. Non-finite inputs pass through: a
    poisoned `term_sum` lasts until that env's episode ends. ``reset(mask)`` forgets the running episodes.

    All state is allocated at construction; a step allocates nothing and has no host argument that changes between
    steps, so it can be captured in a hipGraph (`GraphedLoop`), and it gives the same bits every call. Device only:
    there is no CPU fallback. Statistics are per process (per rank of a sharded run)."""

    def __init__(self, num_envs: int, obs_dim: int, act_dim: int, dt: float, terms, clip: Optional[Tuple[float, float]] = None, device="cuda:0"):
        self.num_envs, self.obs_dim, self.act_dim, self.dt = int(num_envs), int(obs_dim), int(act_dim), float(dt)
        if self.num_envs < 1:
            raise ValueError("num_envs must be positive")
        pairs = list(terms.items() if isinstance(terms, Mapping) else terms)
        packed = pack_terms(self.obs_dim, self.act_dim, self.dt, pairs, clip)
        self.terms = dict(pairs)
        self.clip = None if clip is None else (float(clip[0]), float(clip[1]))
        self.names = tuple(str(n) for n in self.terms)
        self.num_terms = len(self.names)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise UpkieRuntimeError("RewardTerms runs on the HIP device only (there is no CPU fallback): give device='cuda:0'")
        self._lib = lib.load()
        self._launcher = launcher(self.device)
        N, A, K = self.num_envs, self.act_dim, self.num_terms
        self.params = torch.frombuffer(bytearray(packed), dtype=torch.uint8).to(self.device)
        self.prev_action = torch.zeros(A, N, dtype=torch.float32, device=self.device)
        self.term_sum = torch.zeros(K, N, dtype=torch.float64, device=self.device)
        self.term_last = torch.zeros(K, N, dtype=torch.float64, device=self.device)
        self.finished = torch.zeros(N, dtype=torch.int32, device=self.device)
        self.reward = torch.zeros(N, dtype=torch.float32, device=self.device)

    def step(self, next_obs: torch.Tensor, action: torch.Tensor, terminated: Optional[torch.Tensor] = None,
             truncated: Optional[torch.Tensor] = None, final_obs: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One env step: ``next_obs`` / ``final_obs`` [N, D] float32 (``final_obs`` None: ``next_obs`` everywhere),
        ``action`` [N, A] float32, ``terminated`` / ``truncated`` [N] bool or uint8 (None: none). Returns the reward
        [N] float32, written into ``out`` when given (a rollout buffer's slot), else into `reward`."""
        N, D, A, dev = self.num_envs, self.obs_dim, self.act_dim, self.device
        obs_ = device_tensor(next_obs, "next_obs", dev, (N, D))
        action = device_tensor(action, "action", dev, (N, A))
        term, trunc = end_flags(terminated, truncated, dev, N)
        final = device_tensor(final_obs, "final_obs", dev, (N, D), required=False)
        out = self.reward if out is None else device_tensor(out, "out", dev, (N,))
        self._launcher(self._lib.upkie_reward_terms_step, N, D, A, self.num_terms, self.params.data_ptr(), obs_.data_ptr(), action.data_ptr(),
                       ptr(term), ptr(trunc), ptr(final), self.prev_action.data_ptr(), self.term_sum.data_ptr(), self.term_last.data_ptr(),
                       self.finished.data_ptr(), out.data_ptr())
        return out

    def reset(self, mask: Optional[torch.Tensor] = None) -> None:
        """Forget the running episodes of the envs with ``mask`` set ([N] bool or uint8; None: every env): their
        `term_sum` and `prev_action` go back to zero. `term_last` and `finished` are kept."""
        mask = device_tensor(mask, "mask", self.device, (self.num_envs,), (torch.bool, torch.uint8), required=False)
        self._launcher(self._lib.upkie_reward_terms_reset, self.num_envs, self.act_dim, self.num_terms, ptr(mask), self.prev_action.data_ptr(),
                       self.term_sum.data_ptr())

    def state_tensors(self) -> dict:
        """The tensors the next call and the next report read (what `Ppo.save` carries)."""
        return {"prev_action": self.prev_action, "term_sum": self.term_sum, "term_last": self.term_last, "finished": self.finished}

    def term_means(self) -> dict:
        """``{name: mean of term_last[k] over the envs that have finished an episode}``, None for every name while no env
        has: reduced on the device in fp64, read with one device-to-host copy."""
        done = self.finished > 0
        sums = torch.where(done, self.term_last, torch.zeros((), dtype=torch.float64, device=self.device)).sum(dim=1)
        host = torch.cat([sums, done.sum().to(torch.float64).reshape(1)]).cpu().tolist()
        count = host[-1]
        return {name: (None if count == 0 else host[k] / count) for k, name in enumerate(self.names)}
