"""A linear policy as ONE kernel launch, for the loop ``obs, ... = env.step(policy(obs))``.

The reference leaves the policy to the agent (README.md:60-67: ``action =
clamp(gains . obs)``; examples/pybullet/pd_balancing.py). Evaluated with torch
ops on the device -- ``(obs @ W).clamp(-c, c)`` -- it is two or three launches
of 2-5 us each (rocBLAS's gemv for a four-column matrix: 4.9 us) behind a
14.5 us step; `LinearPolicy` is one launch (`upkie_linear_policy`,
csrc/rollout.hpp) writing into a persistent action buffer. `MlpActorCritic` / `MlpPolicy` do the same for the
MLP policies of Stable-Baselines3 (csrc/policy_mlp.hpp)."""

import ctypes as C
from typing import Optional

import torch

from . import abi, lib
from .exceptions import UpkieRuntimeError
from .launch import check, launcher, ptr


class LinearPolicy:
    """``act = clamp(obs @ weights + bias, -clip, clip)`` on the device.

    ``weights`` is ``[obs_dim, act_dim]`` (or ``[obs_dim]`` for one action),
    ``bias`` ``[act_dim]`` or None, ``clip`` a positive bound or None. The call
    returns the policy's own ``[num_envs, act_dim]`` buffer, rewritten by every
    call (as the envs' output buffers are)."""

    def __init__(self, weights, bias=None, clip: Optional[float] = None, device="cuda:0"):
        self.device = torch.device(device)
        w = torch.as_tensor(weights, dtype=torch.float32)
        if w.dim() == 1:
            w = w[:, None]
        if w.dim() != 2:
            raise ValueError("weights must be [obs_dim] or [obs_dim, act_dim]")
        self.weights = w.to(self.device).contiguous()
        self.obs_dim, self.act_dim = (int(d) for d in self.weights.shape)
        self.bias = None if bias is None else torch.as_tensor(bias, dtype=torch.float32).reshape(self.act_dim).to(self.device).contiguous()
        self.clip = 0.0 if clip is None else float(clip)
        if clip is not None and not self.clip > 0.0:
            raise ValueError("clip must be positive (None: no clamp)")
        self._act = None
        self._lib = self._launcher = None

    def __call__(self, obs: torch.Tensor) -> torch.Tensor:
        if not obs.is_cuda:
            raise UpkieRuntimeError("LinearPolicy runs on the HIP device only (there is no CPU fallback)")
        if obs.dtype is not torch.float32 or not obs.is_contiguous():
            obs = obs.to(torch.float32).contiguous()
        n = obs.shape[0]
        if obs.numel() != n * self.obs_dim:
            raise ValueError(f"observation rows must hold {self.obs_dim} words")
        if self._act is None or self._act.shape[0] != n or self._act.device != obs.device:
            self._act = torch.empty((n, self.act_dim), dtype=torch.float32, device=obs.device)
            self._lib = lib.load()
            lib.require(self._lib, "upkie_linear_policy")
            self._launcher = launcher(obs.device)  # (the observations' device, as the action buffer)
        self._launcher(self._lib.upkie_linear_policy, n, self.obs_dim, self.act_dim, obs.data_ptr(), self.weights.data_ptr(), ptr(self.bias),
                       self.clip, self._act.data_ptr())
        return self._act


# ------------------------------------------------------------------ MLP actor-critic
# What sits between two env steps of a PPO rollout with Stable-Baselines3's MlpPolicy -- two towers of addmm +
# activation, the Gaussian draw, its log-probability, the clamp, the buffer copies: about 20 small launches as torch
# ops -- as ONE launch (`upkie_mlp_actor_critic`, csrc/policy_mlp.hpp) that writes straight into the rollout buffer and
# can be captured in a hipGraph together with the step.

_ACTIVATIONS = {"tanh": 0, "relu": 1}  # enum UpkieMlpActivation
OUTPUT_NAMES = ("norm_obs", "mean", "action", "env_action", "value", "log_prob")  # the kernel's outputs, in argument order
# the outputs of `upkie_mlp_actor_critic_asym` (an asymmetric policy: the critic reads a row of its own), in argument order
ASYM_OUTPUT_NAMES = ("norm_obs", "norm_critic_obs", "mean", "action", "env_action", "value", "log_prob")


def _tiles(width: int) -> int:
    return (int(width) + 15) // 16


def _width_class(shape) -> int:
    w = max([shape.obs_dim, shape.act_dim, shape.critic_obs_dim] + list(shape.actor_widths[: shape.actor_layers]) + list(shape.critic_widths[: shape.critic_layers]))
    for c in (16, 32, 64, 128, 256):
        if w <= c:
            return c
    raise ValueError(f"MLP width {w} above 256")


def pack_index(shape, sizes):
    """Gather map of the packed weight buffer (layout: csrc/policy_mlp.hpp): for each packed word, the index of its
    value in the concatenation of the flattened source tensors (`sizes`: their element counts, in the order of
    `MlpActorCritic.sources()`), or ``sum(sizes)`` -- one zero word appended to the concatenation -- for padding. An
    asymmetric shape (``critic_obs_dim > 0``) has two more sources, critic_obs_mean and critic_obs_std, after action_high."""
    import numpy as np

    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    zero = int(starts[-1])
    src = iter(range(len(sizes)))
    pair = 2 if _width_class(shape) >= 32 else 1
    D, A = int(shape.obs_dim), int(shape.act_dim)
    blocks = []

    def vector(n, padded):
        i = next(src)
        idx = np.full(padded, zero, dtype=np.int64)
        idx[:n] = starts[i] + np.arange(n)
        blocks.append(idx)

    def mfma_layer(n_in, n_out, first):
        wi, bi = next(src), next(src)
        in_t, out_t = _tiles(n_in), (_tiles(n_out) + pair - 1) // pair * pair
        o, t, lane, s = np.meshgrid(np.arange(out_t), np.arange(in_t), np.arange(64), np.arange(4), indexing="ij")
        unit = 16 * o + (lane & 15)
        k = 16 * t + (4 * s + (lane >> 4) if first else 4 * (lane >> 4) + s)
        blocks.append(np.where((unit < n_out) & (k < n_in), starts[wi] + unit * n_in + k, zero).reshape(-1))
        unit = np.arange(16 * out_t)
        blocks.append(np.where(unit < n_out, starts[bi] + unit, zero))

    def dot_layer(n_in):
        wi, bi = next(src), next(src)
        k = np.arange(16 * _tiles(n_in))
        blocks.append(np.where(k < n_in, starts[wi] + k, zero))
        blocks.append(np.array([starts[bi], zero, zero, zero], dtype=np.int64))

    def tower(n_in, layers, widths, outputs):
        for i in range(layers):
            mfma_layer(n_in, int(widths[i]), i == 0)
            n_in = int(widths[i])
        if outputs == 1:
            dot_layer(n_in)
        else:
            mfma_layer(n_in, outputs, layers == 0)

    dp = (D + 3) // 4 * 4
    vector(D, dp)  # obs_mean
    vector(D, dp)  # obs_std
    for _ in range(2):  # action_low, action_high
        vector(A, 16 * _tiles(A))
    Dc = int(shape.critic_obs_dim)
    for _ in range(2 if Dc else 0):  # critic_obs_mean, critic_obs_std (an asymmetric shape only)
        vector(Dc, (Dc + 3) // 4 * 4)
    vector(A, 16 * _tiles(A))  # log_std
    tower(D, int(shape.actor_layers), shape.actor_widths, A)
    if shape.critic_layers > 0:
        tower(Dc or D, int(shape.critic_layers), shape.critic_widths, 1)
    return np.concatenate(blocks)


def mlp_shape(actor_dims, critic_dims, activation: str, normalize: bool = False, clip_obs: float = 10.0) -> abi.UpkieMlpShape:
    """`abi.UpkieMlpShape` of an actor (and critic) given as the ``[out, in]`` shapes of their Linear weights, head
    last (``critic_dims`` empty: no critic). A critic whose first layer takes another number of inputs than the actor's
    makes the shape asymmetric: ``critic_obs_dim`` is that number (`critic_obs_dim` of `asymmetric_shape` forces it for a
    critic row as wide as the observation)."""
    if activation not in _ACTIVATIONS:
        raise ValueError(f"activation must be one of {sorted(_ACTIVATIONS)}")
    if not 2 <= len(actor_dims) <= abi.MLP_MAX_LAYERS + 1:
        raise ValueError(f"the actor needs 1-{abi.MLP_MAX_LAYERS} hidden layers and a head")
    if len(critic_dims) == 1 or len(critic_dims) > abi.MLP_MAX_LAYERS + 1:
        raise ValueError(f"the critic needs 1-{abi.MLP_MAX_LAYERS} hidden layers and a head (or nothing)")
    for what, dims in (("actor", actor_dims), ("critic", critic_dims)):
        for i, d in enumerate(dims):
            if len(d) != 2:
                raise ValueError(f"{what} layer {i}: weights must be [out, in]")
            if i and d[1] != dims[i - 1][0]:
                raise ValueError(f"{what} layer {i} takes {d[1]} inputs, the layer before gives {dims[i - 1][0]}")
    shape = abi.UpkieMlpShape()
    shape.obs_dim, shape.act_dim = int(actor_dims[0][1]), int(actor_dims[-1][0])
    if critic_dims and critic_dims[-1][0] != 1:
        raise ValueError(f"the critic must map its {critic_dims[0][1]} inputs to 1 value")
    if not 1 <= shape.obs_dim <= 256 or not 1 <= shape.act_dim <= 64:
        raise ValueError("obs_dim must be in 1-256, act_dim in 1-64")
    if critic_dims and critic_dims[0][1] != shape.obs_dim:
        shape.critic_obs_dim = int(critic_dims[0][1])
        if not 1 <= shape.critic_obs_dim <= 256:
            raise ValueError(f"the critic's observation must have 1-256 words, got {shape.critic_obs_dim}")
    shape.activation = _ACTIVATIONS[activation]
    shape.actor_layers = len(actor_dims) - 1
    shape.critic_layers = max(len(critic_dims) - 1, 0)
    for widths, dims in ((shape.actor_widths, actor_dims), (shape.critic_widths, critic_dims)):
        for i, d in enumerate(dims[:-1]):
            if not 1 <= d[0] <= 256:
                raise ValueError(f"hidden widths must be in 1-256, got {d[0]}")
            widths[i] = int(d[0])
    shape.normalize = int(bool(normalize))
    shape.clip_obs = float(clip_obs)
    if normalize and not shape.clip_obs > 0.0:
        raise ValueError("clip_obs must be positive")
    return shape


def asymmetric_shape(shape: abi.UpkieMlpShape, critic_obs_dim: Optional[int] = None) -> abi.UpkieMlpShape:
    """A copy of ``shape`` whose critic reads a row of its own of ``critic_obs_dim`` words (None: as many as the actor's
    observation -- the degenerate asymmetric shape, which `mlp_shape` cannot tell from a symmetric one)."""
    out = abi.UpkieMlpShape.from_buffer_copy(shape)
    if int(out.critic_layers) < 1:
        raise ValueError("an asymmetric shape needs a critic")
    out.critic_obs_dim = int(shape.obs_dim if critic_obs_dim is None else critic_obs_dim)
    if not 1 <= out.critic_obs_dim <= 256:
        raise ValueError(f"the critic's observation must have 1-256 words, got {out.critic_obs_dim}")
    return out


def sb3_parameters(state_dict):
    """(actor weights, actor biases, critic weights, critic biases, log_std) of the ``state_dict()`` of
    Stable-Baselines3's ``ActorCriticPolicy`` with separate networks, heads last: ``mlp_extractor.policy_net.{0,2,..}``
    + ``action_net``, ``mlp_extractor.value_net.{0,2,..}`` + ``value_net``, ``log_std``. (Key names only: SB3 is not
    imported.)"""
    if any(k.startswith("mlp_extractor.shared_net") for k in state_dict):
        raise ValueError("shared actor-critic layers are not supported (separate policy_net / value_net only)")
    for key in ("action_net.weight", "action_net.bias", "log_std"):
        if key not in state_dict:
            raise KeyError(f"state dict has no {key!r} (not an SB3 ActorCriticPolicy with a Gaussian action)")

    def stack(prefix):
        idx = sorted({int(k[len(prefix):].split(".")[0]) for k in state_dict if k.startswith(prefix) and k.endswith(".weight")})
        return [state_dict[f"{prefix}{i}.weight"] for i in idx], [state_dict[f"{prefix}{i}.bias"] for i in idx]

    aw, ab = stack("mlp_extractor.policy_net.")
    cw, cb = stack("mlp_extractor.value_net.")
    aw, ab = aw + [state_dict["action_net.weight"]], ab + [state_dict["action_net.bias"]]
    if "value_net.weight" in state_dict:
        cw, cb = cw + [state_dict["value_net.weight"]], cb + [state_dict["value_net.bias"]]
    else:
        cw, cb = [], []
    return aw, ab, cw, cb, state_dict["log_std"]


def _linear_stack(seq, what: str):
    """(weights, biases, activation name) of an ``nn.Sequential`` of Linear layers with one activation between them
    (hidden layers) and none after the last (the head)."""
    import torch.nn as nn

    if not isinstance(seq, nn.Sequential):
        raise TypeError(f"{what} must be an nn.Sequential of Linear and Tanh / ReLU modules")
    mods = list(seq)
    linears, act = [], None
    for i, m in enumerate(mods):
        if isinstance(m, nn.Linear):
            if m.bias is None:
                raise ValueError(f"{what}: Linear layers need a bias")
            linears.append(m)
            nxt = mods[i + 1] if i + 1 < len(mods) else None
            if nxt is None:
                continue
            name = "tanh" if isinstance(nxt, nn.Tanh) else "relu" if isinstance(nxt, nn.ReLU) else None
            if name is None:
                raise ValueError(f"{what}: a hidden Linear must be followed by Tanh or ReLU, not {type(nxt).__name__}")
            if act not in (None, name):
                raise ValueError(f"{what}: one activation per network (found {act} and {name})")
            act = name
        elif not isinstance(m, (nn.Tanh, nn.ReLU)):
            raise ValueError(f"{what}: unsupported module {type(m).__name__}")
    if not linears or not isinstance(mods[-1], nn.Linear):
        raise ValueError(f"{what} must end with a Linear head")
    return [m.weight for m in linears], [m.bias for m in linears], act


class MlpActorCritic:
    """An SB3-style MLP actor-critic on the device, one launch per call.

    ``act(obs)`` returns ``(env_action, action, value, log_prob)``: the action clamped to the action bounds (what the
    env gets), the raw Gaussian sample, the critic's value and the log-probability of the raw sample -- what PPO's
    rollout buffer stores. The tensors are the policy's persistent buffers, rewritten by every call, or the ones given
    in ``out=`` (a dict over `OUTPUT_NAMES`, e.g. ``{"action": buffer.actions[t], "value": buffer.values[t],
    "log_prob": buffer.log_probs[t], "norm_obs": buffer.observations[t]}``), which the kernel writes directly.

    Randomness: Philox4x32-10 keyed by ``seed``, counted by a per-env call counter in device memory (include/
    upkie_hip.h documents the mapping), so a call has no host argument that changes between calls and can be replayed
    from a hipGraph. ``reseed(seed)`` resets the counters (a new seed value is a new launch argument: re-capture).
    The first call fixes the batch size N (outputs and counters are allocated once; a call with another N raises).
    Observation normalisation uses VecNormalize statistics: frozen ones given here, or live ones kept by a
    `upkie_amd.normalize.RunningNormalizer` it is attached to (`attach`). Build with `from_modules` or
    `from_sb3_state_dict`; after an optimiser step on those modules, `update_from` re-packs on the device.

    Asymmetric actor-critic ("privileged observations"): a critic whose first layer takes another number of inputs than
    the actor's (or ``asymmetric=True`` for one of the same width) reads a row of its own, ``critic_obs`` ``[N, Dc]``,
    normalised with statistics of its own (``critic_obs_mean`` / ``critic_obs_var``, or a second `RunningNormalizer`
    attached with ``tower="critic"``): ``act(obs, critic_obs=...)``, ``value(critic_obs)``,
    ``bootstrap_time_limits(final_critic_obs, ...)``. `mean_action` and everything else of the actor are unchanged; the
    observation normalisation switch and ``clip_obs`` are shared by both towers. `from_sb3_state_dict` stays symmetric."""

    asymmetric = False  # (set per object by __init__: whether the critic reads a row of its own)

    def __init__(self, actor_weights, actor_biases, critic_weights, critic_biases, log_std, activation: str, action_low=None,
                 action_high=None, obs_mean=None, obs_var=None, clip_obs: float = 10.0, eps: float = 1e-8, seed: int = 0, device=None,
                 critic_obs_mean=None, critic_obs_var=None, asymmetric: bool = False):
        critic_weights, critic_biases = list(critic_weights or []), list(critic_biases or [])
        shape = mlp_shape([tuple(w.shape) for w in actor_weights], [tuple(w.shape) for w in critic_weights], activation,
                          any(v is not None for v in (obs_mean, obs_var, critic_obs_mean, critic_obs_var)), clip_obs)
        if asymmetric and not shape.critic_obs_dim:
            shape = asymmetric_shape(shape)
        if not shape.critic_obs_dim and (critic_obs_mean is not None or critic_obs_var is not None):
            raise ValueError(f"critic_obs_mean / critic_obs_var are an asymmetric policy's: this critic reads the actor's "
                             f"{shape.obs_dim}-word observation (asymmetric=True gives it a row of its own)")
        for w, b in zip(list(actor_weights) + critic_weights, list(actor_biases) + critic_biases):
            if tuple(b.shape) != (w.shape[0],):
                raise ValueError(f"bias of shape {tuple(b.shape)} for a weight of shape {tuple(w.shape)}")
        if len(actor_biases) != len(actor_weights) or len(critic_biases) != len(critic_weights):
            raise ValueError("one bias per weight")
        self.device = torch.device(device) if device is not None else actor_weights[0].device
        if self.device.type != "cuda":
            raise UpkieRuntimeError("MlpActorCritic runs on the HIP device only (there is no CPU fallback): give device='cuda:0'")
        D, A, Dc = shape.obs_dim, shape.act_dim, int(shape.critic_obs_dim)
        self.shape = shape
        self.asymmetric = Dc > 0
        self.critic_obs_dim = Dc if Dc else int(D)  # (words of the row the critic reads)
        self.activation = activation
        self.clip_obs, self.eps = float(clip_obs), float(eps)
        self._lib = lib.load()
        lib.require(self._lib, "upkie_mlp_actor_critic_asym" if self.asymmetric else "upkie_mlp_actor_critic")
        words = int(self._lib.upkie_mlp_packed_words(C.byref(shape)))
        check(words)
        self._launcher = launcher(self.device)

        def vec(v, n, fill, name):
            t = torch.full((n,), fill, dtype=torch.float64) if v is None else torch.as_tensor(v, dtype=torch.float64).detach().cpu().reshape(-1)
            if t.numel() != n:
                raise ValueError(f"{name} needs {n} values")
            return t

        mean = vec(obs_mean, D, 0.0, "obs_mean")
        std = torch.sqrt(vec(obs_var, D, 1.0, "obs_var") + self.eps)  # (fp64, as VecNormalize)
        low = vec(action_low, A, float("-inf"), "action_low")
        high = vec(action_high, A, float("inf"), "action_high")
        if bool((low > high).any()):
            raise ValueError("action_low must not exceed action_high")
        f32 = dict(dtype=torch.float32, device=self.device)
        self._fixed = [mean.to(**f32), std.to(**f32), low.to(**f32), high.to(**f32)]
        if self.asymmetric:  # (the critic's statistics block: after action_high, before log_std)
            cstd = torch.sqrt(vec(critic_obs_var, Dc, 1.0, "critic_obs_var") + self.eps)
            self._fixed += [vec(critic_obs_mean, Dc, 0.0, "critic_obs_mean").to(**f32), cstd.to(**f32)]
        self.action_low, self.action_high = self._fixed[2], self._fixed[3]
        self._params = None
        self._set_params(actor_weights, actor_biases, critic_weights, critic_biases, log_std)
        sizes = [t.numel() for t in self.sources()]
        index = pack_index(shape, sizes)
        if index.size != words:
            raise UpkieRuntimeError(f"packed layout of {index.size} words here, {words} in the library: rebuild it")
        self._index = torch.as_tensor(index, device=self.device)
        self.packed = torch.empty(words, **f32)
        self._zero = torch.zeros(1, **f32)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.calls = None  # [N] int32 words read as uint32 call counters by the kernel
        self._out = {}
        self.update_from()

    # ---- construction
    @classmethod
    def from_modules(cls, actor, critic, log_std, action_low, action_high, obs_mean=None, obs_var=None, clip_obs: float = 10.0,
                     eps: float = 1e-8, seed: int = 0, device=None, critic_obs_mean=None, critic_obs_var=None, asymmetric: bool = False):
        """``actor``: nn.Sequential(Linear, act, ..., Linear) to the action mean; ``critic``: the same to one value (or
        None); ``log_std``: [act_dim] tensor; act is Tanh or ReLU, the same in both. The modules stay referenced:
        `update_from()` re-packs their current parameters. A critic with another input width than the actor's (or
        ``asymmetric=True``) makes the policy asymmetric; ``critic_obs_mean`` / ``critic_obs_var`` are its statistics."""
        aw, ab, act = _linear_stack(actor, "actor")
        cw, cb, cact = ([], [], None) if critic is None else _linear_stack(critic, "critic")
        if act is not None and cact is not None and act != cact:
            raise ValueError("one activation for both towers")
        self = cls(aw, ab, cw, cb, log_std, act or cact or "tanh", action_low, action_high, obs_mean, obs_var, clip_obs, eps, seed,
                   device if device is not None else aw[0].device, critic_obs_mean, critic_obs_var, asymmetric)
        self._modules = (actor, critic, log_std)
        return self

    @classmethod
    def from_sb3_state_dict(cls, state_dict, activation: str, action_space, obs_mean=None, obs_var=None, clip_obs: float = 10.0,
                            eps: float = 1e-8, seed: int = 0, device="cuda:0"):
        """From the ``state_dict()`` of Stable-Baselines3's ``ActorCriticPolicy`` (MlpPolicy, separate networks):
        ``mlp_extractor.policy_net.{0,2,..}``, ``mlp_extractor.value_net.{0,2,..}``, ``action_net``, ``value_net``,
        ``log_std``. ``action_space``: a Box (``.low`` / ``.high``) or a ``(low, high)`` pair. SB3 is not imported;
        ``activation`` ("tanh" or "relu") is the ``activation_fn`` the policy was built with (not in the state dict)."""
        aw, ab, cw, cb, log_std = sb3_parameters(state_dict)
        low, high = (action_space.low, action_space.high) if hasattr(action_space, "low") else action_space
        dev = torch.device(device)
        f = lambda ts: [torch.as_tensor(t, dtype=torch.float32).to(dev) for t in ts]  # noqa: E731
        return cls(f(aw), f(ab), f(cw), f(cb), f([log_std])[0], activation, low, high,
                   obs_mean, obs_var, clip_obs, eps, seed, dev)

    # ---- parameters
    def _set_params(self, aw, ab, cw, cb, log_std):
        A = self.shape.act_dim
        log_std = torch.as_tensor(log_std)
        if log_std.numel() != A:
            raise ValueError(f"log_std needs {A} values")
        params = []
        for w, b in zip(list(aw) + list(cw), list(ab) + list(cb)):
            params += [w, b]
        params.append(log_std)
        if self._params is not None and [tuple(p.shape) for p in params[:-1]] != [tuple(p.shape) for p in self._params[:-1]]:
            raise ValueError("update_from: the networks' shapes changed (build a new policy)")
        self._params = params

    def sources(self):
        """The tensors the packed buffer is gathered from, in `pack_index` order: obs_mean, obs_std, action_low,
        action_high, (an asymmetric policy: critic_obs_mean, critic_obs_std,) log_std, then (weight, bias) per layer of
        the actor (head last) and of the critic. The first `n_fixed` are never trained."""
        p = self._params
        return self._fixed + [p[-1]] + p[:-1]

    @property
    def n_fixed(self) -> int:
        """How many of `sources()` are fixed (statistics and action bounds): 4, or 6 for an asymmetric policy."""
        return len(self._fixed)

    def critic_stats_offset(self) -> int:
        """First word of critic_obs_mean in the packed buffer of an asymmetric policy (critic_obs_std follows it at the
        width rounded up to 4): what a critic normaliser hands to ``upkie_vecnorm_step`` as ``packed_stats``."""
        if not self.asymmetric:
            raise UpkieRuntimeError("a symmetric policy has no critic statistics block")
        return 2 * ((int(self.shape.obs_dim) + 3) // 4 * 4) + 2 * 16 * _tiles(self.shape.act_dim)

    def update_from(self, actor=None, critic=None, log_std=None) -> None:
        """Re-pack the weights -- of the given modules, or of the ones the policy was built from (`from_modules`),
        after an optimiser step on them -- with torch ops on the device: one gather into the packed buffer in place
        (captured graphs keep reading it), no host synchronisation."""
        if actor is not None or critic is not None or log_std is not None:
            mods = getattr(self, "_modules", (None, None, None))
            actor = actor if actor is not None else mods[0]
            critic = critic if critic is not None else mods[1]
            log_std = log_std if log_std is not None else mods[2]
            if actor is None or log_std is None:
                raise ValueError("update_from needs the actor and log_std (the policy was not built from modules)")
            aw, ab, _ = _linear_stack(actor, "actor")
            cw, cb, _ = ([], [], None) if critic is None else _linear_stack(critic, "critic")
            self._set_params(aw, ab, cw, cb, log_std)
            self._modules = (actor, critic, log_std)
        flat = [t.detach().reshape(-1).to(device=self.device, dtype=torch.float32) for t in self.sources()]
        torch.index_select(torch.cat(flat + [self._zero]), 0, self._index, out=self.packed)

    def unpack(self):
        """The source tensors (`sources()` order, flattened) read back from the packed buffer."""
        sizes = [t.numel() for t in self.sources()]
        flat = torch.zeros(sum(sizes) + 1, dtype=torch.float32, device=self.device)
        flat[self._index] = self.packed
        return list(torch.split(flat[:-1], sizes))

    def reseed(self, seed: Optional[int] = None) -> None:
        """Reset every env's call counter (and set a new seed): the draws start over."""
        if seed is not None:
            self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        if self.calls is not None:
            self.calls.zero_()

    def state_tensors(self) -> dict:
        """The packed weights and the per-env call counters of the noise (None before the first call): what `Ppo.save`
        carries."""
        return {"packed": self.packed, "calls": self.calls}

    # ---- calls
    def _obs(self, obs: torch.Tensor, critic: bool = False) -> torch.Tensor:
        words, what = (self.critic_obs_dim, "critic observations") if critic else (int(self.shape.obs_dim), "observations")
        if not isinstance(obs, torch.Tensor) or not obs.is_cuda:
            raise UpkieRuntimeError(f"MlpActorCritic runs on the HIP device only (there is no CPU fallback): {what} must be device tensors")
        if obs.device != self.device:
            raise ValueError(f"{what} on {obs.device}, policy on {self.device}")
        if obs.dim() < 1 or obs.shape[0] < 1 or obs[0].numel() != words:
            raise ValueError(f"{what} must be [N, ...] with {words} words per env, got {tuple(obs.shape)}")
        if obs.dtype is not torch.float32 or not obs.is_contiguous():
            obs = obs.to(torch.float32).contiguous()
        return obs

    def _buffers(self, n: int):
        """The persistent outputs and per-env call counters, allocated by the first call: a policy serves ONE batch
        size, so that they are never reallocated under a captured graph and the random stream never restarts behind
        the caller's back (another N: build another policy)."""
        if self._out.get("n") != n:
            if self._out:
                raise ValueError(f"this policy serves batches of {self._out['n']} envs (its outputs and call counters are sized by "
                                 f"the first call); build another policy for {n}")
            f32 = dict(dtype=torch.float32, device=self.device)
            A = self.shape.act_dim
            self._out = {"n": n, "env_action": torch.empty((n, A), **f32), "action": torch.empty((n, A), **f32),
                         "value": torch.empty(n, **f32), "log_prob": torch.empty(n, **f32)}
            self.calls = torch.zeros(n, dtype=torch.int32, device=self.device)
        return self._out

    def _check_out(self, name: str, t: torch.Tensor, n: int) -> torch.Tensor:
        words = {"norm_obs": self.shape.obs_dim, "norm_critic_obs": self.critic_obs_dim, "value": 1, "log_prob": 1}.get(name, self.shape.act_dim) * n
        names = ASYM_OUTPUT_NAMES if self.asymmetric else OUTPUT_NAMES
        if name not in names:
            raise ValueError(f"unknown output {name!r} (one of {names})")
        if not isinstance(t, torch.Tensor) or t.device != self.device or t.dtype is not torch.float32 or not t.is_contiguous() or t.numel() != words:
            raise ValueError(f"out[{name!r}] must be a contiguous float32 tensor of {words} words on {self.device}")
        return t

    def _launch(self, obs, deterministic: bool, outs: dict, critic_obs=None) -> None:
        """One launch: the symmetric entry point, or for an asymmetric policy the one that also takes the critic's rows
        (``obs`` None: the critic alone; the actor's pointer is then the critic's rows, which no wave reads)."""
        if not self.asymmetric:
            self._launcher(self._lib.upkie_mlp_actor_critic, obs.shape[0], C.byref(self.shape), self.packed.data_ptr(), obs.data_ptr(),
                           self.calls.data_ptr(), self.seed, int(bool(deterministic)), *[ptr(outs.get(name)) for name in OUTPUT_NAMES])
            return
        rows = obs if obs is not None else critic_obs
        self._launcher(self._lib.upkie_mlp_actor_critic_asym, rows.shape[0], C.byref(self.shape), self.packed.data_ptr(), rows.data_ptr(),
                       ptr(critic_obs), ptr(self.calls), self.seed, int(bool(deterministic)), *[ptr(outs.get(name)) for name in ASYM_OUTPUT_NAMES])

    def _critic_rows(self, critic_obs, n=None):
        """The critic's rows of an asymmetric policy, checked (``n``: the actor's batch)."""
        if critic_obs is None:
            raise ValueError(f"this policy is asymmetric: its critic reads rows of {self.critic_obs_dim} words of its own, the actor "
                             f"{int(self.shape.obs_dim)}; give critic_obs=")
        critic_obs = self._obs(critic_obs, critic=True)
        if n is not None and critic_obs.shape[0] != n:
            raise ValueError(f"{n} observations but {critic_obs.shape[0]} critic observations")
        return critic_obs

    def act(self, obs: torch.Tensor, deterministic: bool = False, out: Optional[dict] = None, critic_obs: Optional[torch.Tensor] = None):
        """(env_action, action, value, log_prob) of a batch of observations ``[N, ...]``; value is None without a
        critic. ``out``: tensors to write instead of the persistent buffers (any of `OUTPUT_NAMES`; "norm_obs" and
        "mean" are written only when given). An asymmetric policy also takes ``critic_obs`` ``[N, Dc]``, the rows its
        critic reads, and may write "norm_critic_obs"."""
        obs = self._obs(obs)
        n = obs.shape[0]
        if self.asymmetric:
            critic_obs = self._critic_rows(critic_obs, n)
        elif critic_obs is not None:
            raise ValueError(f"this policy is symmetric: its critic reads the actor's {int(self.shape.obs_dim)}-word observation, not a "
                             f"critic_obs of {critic_obs[0].numel()} words")
        outs = dict(self._buffers(n))
        del outs["n"]
        if self.shape.critic_layers == 0:
            outs["value"] = None
        for name, t in (out or {}).items():
            outs[name] = self._check_out(name, t, n)
        self._launch(obs, deterministic, outs, critic_obs)
        return outs["env_action"], outs["action"], outs["value"], outs["log_prob"]

    def mean_action(self, obs: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        """The deterministic action (the Gaussian's mean, clamped to the action bounds) of a batch of ANY size into the
        caller's ``out`` ``[N, act_dim]``, which is returned: bit for bit the ``env_action`` of ``act(obs,
        deterministic=True)``. The launch is handed no call counters and writes nothing but ``out``: neither the
        persistent output buffers nor `calls` are touched (or allocated), so a policy that trains on one batch size can
        be evaluated on an env of another (`upkie_amd.evaluation`) without a bit of its training changing."""
        obs = self._obs(obs)
        out = self._check_out("env_action", out, obs.shape[0])
        if self.asymmetric:  # (the actor alone: no critic rows, no counters)
            self._launcher(self._lib.upkie_mlp_actor_critic_asym, obs.shape[0], C.byref(self.shape), self.packed.data_ptr(), obs.data_ptr(), None,
                           None, self.seed, 1, None, None, None, None, out.data_ptr(), None, None)
            return out
        self._launcher(self._lib.upkie_mlp_actor_critic, obs.shape[0], C.byref(self.shape), self.packed.data_ptr(), obs.data_ptr(), None, self.seed, 1,
                       None, None, None, out.data_ptr(), None, None)
        return out

    def mean(self, obs: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        """The Gaussian's mean, NOT clamped to the action bounds, of a batch of any size into the caller's ``out``
        ``[N, act_dim]``, which is returned: a teacher's label (`upkie_amd.distill`). Like `mean_action` the launch is
        handed no call counters and writes nothing but ``out``."""
        obs = self._obs(obs)
        out = self._check_out("mean", out, obs.shape[0])
        if self.asymmetric:
            self._launcher(self._lib.upkie_mlp_actor_critic_asym, obs.shape[0], C.byref(self.shape), self.packed.data_ptr(), obs.data_ptr(), None,
                           None, self.seed, 1, None, None, out.data_ptr(), None, None, None, None)
            return out
        self._launcher(self._lib.upkie_mlp_actor_critic, obs.shape[0], C.byref(self.shape), self.packed.data_ptr(), obs.data_ptr(), None, self.seed, 1,
                       None, out.data_ptr(), None, None, None, None)
        return out

    def act_actor(self, obs: torch.Tensor, deterministic: bool = False, out: Optional[dict] = None):
        """`act` without the critic (no value output, so its wave returns at once, and an asymmetric policy needs no
        ``critic_obs``): returns ``(env_action, action, log_prob)``. The noise counters advance as in `act`."""
        obs = self._obs(obs)
        n = obs.shape[0]
        outs = dict(self._buffers(n))
        del outs["n"], outs["value"]
        for name, t in (out or {}).items():
            if name == "value":
                raise ValueError("act_actor does not run the critic: no value output")
            outs[name] = self._check_out(name, t, n)
        self._launch(obs, deterministic, outs, None)
        return outs["env_action"], outs["action"], outs["log_prob"]

    def value(self, obs: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The critic alone (e.g. the bootstrap values of the observations after a rollout's last step). An asymmetric
        policy takes the critic's rows ``[N, Dc]``."""
        if self.shape.critic_layers == 0:
            raise UpkieRuntimeError("this policy has no critic")
        obs = self._obs(obs, critic=self.asymmetric)
        n = obs.shape[0]
        v = self._buffers(n)["value"] if out is None else self._check_out("value", out, n)
        if self.asymmetric:
            self._launch(None, True, {"value": v}, critic_obs=obs)
        else:
            self._launch(obs, True, {"value": v})
        return v

    def bootstrap_time_limits(self, final_obs: torch.Tensor, terminated: torch.Tensor, truncated: torch.Tensor, reward: torch.Tensor,
                              gamma: float) -> torch.Tensor:
        """Stable-Baselines3's time-limit bootstrap (``collect_rollouts``), one launch: for every env with
        ``truncated & ~terminated``, ``reward += gamma * value(final_obs)`` in float32 (two roundings, no fused
        multiply-add), in place; returns ``reward``. The value is the critic's on ``final_obs`` normalised with the
        policy's current statistics, bit for bit what `value` gives for the same rows. ``final_obs`` ``[N, ...]`` float32
        (an env's ``info["final_obs"]``), ``terminated`` / ``truncated`` ``[N]`` bool or uint8, ``reward`` a contiguous
        ``[N]`` float32 device tensor (e.g. ``buffer.rewards[t]``). No host synchronisation: it can be captured in a
        graph.

        Order inside a rollout step, as in SB3 (Monitor under VecNormalize):
        1. ``policy.act``; 2. ``env.step``; 3. the user's reward; 4. `upkie_amd.episodes.EpisodeStatistics.step` on
        the raw reward; 5. `RunningNormalizer.step` into ``buffer.rewards[t]``; 6. this, on the normalised slot
        ``buffer.rewards[t]`` with ``buffer.gamma``. SB3's semantics assume same-step autoreset (``final_obs``: the
        observation the ended episode stopped in)."""
        if self.shape.critic_layers == 0:
            raise UpkieRuntimeError("this policy has no critic: the time-limit bootstrap needs V(final_obs)")
        final_obs = self._obs(final_obs, critic=self.asymmetric)  # (only the critic runs: an asymmetric policy's final critic rows)
        n = final_obs.shape[0]
        flags = []
        for name, t in (("terminated", terminated), ("truncated", truncated)):
            if (not isinstance(t, torch.Tensor) or t.device != self.device or t.dtype not in (torch.bool, torch.uint8) or not t.is_contiguous()
                    or t.numel() != n):
                raise ValueError(f"{name} must be a contiguous bool or uint8 tensor of {n} values on {self.device}")
            flags.append(t)
        if (not isinstance(reward, torch.Tensor) or reward.device != self.device or reward.dtype is not torch.float32 or not reward.is_contiguous()
                or reward.numel() != n):
            raise ValueError(f"reward must be a contiguous float32 tensor of {n} values on {self.device} (it is updated in place)")
        gamma = float(gamma)
        if not 0.0 <= gamma <= 1.0:
            raise ValueError("gamma must be in [0, 1]")
        lib.require(self._lib, "upkie_mlp_bootstrap_time_limits")
        self._launcher(self._lib.upkie_mlp_bootstrap_time_limits, n, C.byref(self.shape), self.packed.data_ptr(), final_obs.data_ptr(),
                       flags[0].data_ptr(), flags[1].data_ptr(), gamma, reward.data_ptr())
        return reward


class MlpPolicy(MlpActorCritic):
    """The actor of `MlpActorCritic` alone, deterministic (the Gaussian's mean, clamped to the action bounds):
    ``policy(obs)`` returns the ``[N, act_dim]`` env action, like `LinearPolicy`, for ``env.step(policy(obs))``."""

    @classmethod
    def from_modules(cls, actor, action_low=None, action_high=None, obs_mean=None, obs_var=None, clip_obs: float = 10.0, eps: float = 1e-8,
                     device=None):
        aw = _linear_stack(actor, "actor")[0]
        log_std = torch.zeros(aw[-1].shape[0], device=aw[-1].device)
        return super().from_modules(actor, None, log_std, action_low, action_high, obs_mean, obs_var, clip_obs, eps, 0, device)

    def __call__(self, obs: torch.Tensor) -> torch.Tensor:
        obs = self._obs(obs)
        env_action = self._buffers(obs.shape[0])["env_action"]
        self._launch(obs, True, {"env_action": env_action})
        return env_action
