"""The learner half of PPO on the device: Stable-Baselines3's ``PPO.train`` for an `MlpActorCritic`, every epoch and
minibatch as HIP launches (csrc/ppo.hpp) that update the policy's packed weight buffer in place -- the buffer its
rollout kernel reads, so captured rollout graphs pick up the new weights with no re-pack and no host synchronisation.
include/upkie_hip.h states the arithmetic (SB3's, restated there)."""

import ctypes as C
import math
from typing import Callable, Optional, Union

import torch

from . import abi, lib
from .agent_step import AgentStep
from .exceptions import UpkieRuntimeError
from .launch import check, launcher, ptr
from .on_policy import OnPolicyDriver

STAT_NAMES = ("policy_gradient_loss", "value_loss", "entropy_loss", "loss", "approx_kl", "clip_fraction", "grad_norm")
MIRROR_STAT_NAMES = STAT_NAMES + ("mirror_loss",)  # the statistics row of a trainer with ``symmetry``
Schedule = Union[float, Callable[[float], float]]  # a constant, or SB3's schedule: a function of progress_remaining (1 -> 0)


def _at(schedule, progress: float) -> Optional[float]:
    """The value of a schedule (a callable of progress_remaining, a number, or None) at `progress`."""
    if schedule is None:
        return None
    return float(schedule(progress)) if callable(schedule) else float(schedule)


def trainable_offset(shape) -> int:
    """First trainable word of the packed buffer (csrc/policy_mlp.hpp): log_std's. The words before it -- obs_mean,
    obs_std, action_low, action_high and an asymmetric shape's critic_obs_mean, critic_obs_std -- are never written by
    the update; from it on every word is a parameter (log_std, the towers' weights and biases) or padding, which stays
    zero."""
    at = 16 * ((int(shape.act_dim) + 15) // 16)
    return 2 * ((int(shape.obs_dim) + 3) // 4 * 4) + 2 * at + 2 * ((int(getattr(shape, "critic_obs_dim", 0)) + 3) // 4 * 4)


class PackedTrainerState:
    """What the trainers of an `MlpActorCritic`'s packed buffer share (`PpoTrainer`, `upkie_amd.distill.DistillTrainer`):
    Adam's moments ``m`` and ``v`` in the packed layout, the seeded device ``generator`` of the epochs' permutations and
    the index buffer they are drawn into (`_allocate`, `shuffle`), the write-back of the trained words into the tensors
    the policy was built from, and the conversion between the packed layout of the moments and lists in
    ``policy.sources()`` order. ``_sizes`` holds the element counts of ``policy.sources()``, ``_flat``
    ``sum(_sizes) + 1`` float32 words on the device. The learning rate and Adam's step count are per class: their device
    words live where the class's launches read them."""

    def __init__(self, policy, seed: int):
        self.policy = policy
        self.device = policy.device
        self._lib = lib.load()
        self._launcher = launcher(self.device)
        f32 = dict(dtype=torch.float32, device=self.device)
        self.m = torch.zeros(policy.packed.numel(), **f32)
        self.v = torch.zeros(policy.packed.numel(), **f32)
        self.generator = torch.Generator(device=self.device)
        self.generator.manual_seed(int(seed))
        self._sizes = [t.numel() for t in policy.sources()]
        self._flat = torch.zeros(sum(self._sizes) + 1, **f32)  # (sync_modules' scatter target)
        self._total = None

    def _allocate(self, total: int) -> bool:
        """Size the minibatches and the index buffer for ``total`` samples (the first call; one size per trainer). False
        when they are sized already; the caller then allocates nothing either."""
        if self._total == total:
            return False
        if self._total is not None:
            raise ValueError(f"this trainer serves {self._total} samples (its buffers are sized by the first call); build another for {total}")
        self._mb = min(self.batch_size, total)
        self.n_minibatches = (total + self._mb - 1) // self._mb
        self.perm = torch.empty((self.n_epochs, total), dtype=torch.int32, device=self.device)
        self._total = total
        return True

    def shuffle(self) -> None:
        """One ``randperm`` per epoch into the persistent index buffer (outside any capture)."""
        if self._total is None:
            raise UpkieRuntimeError("call prepare() first (it sizes the buffers)")
        for e in range(self.n_epochs):
            self.perm[e].copy_(torch.randperm(self._total, generator=self.generator, device=self.device))

    def sync_modules(self) -> None:
        """Write the packed weights back into the tensors the policy was built from (the modules' parameters, or the
        tensors of `from_sb3_state_dict`): one scatter on the device, then a copy per tensor. The fixed sources
        (observation statistics, action bounds) are not written."""
        pol = self.policy
        self._flat.index_copy_(0, pol._index, pol.packed)  # (padding words, all mapped to the last slot, are zero)
        params = pol._params
        trainable = [params[-1]] + params[:-1]  # sources() order after the fixed tensors
        nf = getattr(pol, "n_fixed", 4)
        start = sum(self._sizes[:nf])
        with torch.no_grad():
            for t, n in zip(trainable, self._sizes[nf:]):
                t.detach().view(-1).copy_(self._flat[start:start + n])
                start += n

    def _unpack(self, packed: torch.Tensor):
        flat = torch.zeros(sum(self._sizes) + 1, dtype=torch.float32, device=self.device)
        flat.index_copy_(0, self.policy._index, packed)
        return [t.clone() for t in torch.split(flat[:-1], self._sizes)[getattr(self.policy, "n_fixed", 4):]]

    def _pack(self, tensors, into: torch.Tensor) -> None:
        nf = getattr(self.policy, "n_fixed", 4)
        if len(tensors) != len(self._sizes) - nf:
            raise ValueError(f"need {len(self._sizes) - nf} tensors (log_std, then weight and bias per layer)")
        flat = [torch.zeros(n, dtype=torch.float32, device=self.device) for n in self._sizes[:nf]]
        for t, n in zip(tensors, self._sizes[nf:]):
            t = torch.as_tensor(t, dtype=torch.float32).to(self.device).reshape(-1)
            if t.numel() != n:
                raise ValueError(f"a tensor of {t.numel()} values where {n} belong")
            flat.append(t)
        torch.index_select(torch.cat(flat + [torch.zeros(1, dtype=torch.float32, device=self.device)]), 0, self.policy._index, out=into)


class PpoTrainer(PackedTrainerState):
    """``train(buffer)`` runs ``n_epochs`` epochs of minibatches of ``batch_size`` samples over a full `RolloutBuffer`
    (after ``compute_returns_and_advantage``): per epoch one ``randperm`` of the ``T N`` samples (a ``torch.Generator``
    on the device seeded with ``seed``), one launch for the advantage statistics of its minibatches, then per minibatch
    gradient, clip_grad_norm_ and Adam (three launches). It returns the device tensor ``[n_epochs, n_minibatches, 7]`` of
    `STAT_NAMES` without reading it back, and (``sync=True``) writes the trained weights back into the modules or tensors
    the policy was built from (`sync_modules`), so that a later ``policy.update_from()`` does not revert them.

    Graph capture: ``train`` is ``prepare(buffer); update(buffer)``. `prepare` stays OUTSIDE a capture: it copies the
    buffer's advantages and returns into the trainer's own tensors (``compute_returns_and_advantage`` allocates new ones
    on every call, so a captured launch must not read the buffer's) and draws the epochs' ``randperm`` into the trainer's
    index buffer. `update(buffer)` -- every epoch and minibatch, and the write-back -- reads those, and the buffer's
    observations, actions, values and log-probs, which a `RolloutBuffer` allocates once; its launch arguments are
    constant from one iteration to the next (the step count, lr and counters live in device memory) and it allocates
    nothing. So a caller may capture ``update(buffer)`` once and replay it every iteration, calling ``prepare(buffer)``
    after ``compute_returns_and_advantage`` and before each replay. A trainer serves ONE buffer: `prepare` refuses
    another, whose tensors a captured update would not read.

    An asymmetric policy (its critic reads rows of its own: `MlpActorCritic`) trains from a buffer built with
    ``critic_obs_shape=(Dc,)``: the gradient launch reads ``buffer.critic_observations`` for the critic
    (``upkie_ppo_minibatch_update_asym`` / ``upkie_ppo_minibatch_gradient_asym``); ``obs_normalized`` then says that BOTH
    tensors hold normalised rows. A symmetric policy issues exactly the launches it always did.

    Speed: with [64, 64] towers an update is several times faster than the same SB3 minibatch as torch ops. With
    256-unit layers the gradient launch spills registers and runs few blocks, and the update is many times SLOWER than
    torch (21.6 x at [256, 256] and 131072 samples: DESIGN.md section 6); prefer a torch learner there.

    ``obs_normalized``: the buffer holds normalised observations (the rollout wrote ``norm_obs``); otherwise the
    training forward normalises them as ``act()`` does. With a live `RunningNormalizer` attached to the policy the
    statistics moved during the rollout, so raw observations are refused (SB3 trains on the normalised ones too).
    Adam's ``m`` and ``v`` live in the packed layout; `state_dict` gives them in ``policy.sources()`` order.

    ``process_group``: data-parallel PPO over a ``torch.distributed`` group. Each rank holds a policy replica and a
    `RolloutBuffer` of its own envs, all of the same size; together they train as ONE learner on the union of the
    samples: minibatch j of the union is the union of the ranks' minibatches j, and every rank holds the same weights, m,
    v and step count, bit for bit, after every minibatch. Per epoch the advantage statistics take two exchanges of
    per-minibatch sums; per minibatch this rank's gradient and loss sums go to a slot, one collective makes every slot
    visible on every rank (`upkie_amd.distributed.SlotExchange`), and every rank sums them in rank order, then clips
    and steps Adam (``upkie_ppo_minibatch_gradient`` / ``upkie_ppo_minibatch_apply``). `prepare` checks, collectively,
    that every rank has the same sample count; `broadcast_parameters` makes the replicas start identical. With a group
    of one rank the results are the same bits as without a group. An update with a group cannot be captured in a graph.
    Give each rank's policy its own seed (e.g. ``seed + rank``): its noise is keyed by the local env index.

    Schedules and ``target_kl`` (the controlled form): ``lr``, ``clip_range`` and ``clip_range_vf`` may be callables of
    SB3's ``progress_remaining`` (1 at the start of training, 0 at its end), evaluated on the host by
    `set_progress`, and ``target_kl`` ends an update at the first minibatch whose ``approx_kl > 1.5 * target_kl``,
    before that minibatch's optimiser step, as SB3 does. With any of these (or ``controlled=True``) the trainer takes
    the ``*_controlled`` entry points: the values live in a control block in device memory (`control`, whose first two
    words are `scalars`), the stop is decided on the device, and the launches of the minibatches after it return at
    once and leave NaN statistics rows. A captured `update` therefore stays valid across `set_progress`,
    `set_clip_range`, `set_target_kl` and across iterations that stop at different minibatches. Without them the
    trainer issues exactly the launches it always did. With a process group every rank takes the same decision from
    the same exchanged bits; the collectives of the minibatches after a stop still run (the host cannot see the flag
    without a synchronisation) and change nothing. `log` returns SB3's ``train/*`` record with one device-to-host copy.

    ``symmetry`` (a `upkie_amd.symmetry.MirrorSymmetry`): every minibatch goes through
    ``upkie_ppo_minibatch_update_mirror`` -- each sample next to its mirrored partner in the gradient launch (twice the
    tiles of the plain update through the same towers), the partners' surrogate and value terms in the loss when
    ``augment``, and ``mirror_coef`` times the mirror loss. The statistics are then ``[n_epochs, n_minibatches, 8]``
    (`MIRROR_STAT_NAMES`: ``mirror_loss`` last), ``approx_kl`` and ``clip_fraction`` run over the originals alone, so
    ``target_kl`` means what it means in SB3, and `log` gains ``mirror_loss``. With ``obs_normalized`` the mirror acts on
    the stored normalised rows (`upkie_amd.symmetry`). The tables are validated on the host and written to the device
    once, here. A ``process_group`` with ``symmetry`` is refused: the ranks' slots would need the mirror loss's sum.
    ``symmetry=None`` issues exactly the launches and bits it always did."""

    asymmetric = False  # (set per object by __init__: whether the policy's critic reads rows of its own)
    symmetry, _mirror, stat_names = None, None, STAT_NAMES  # (set per object by __init__: the mirrored form)

    def __init__(self, policy, lr: Schedule = 3e-4, n_epochs: int = 10, batch_size: int = 64, clip_range: Schedule = 0.2,
                 clip_range_vf: Optional[Schedule] = None, normalize_advantage: bool = True, ent_coef: float = 0.0, vf_coef: float = 0.5,
                 max_grad_norm: float = 0.5, obs_normalized: bool = False, seed: int = 0, process_group=None,
                 target_kl: Optional[float] = None, controlled: Optional[bool] = None, symmetry=None):
        from .policies import MlpActorCritic

        if not isinstance(policy, MlpActorCritic):
            raise TypeError("PpoTrainer trains an MlpActorCritic")
        if int(policy.shape.critic_layers) < 1:
            raise ValueError("PPO needs a critic: the policy has none")
        if int(n_epochs) < 1 or int(batch_size) < 1:
            raise ValueError("n_epochs and batch_size must be positive")
        if symmetry is not None:
            from .symmetry import MirrorSymmetry

            if not isinstance(symmetry, MirrorSymmetry):
                raise TypeError("symmetry must be a upkie_amd.symmetry.MirrorSymmetry (or None)")
            if process_group is not None:
                raise ValueError("symmetry with a process_group is not supported: the ranks' slots carry four loss sums and the mirror "
                                 "loss needs a fifth (train with symmetry on one rank, or without it on several)")
            symmetry.check_shape(policy.shape)
        self.symmetry = symmetry
        self.stat_names = STAT_NAMES if symmetry is None else MIRROR_STAT_NAMES
        self._schedules = {"lr": lr, "clip_range": clip_range, "clip_range_vf": clip_range_vf}
        self.progress_remaining = 1.0
        lr, clip_range, clip_range_vf = (_at(x, 1.0) for x in (lr, clip_range, clip_range_vf))
        if not clip_range > 0.0 or not max_grad_norm > 0.0:
            raise ValueError("clip_range and max_grad_norm must be positive")
        if clip_range_vf is not None and not clip_range_vf > 0.0:
            raise ValueError("clip_range_vf must be positive (or None)")
        if target_kl is not None and not (float(target_kl) > 0.0 and math.isfinite(float(target_kl))):
            raise ValueError("target_kl must be positive and finite (or None)")
        uses = target_kl is not None or any(callable(x) for x in self._schedules.values())
        if controlled is not None and not controlled and uses:
            raise ValueError("target_kl and schedules need the controlled form (leave controlled unset)")
        self.controlled = uses if controlled is None else bool(controlled)
        self._clip_range, self._clip_range_vf = clip_range, clip_range_vf
        self._target_kl = float(target_kl) if target_kl is not None else None
        super().__init__(policy, seed)
        self.n_epochs, self.batch_size = int(n_epochs), int(batch_size)
        self.normalize_advantage = bool(normalize_advantage)
        self.obs_normalized = bool(obs_normalized)
        cfg = abi.UpkiePpoConfig()
        cfg.clip_range, cfg.clip_range_vf = float(clip_range), float(clip_range_vf) if clip_range_vf is not None else 0.0
        cfg.ent_coef, cfg.vf_coef, cfg.max_grad_norm = float(ent_coef), float(vf_coef), float(max_grad_norm)
        cfg.adam_beta1, cfg.adam_beta2, cfg.adam_eps = 0.9, 0.999, 1e-5  # (torch.optim.Adam as SB3 builds it: eps 1e-5)
        cfg.obs_normalized = int(self.obs_normalized)
        self.config = cfg
        lib.require(self._lib, "upkie_ppo_minibatch_update")
        self.asymmetric = bool(getattr(policy, "asymmetric", False))
        if self.asymmetric:
            lib.require(self._lib, "upkie_ppo_minibatch_update_asym", "for an asymmetric policy")
        if self.controlled:
            lib.require(self._lib, "upkie_ppo_minibatch_update_controlled", "for target_kl and schedules")
        # the control block (include/upkie_hip.h: UPKIE_PPO_CTRL_*); `scalars` (lr, t) is its first two words
        self.control = torch.zeros(abi.PPO_CTRL_WORDS, dtype=torch.float64, device=self.device)
        self.control[abi.PPO_CTRL_LR] = float(lr)
        self.scalars = self.control[:2]
        self._lr = float(lr)
        if self.controlled:
            self._write_control(float(lr))
        self._mirror = None
        if symmetry is not None:
            self._mirror = self._mirror_tables(symmetry)
        self._values = None  # (the buffer's value tensor: explained_variance reads it)
        self._log_words = torch.zeros(2, dtype=torch.float64, device=self.device)  # explained variance, std
        self._ev_exchange = None
        self._buffer = None  # (addresses of the buffer's observations, actions, values and log-probs)
        self.process_group = process_group
        self._grad_exchange = self._adv_exchange = None
        if process_group is not None:
            from .distributed import SlotExchange

            lib.require(self._lib, "upkie_ppo_minibatch_apply", "for a process group")
            self._grad_exchange = SlotExchange(int(self._lib.upkie_ppo_slot_bytes(C.byref(policy.shape))) // 4, self.device, process_group)
            self._ev_exchange = SlotExchange(8, self.device, process_group)  # (4 doubles per rank)

    def _mirror_tables(self, symmetry) -> abi.UpkiePpoMirror:
        """The library's own validation of the tables (host), then their one copy to the device; the struct every
        mirrored minibatch launch is given."""
        lb, shape = self._lib, self.policy.shape
        lib.require(lb, "upkie_ppo_minibatch_update_mirror", "for symmetry")
        words = int(lb.upkie_ppo_mirror_words(C.byref(shape)))
        check(words)
        self.mirror_tables = torch.zeros(words, dtype=torch.int32, device=self.device)
        host = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        sym = symmetry
        self._launcher(lb.upkie_ppo_mirror_set, C.byref(shape), host(sym.obs_index), host(sym.obs_sign), host(sym.critic_index), host(sym.critic_sign),
                       host(sym.act_index), host(sym.act_sign), ptr(self.mirror_tables))
        mirror = abi.UpkiePpoMirror()
        mirror.augment, mirror.mirror_coef, mirror.tables = int(sym.augment), float(sym.mirror_coef), self.mirror_tables.data_ptr()
        return mirror

    # ---- buffers, allocated by the first train() (one rollout size per trainer)
    def _allocate(self, total: int) -> None:
        if not super()._allocate(total):
            return
        mb = self._mb
        workspace_bytes = self._lib.upkie_ppo_workspace_bytes if self._mirror is None else self._lib.upkie_ppo_mirror_workspace_bytes
        nbytes = int(workspace_bytes(C.byref(self.policy.shape), mb))
        check(nbytes)
        self.workspace = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
        self.adv_stats = torch.zeros((self.n_epochs, self.n_minibatches, 2), dtype=torch.float64, device=self.device)
        self.stats = torch.zeros((self.n_epochs, self.n_minibatches, len(self.stat_names)), dtype=torch.float32, device=self.device)
        self.advantages = torch.zeros(total, dtype=torch.float32, device=self.device)  # (fixed addresses: what update() reads)
        self.returns = torch.zeros(total, dtype=torch.float32, device=self.device)
        if self.process_group is not None:
            from .distributed import SlotExchange

            self._adv_exchange = SlotExchange(int(self._lib.upkie_ppo_advantage_slot_bytes(total, mb)) // 4, self.device, self.process_group)

    def _check_buffer(self, buffer):
        if buffer.advantages is None:
            raise UpkieRuntimeError("call buffer.compute_returns_and_advantage() first")
        if buffer.device != self.device:
            raise ValueError(f"the buffer is on {buffer.device}, the policy on {self.device}")
        D, A = int(self.policy.shape.obs_dim), int(self.policy.shape.act_dim)
        total = buffer.buffer_size * buffer.n_envs
        if buffer.observations[0, 0].numel() != D or buffer.actions[0, 0].numel() != A:
            raise ValueError(f"the buffer holds {buffer.observations[0, 0].numel()} observation and {buffer.actions[0, 0].numel()} action "
                             f"words per sample, the policy takes {D} and {A}")
        critic_rows = getattr(buffer, "critic_observations", None)
        Dc = int(getattr(self.policy, "critic_obs_dim", D))
        if self.asymmetric and critic_rows is None:
            raise ValueError(f"the policy is asymmetric (its critic reads {Dc} words, its actor {D}) but the buffer holds no "
                             f"critic_observations: build it with critic_obs_shape=({Dc},)")
        if not self.asymmetric and critic_rows is not None:
            raise ValueError(f"the buffer holds critic_observations of {critic_rows[0, 0].numel()} words but the policy is symmetric (its "
                             f"critic reads the actor's {D}-word observation)")
        if self.asymmetric and critic_rows[0, 0].numel() != Dc:
            raise ValueError(f"the buffer holds {critic_rows[0, 0].numel()} critic observation words per sample, the policy's critic takes {Dc}")
        if self.asymmetric and (critic_rows.dtype is not torch.float32 or not critic_rows.is_contiguous()):
            raise ValueError("the buffer's tensors must be contiguous float32")
        live = getattr(self.policy, "_normalizer", None) is not None or getattr(self.policy, "_critic_normalizer", None) is not None
        if not self.obs_normalized and live:
            raise UpkieRuntimeError("the policy reads a live RunningNormalizer: its statistics moved during the rollout, so train on the "
                                    "normalised observations the rollout stored (act(out={'norm_obs': ...})) with obs_normalized=True")
        for t in (buffer.observations, buffer.actions, buffer.values, buffer.log_probs, buffer.advantages, buffer.returns):
            if t.dtype is not torch.float32 or not t.is_contiguous():
                raise ValueError("the buffer's tensors must be contiguous float32")
        return total

    @staticmethod
    def _addresses(buffer):
        tensors = (buffer.observations, buffer.actions, buffer.values, buffer.log_probs, getattr(buffer, "critic_observations", None))
        return tuple(t.data_ptr() for t in tensors if t is not None)

    # ---- training
    def prepare(self, buffer) -> None:
        """Outside any capture, after ``buffer.compute_returns_and_advantage``: copy the buffer's advantages and returns
        into the trainer's own tensors and draw this iteration's permutations (`shuffle`)."""
        total = self._check_buffer(buffer)
        if self.process_group is not None:
            self._check_ranks(total)
        self._allocate(total)
        if self._buffer is None:
            self._buffer = self._addresses(buffer)
        elif self._addresses(buffer) != self._buffer:
            raise ValueError("this trainer serves one rollout buffer (a captured update reads its tensors): build another trainer")
        self._values = buffer.values
        self.advantages.copy_(buffer.advantages.reshape(total))
        self.returns.copy_(buffer.returns.reshape(total))
        self.shuffle()

    def _check_ranks(self, total: int) -> None:
        """Every rank the same sample count and minibatch count (one learner on the union needs minibatches of the same
        size on every rank). Collective: every rank sends its sizes and every rank raises when any differ."""
        from .distributed import all_gather_ints

        mb = min(self.batch_size, total)
        sizes = all_gather_ints([total, (total + mb - 1) // mb], self.process_group, self.device)
        if any(s != sizes[0] for s in sizes):
            raise ValueError(f"every rank of the process group must hold the same number of samples and minibatches; (samples, minibatches) "
                             f"by rank: {[tuple(s) for s in sizes]} (uneven shards are not supported)")

    def broadcast_parameters(self, src: int = 0) -> None:
        """Copy group rank `src`'s trainable packed words, Adam's m and v, lr and t to every rank, so that the replicas
        start identical however they were built; then `sync_modules`. A collective: every rank calls it."""
        if self.process_group is None:
            return
        from .distributed import broadcast_tensor_

        off = trainable_offset(self.policy.shape)
        trainable = self.policy.packed[off:]
        for t in (trainable, self.m, self.v, self.scalars):
            broadcast_tensor_(t, src, self.process_group)
        self._lr = None
        self.sync_modules()

    def update(self, buffer, sync: bool = True) -> torch.Tensor:
        """Every epoch and minibatch on the current permutations (no randperm, no allocation, no host synchronisation:
        capturable), then `sync_modules` when ``sync``. Reads the advantages and returns of the last `prepare`."""
        total = self._check_buffer(buffer)
        if self._buffer is None:
            raise UpkieRuntimeError("call prepare(buffer) first: it copies the advantages and returns update() reads")
        if self._addresses(buffer) != self._buffer:
            raise ValueError("this trainer serves one rollout buffer (a captured update reads its tensors): build another trainer")
        if self.process_group is not None and torch.cuda.is_current_stream_capturing():
            raise UpkieRuntimeError("a PpoTrainer with a process group cannot be captured in a graph (every minibatch exchanges the "
                                    "gradients through a collective)")
        mb = self._mb
        # what every minibatch launch begins with, and the six sample arrays it reads
        head = (C.byref(self.policy.shape), C.byref(self.config))
        data = tuple(ptr(t) for t in (buffer.observations, buffer.actions, buffer.values, buffer.log_probs, self.advantages, self.returns))
        if self.asymmetric:  # (the critic's rows go after obs)
            data = data[:1] + (ptr(buffer.critic_observations),) + data[1:]
        with torch.cuda.device(self.device):  # (around the whole block: every launch takes the launcher's fast path, and the collectives rely on it)
            if self.controlled:
                self._launcher(self._lib.upkie_ppo_update_begin, ptr(self.control))
            for e in range(self.n_epochs):
                perm = ptr(self.perm[e])
                self._advantage_stats(e, total, perm, data[-2])
                for j in range(self.n_minibatches):
                    start = j * mb
                    self._minibatch(e, j, head, total, start, min(mb, total - start), perm, data)
        if sync:
            self.sync_modules()
        return self.stats

    def _advantage_stats(self, e: int, total: int, perm, adv) -> None:
        """Epoch ``e``'s per-minibatch advantage statistics: one launch, or with a process group two exchanges of
        per-minibatch sums (the means, then the squared deviations) and the finish."""
        lb, launch, ax, norm, out = self._lib, self._launcher, self._adv_exchange, int(self.normalize_advantage), ptr(self.adv_stats[e])
        if ax is None:
            launch(lb.upkie_ppo_advantage_stats, total, self._mb, perm, adv, norm, out)
            return
        launch(lb.upkie_ppo_advantage_partials, total, self._mb, perm, adv, 0, None, ax.world, ptr(ax.mine))
        ax.exchange()
        launch(lb.upkie_ppo_advantage_partials, total, self._mb, perm, adv, 1, ptr(ax.slots), ax.world, ptr(ax.mine))
        ax.exchange()
        launch(lb.upkie_ppo_advantage_finish, total, self._mb, norm, ptr(ax.slots), ax.world, out)

    def _minibatch(self, e: int, j: int, head, total: int, start: int, size: int, perm, data) -> None:
        """Minibatch ``j`` of epoch ``e``: gradient, clip and Adam in one launch, or with a process group the gradient
        half, the exchange of the ranks' slots and the apply half. The controlled entry points have the plain ones'
        signatures with the control block where ``adam_scalars`` is (the fused one), after it (the gradient half), and
        with ``minibatch_start`` first (the apply half)."""
        lb, launch, gx, ctl, mb = self._lib, self._launcher, self._grad_exchange, self.controlled, self._mb
        adv_stats, packed, work, stats = ptr(self.adv_stats[e, j]), ptr(self.policy.packed), ptr(self.workspace), ptr(self.stats[e, j])
        if self._mirror is not None:  # (one entry point: a nullable critic_obs after obs, a nullable control block)
            rows = data if self.asymmetric else data[:1] + (None,) + data[1:]
            launch(lb.upkie_ppo_minibatch_update_mirror, *head, C.byref(self._mirror), total, start, size, mb, perm, *rows, adv_stats, packed,
                   ptr(self.m), ptr(self.v), ptr(self.scalars), ptr(self.control) if ctl else None, work, stats)
            return
        if self.asymmetric:  # (one entry point per half serves the plain and the controlled form: a nullable control block)
            control = ptr(self.control) if ctl else None
            if gx is None:
                launch(lb.upkie_ppo_minibatch_update_asym, *head, total, start, size, mb, perm, *data, adv_stats, packed, ptr(self.m), ptr(self.v),
                       ptr(self.scalars), control, work, stats)
                return
            launch(lb.upkie_ppo_minibatch_gradient_asym, *head, total, start, size, gx.world * size, mb, perm, *data, adv_stats, packed, work,
                   ptr(gx.mine), control)
            gx.exchange()
            launch(lb.upkie_ppo_minibatch_apply_controlled if ctl else lb.upkie_ppo_minibatch_apply, *head, *((start,) if ctl else ()), gx.world * size,
                   mb, ptr(gx.slots), gx.world, packed, ptr(self.m), ptr(self.v), ptr(self.control if ctl else self.scalars), work, stats)
            return
        if gx is None:
            launch(lb.upkie_ppo_minibatch_update_controlled if ctl else lb.upkie_ppo_minibatch_update, *head, total, start, size, mb, perm, *data,
                   adv_stats, packed, ptr(self.m), ptr(self.v), ptr(self.control), work, stats)
            return
        W = gx.world
        launch(lb.upkie_ppo_minibatch_gradient_controlled if ctl else lb.upkie_ppo_minibatch_gradient, *head, total, start, size, W * size, mb, perm,
               *data, adv_stats, packed, work, ptr(gx.mine), *((ptr(self.control),) if ctl else ()))
        gx.exchange()  # (after a stop: still a collective every rank joins; the apply half ignores it)
        launch(lb.upkie_ppo_minibatch_apply_controlled if ctl else lb.upkie_ppo_minibatch_apply, *head, *((start,) if ctl else ()), W * size, mb,
               ptr(gx.slots), W, packed, ptr(self.m), ptr(self.v), ptr(self.control if ctl else self.scalars), work, stats)

    def train(self, buffer, sync: bool = True) -> torch.Tensor:
        """`prepare` then `update`: SB3's ``PPO.train`` on one full rollout buffer. Returns ``[n_epochs, n_minibatches, 7]``
        (`STAT_NAMES`), on the device."""
        self.prepare(buffer)
        return self.update(buffer, sync)

    def set_lr(self, lr: float) -> None:
        """Write the learning rate (a device word: a captured update reads the new value)."""
        self.scalars[0].fill_(float(lr))
        self._lr = float(lr)

    # ---- the control block (schedules, target_kl)
    def _need_control(self, what: str) -> None:
        if not self.controlled:
            raise UpkieRuntimeError(f"{what} needs the controlled form: build the trainer with target_kl, a schedule or controlled=True "
                                    "(its update then reads the control block)")

    def _write_control(self, lr: float) -> None:
        """lr, clip_range, clip_range_vf and target_kl to the control block (one launch; outside any capture)."""
        if torch.cuda.is_current_stream_capturing():
            raise UpkieRuntimeError("set the schedules' values outside a graph capture (a captured write would replay its old value)")
        self._launcher(self._lib.upkie_ppo_control_set, self.control.data_ptr(), float(lr), float(self._clip_range),
                       float(self._clip_range_vf or 0.0), float(self._target_kl or 0.0))
        self._lr = float(lr)

    def set_progress(self, progress_remaining: float) -> None:
        """SB3's ``_update_current_progress_remaining`` + ``_update_learning_rate``: evaluate the callables among ``lr``,
        ``clip_range`` and ``clip_range_vf`` at ``progress_remaining`` on the host and write the words a captured update
        reads. Constants stay as they are (a `set_lr` / `set_clip_range` value included)."""
        progress = float(progress_remaining)
        self.progress_remaining = progress
        sch = self._schedules
        if not any(callable(x) for x in sch.values()):
            return
        self._need_control("a schedule")
        lr = _at(sch["lr"], progress) if callable(sch["lr"]) else None
        if callable(sch["clip_range"]):
            self._clip_range = _at(sch["clip_range"], progress)
        if callable(sch["clip_range_vf"]):
            self._clip_range_vf = _at(sch["clip_range_vf"], progress)
        self._write_control(self._current_lr() if lr is None else lr)

    def _current_lr(self) -> float:
        if self._lr is None:  # (the word came from another rank: read it once)
            self._lr = float(self.scalars[0].item())
        return self._lr

    def set_clip_range(self, clip_range: float, clip_range_vf: Optional[float] = None) -> None:
        """Write ``clip_range`` (and ``clip_range_vf``; None: no value clipping) for the next update."""
        self._need_control("set_clip_range")
        if not float(clip_range) > 0.0 or (clip_range_vf is not None and not float(clip_range_vf) > 0.0):
            raise ValueError("clip_range and clip_range_vf must be positive")
        self._clip_range, self._clip_range_vf = float(clip_range), None if clip_range_vf is None else float(clip_range_vf)
        self._write_control(self._current_lr())

    def set_target_kl(self, target_kl: Optional[float]) -> None:
        """Write ``target_kl`` for the next update; None switches the early stop off."""
        self._need_control("set_target_kl")
        if target_kl is not None and not (float(target_kl) > 0.0 and math.isfinite(float(target_kl))):
            raise ValueError("target_kl must be positive and finite (or None)")
        self._target_kl = None if target_kl is None else float(target_kl)
        self._write_control(self._current_lr())

    def explained_variance(self) -> torch.Tensor:
        """SB3's ``explained_variance(values, returns)`` of the last `prepare`'s rollout (fp64, one launch, a device word;
        with a process group over every rank's samples: two exchanges, so every rank calls it)."""
        if self._values is None:
            raise UpkieRuntimeError("call prepare(buffer) first")
        lib.require(self._lib, "upkie_ppo_explained_variance")
        lb, ret, val, out, ex = self._lib, self.returns.data_ptr(), self._values.data_ptr(), self._log_words.data_ptr(), self._ev_exchange
        with torch.cuda.device(self.device):  # (around the whole block: the collectives between the launches rely on it)
            if ex is None:
                steps = [(-1, None, 1, None)]
            else:
                steps = [(0, None, ex.world, ex.mine.data_ptr()), (1, ex.slots.data_ptr(), ex.world, ex.mine.data_ptr()),
                         (2, ex.slots.data_ptr(), ex.world, None)]
            for phase, slots, world, mine in steps:
                self._launcher(lb.upkie_ppo_explained_variance, self._total, ret, val, phase, slots, world, mine, out)
                if phase in (0, 1):
                    ex.exchange()
        return self._log_words[0]

    def log(self) -> dict:
        """SB3's ``train/*`` record of the last update, with ONE device-to-host copy: the seven `STAT_NAMES` averaged over
        the minibatches that ran (NaN rows, those after an early stop, excluded; SB3 logs ``np.mean`` over every minibatch
        of the update for each, ``approx_kl`` and ``clip_fraction`` included), ``explained_variance``, ``std``
        (``exp(log_std).mean()``), ``n_updates``, ``clip_range``, ``clip_range_vf`` when set, ``learning_rate`` and
        ``early_stopped_at``: the (epoch, minibatch) whose ``approx_kl`` ended the update, or None."""
        if self._total is None:
            raise UpkieRuntimeError("call train(buffer) first")
        self.explained_variance()
        off, A = trainable_offset(self.policy.shape), int(self.policy.shape.act_dim)
        torch.mean(torch.exp(self.policy.packed[off:off + A]).double(), dim=0, out=self._log_words[1])
        host = torch.cat([self.stats.reshape(-1).double(), self.control, self._log_words]).cpu().numpy()  # the one copy
        n = self.stats.numel()
        rows, ctrl, words = host[:n].reshape(-1, len(self.stat_names)), host[n:n + abi.PPO_CTRL_WORDS], host[n + abi.PPO_CTRL_WORDS:]
        ran = rows[~(rows != rows).any(axis=1)]
        record = {name: float(ran[:, k].mean()) if len(ran) else math.nan for k, name in enumerate(self.stat_names)}
        stopped = self.controlled and ctrl[abi.PPO_CTRL_STOPPED] != 0.0
        record.update(explained_variance=float(words[0]), std=float(words[1]), n_updates=self._n_updates(ctrl),
                      clip_range=float(ctrl[abi.PPO_CTRL_CLIP_RANGE]) if self.controlled else float(self._clip_range),
                      learning_rate=float(ctrl[abi.PPO_CTRL_LR]),
                      early_stopped_at=divmod(int(ctrl[abi.PPO_CTRL_MINIBATCHES_RUN]) - 1, self.n_minibatches) if stopped else None)
        if self._clip_range_vf is not None:
            record["clip_range_vf"] = float(ctrl[abi.PPO_CTRL_CLIP_RANGE_VF]) if self.controlled else float(self._clip_range_vf)
        return record

    def _n_updates(self, ctrl) -> int:
        """SB3's ``_n_updates``: the control block counts the epochs entered; without it every epoch of every update ran,
        so it is the step count over the minibatches per epoch."""
        if self.controlled:
            return int(ctrl[abi.PPO_CTRL_N_UPDATES])
        return int(ctrl[abi.PPO_CTRL_T]) // self.n_minibatches if self._total is not None else 0

    # ---- state
    def state_tensors(self) -> dict:
        """Adam's moments and the control block (what `Ppo.save` carries)."""
        return {"m": self.m, "v": self.v, "control": self.control}

    def host_state(self) -> dict:
        """The host's copies of what the control block holds: the values the setters and the schedules wrote last."""
        return {"clip_range": self._clip_range, "clip_range_vf": self._clip_range_vf, "target_kl": self._target_kl, "lr": self._current_lr()}

    def load_host_state(self, state: dict, progress_remaining: float) -> None:
        """`host_state` of a saved run, and where its schedules stood (the control block itself is a tensor)."""
        self._clip_range, self._clip_range_vf, self._target_kl, self._lr = (state[k] for k in ("clip_range", "clip_range_vf", "target_kl", "lr"))
        self.progress_remaining = progress_remaining

    def state_dict(self) -> dict:
        """Adam's state: ``m`` and ``v`` as lists in ``policy.sources()`` order of the trainable tensors (log_std, then
        weight and bias per layer of the actor and of the critic), the step count ``t``, ``lr`` and ``n_updates`` (SB3's
        ``_n_updates``: the epochs entered)."""
        ctrl = self.control.cpu().numpy()
        return {"m": self._unpack(self.m), "v": self._unpack(self.v), "t": int(ctrl[abi.PPO_CTRL_T]), "lr": float(ctrl[abi.PPO_CTRL_LR]),
                "n_updates": self._n_updates(ctrl)}

    def load_state_dict(self, sd: dict) -> None:
        self._pack(sd["m"], self.m)
        self._pack(sd["v"], self.v)
        self.scalars.copy_(torch.tensor([float(sd["lr"]), float(sd["t"])], dtype=torch.float64))
        self.control[abi.PPO_CTRL_N_UPDATES] = float(sd.get("n_updates", 0))
        self._lr = float(sd["lr"])


class Ppo(OnPolicyDriver):
    """Stable-Baselines3's ``PPO(...).learn(...)`` on the device: the driver that owns the `RolloutBuffer`, the
    `RunningNormalizer` (``normalize``), the `EpisodeStatistics`, the `PpoTrainer` and the rollout's `GraphedLoop`, and
    runs them in the order examples/ppo_mlp_train_time_limits.py establishes. One rollout step is: store the episode
    starts; ``policy.act`` (normalised observation, action, value and log-prob straight into the buffer); the env's step
    and the reward (``reward_fn``, ``reward`` or the env's own) as `upkie_amd.agent_step` states them; ``episodes.step``
    on the raw reward; the pipeline's observation (same module); ``normalizer.step`` (normalised reward and the next
    episode starts); the time-limit bootstrap
    (``bootstrap_time_limits``). With ``graph=True`` an iteration is two graph replays (the ``n_steps`` rollout steps,
    the update) around GAE and ``trainer.prepare``; capturing the rollout runs ONE real warm-up step first, as
    `GraphedLoop` does, which is not counted in ``num_timesteps``. With a ``process_group`` (data-parallel: every rank
    its own env, policy replica and `Ppo`) nothing is captured, because the normaliser and the update exchange slots
    through collectives; ``num_timesteps`` then counts this rank's steps.

    `learn` (`upkie_amd.on_policy.OnPolicyDriver`, shared with `Distillation`) follows ``OnPolicyAlgorithm.learn``: ``num_timesteps += n_envs`` per step; after each rollout
    ``progress_remaining = 1 - num_timesteps / total_timesteps`` goes to the trainer's schedules (`set_progress`) BEFORE
    the update; every ``log_interval`` iterations one `PpoTrainer.log` (one device-to-host copy) plus
    ``rollout/ep_rew_mean``, ``rollout/ep_len_mean``, ``time/total_timesteps`` and ``time/iterations`` make a record,
    appended to ``records`` and given to ``callback(model, record)`` (called every iteration, ``record`` None off the
    interval; with ``reward`` it also carries ``rollout/ep_rew_<name>_mean`` of every term); a callback that returns False ends training, as SB3's does. ``learning_rate``, ``clip_range`` and
    ``clip_range_vf`` take floats or callables of ``progress_remaining``; ``target_kl`` as SB3.

    `save` / `load` carry everything the next iteration reads -- packed weights, Adam's moments and control block, the
    trainer's generator, the policy's per-env noise counters, the normaliser, the episode statistics, the reward's state (``reward.*``, when one is given), the episode events' (``events.*``: counters, force, inertial records), the episode
    starts, the counters and the env (the simulation's state block, its observation and step outputs) -- so a run
    resumed in fresh objects continues bit for bit. Schedules, ``reward_fn``, ``reward`` and ``events`` are code: give them to `load` again.

    ``events`` (a `upkie_amd.events.EpisodeEvents` built on ``env``) perturbs the rollout: random pushes and per-episode
    inertias, one more launch per step, after the reward (`AgentStep`). Built with a ``curriculum`` (`PushLevels`) every
    env carries a push difficulty level, decided in that same launch from the env's own episodes: nothing to reduce, so
    it runs under a ``process_group`` as it is; a record then carries ``rollout/push_level_mean`` and
    ``rollout/push_level_top_frac``, and with ``live`` ``rollout/push_prob`` and ``rollout/push_norm_high`` (read once
    per record, outside the rollout). A callback's ``events.set_push(...)`` is followed by the captured rollout.

    ``critic_observation`` (a `upkie_amd.privileged.PrivilegedObservation` built on ``env``, ``events`` and ``pipeline``)
    trains an asymmetric ``policy``: the critic reads the privileged row, the actor what the robot will see. One more
    launch per step after `AgentStep.apply` (so after ``events.step``); the row is normalised by a second
    `RunningNormalizer` (``critic_normalizer``, ``norm_reward=False``, attached with ``tower="critic"``; its return
    statistics are unused) into ``buffer.critic_observations``; the time-limit bootstrap reads the row's
    ``final_observation`` and ``last_values`` the current row. `save` / `load` carry ``critic_observation.*`` and the
    critic's normaliser. Evaluation never runs the critic and takes such a policy unchanged.

    ``targets`` (a `upkie_amd.targets.TaskTargets` built on ``env``) trains a goal-conditioned policy: one more launch per
    step right after ``env.step`` (`AgentStep`) appends the env's target to the raw observation, so ``policy`` (or
    ``pipeline``) reads D + G words, ``reward`` is built with ``obs_dim = D + G`` (a tracking term taps ``obs(D + g)``)
    and scores the step under the target the policy was given, and a ``critic_observation`` is built with
    ``obs_dim=D + G``. Without a pipeline the normaliser has D + G columns. With a `TargetCurriculum` one launch after
    every rollout widens the ranges from the named reward term's episode sums (it must be one of ``reward``'s; with a
    ``process_group`` it is refused); a record carries ``rollout/target_<name>_low`` and ``_high``. `save` / `load`
    carry ``targets.*``, the ranges included. ``targets=None``: every launch and every bit as without.

    ``symmetry`` (a `upkie_amd.symmetry.MirrorSymmetry` of the words the POLICY reads: `MirrorSymmetry.gyropod(targets)` for
    a Gyropod env with targets, ``.for_pipeline(pipeline)`` behind a pipeline) adds the robot's left/right symmetry to the
    update, as rsl_rl's ``symmetry_cfg`` does: mirrored samples join every minibatch (``augment``) and ``mirror_coef``
    weighs the mirror loss (`PpoTrainer`). The rollout does not change; the update's graph holds the mirrored launches; a
    record gains ``train/mirror_loss``. With ``normalize`` the mirror acts on the normalised rows the rollout stored: a
    sign-flipped word with a non-zero running mean is slightly off. Symmetry is code, like a schedule: give it to `load`
    again. With a ``process_group`` it is refused. ``symmetry=None``: every launch and every bit as without.

    A ``policy`` that arrives with a live `RunningNormalizer` and has been called (a student of
    `upkie_amd.distill.Distillation`) keeps that normaliser: with ``normalize`` the run goes on under the statistics the
    policy was fitted under, on an env of the same size and with the same ``gamma`` (another size or ``gamma`` is refused).
    The hand-over is for symmetric training: with ``critic_observation=`` it is refused, because the critic's rows would need
    a second normaliser and a policy that has been called cannot be attached to one."""

    def __init__(self, env, policy, n_steps: int = 128, gamma: float = 0.99, gae_lambda: float = 0.95, n_epochs: int = 10, batch_size: int = 64,
                 learning_rate: Schedule = 3e-4, clip_range: Schedule = 0.2, clip_range_vf: Optional[Schedule] = None,
                 normalize_advantage: bool = True, ent_coef: float = 0.0, vf_coef: float = 0.5, max_grad_norm: float = 0.5,
                 target_kl: Optional[float] = None, normalize: bool = True, bootstrap_time_limits: bool = True, stats_window_size: int = 100,
                 reward_fn: Optional[Callable] = None, graph: bool = True, seed: int = 0, process_group=None, pipeline=None, reward=None,
                 events=None, critic_observation=None, targets=None, symmetry=None):
        if int(n_steps) < 1:
            raise ValueError("n_steps must be positive")
        if symmetry is not None and process_group is not None:
            raise ValueError("symmetry with a process_group is not supported: the ranks' slots carry four loss sums and the mirror "
                             "loss needs a fifth (train with symmetry on one rank, or without it on several)")
        curriculum = getattr(targets, "curriculum", None)
        if curriculum is not None and process_group is not None:
            raise ValueError("a TargetCurriculum with a process_group is not supported: every rank would widen its own ranges from its own "
                             "envs' scores and the ranks' ranges would part (targets without a curriculum shard: their draws are keyed by "
                             "global env ids)")
        if curriculum is not None and (reward is None or curriculum.term not in reward.names):
            raise ValueError(f"the curriculum reads the reward term {curriculum.term!r}, the reward has "
                             f"{list(reward.names) if reward is not None else 'no terms (give reward=, a RewardTerms)'}")
        self._curriculum_term = reward.names.index(curriculum.term) if curriculum is not None else None
        D = int(getattr(getattr(policy, "shape", None), "obs_dim", 0))
        Dc = int(getattr(policy, "critic_obs_dim", D))
        if getattr(policy, "asymmetric", False) and critic_observation is None:
            raise ValueError(f"the policy is asymmetric (its critic reads {Dc} words, its actor {D}): give critic_observation= (a "
                             f"PrivilegedObservation of {Dc} words)")
        if critic_observation is not None and not getattr(policy, "asymmetric", False):
            raise ValueError(f"critic_observation has {int(critic_observation.dim)} words but the policy is symmetric (its critic reads the "
                             f"actor's {D}-word observation): build the critic on {int(critic_observation.dim)} inputs")
        if critic_observation is not None and int(critic_observation.dim) != Dc:
            raise ValueError(f"critic_observation has {int(critic_observation.dim)} words, the policy's critic takes {Dc}")
        if critic_observation is not None and int(critic_observation.num_envs) != int(env.num_envs):
            raise ValueError(f"critic_observation serves {int(critic_observation.num_envs)} envs, the env has {int(env.num_envs)}")
        self.critic_observation = critic_observation
        self._agent = AgentStep(env, policy, pipeline, reward, reward_fn, noun="rollout", events=events, targets=targets)  # (checks the sizes)
        self.reward, self.pipeline, self.events, self.targets = reward, pipeline, events, targets
        self.env, self.policy = env, policy
        self.n_envs = int(env.num_envs)
        self.n_steps, self.gamma, self.gae_lambda = int(n_steps), float(gamma), float(gae_lambda)
        self.normalize, self.bootstrap, self.window = bool(normalize), bool(bootstrap_time_limits), int(stats_window_size)
        self.reward_fn, self.seed, self.process_group = reward_fn, int(seed), process_group
        self.graph = bool(graph) and process_group is None
        self._trainer_args = dict(lr=learning_rate, n_epochs=n_epochs, batch_size=batch_size, clip_range=clip_range, clip_range_vf=clip_range_vf,
                                  normalize_advantage=normalize_advantage, ent_coef=ent_coef, vf_coef=vf_coef, max_grad_norm=max_grad_norm,
                                  target_kl=target_kl, obs_normalized=self.normalize, seed=seed, process_group=process_group)
        if symmetry is not None:  # (a run without it builds its trainer with the arguments it always did)
            self._trainer_args["symmetry"] = symmetry
        self.symmetry = symmetry
        super().__init__()
        self.trainer = self.buffer = self.normalizer = self.critic_normalizer = self.episodes = None

    # ---- the objects, built by the first learn() (or by load())
    def _setup(self) -> None:
        if self.buffer is not None:
            return
        from .episodes import EpisodeStatistics
        from .normalize import RunningNormalizer
        from .rollout import RolloutBuffer

        env, pol, N, T = self.env, self.policy, self.n_envs, self.n_steps
        dev = self.device = env.device
        D, A = int(pol.shape.obs_dim), int(pol.shape.act_dim)
        if self.normalize:
            kw = {} if self.process_group is None else {"process_group": self.process_group}
            live = getattr(pol, "_normalizer", None)
            if live is not None and pol._out and self.process_group is None:
                # a policy handed over with its statistics (`upkie_amd.distill.Distillation` trained it under them; a policy
                # that has been called cannot be attached to new ones): training goes on under the same normaliser
                if self.critic_observation is not None:
                    raise ValueError("a policy that arrives with a live normaliser is taken over for symmetric training only: its critic's "
                                     "rows would need a second normaliser, and a policy that has been called cannot be attached to one "
                                     "(build a fresh policy from the trained modules for critic_observation=)")
                if int(live.num_envs) != N or float(live.gamma) != self.gamma:
                    raise ValueError(f"the policy's normaliser serves {int(live.num_envs)} envs at gamma {float(live.gamma)}, this run has {N} at "
                                     f"{self.gamma}: hand the policy over on an env of the same size, with the same gamma")
                self.normalizer = live
            else:
                self.normalizer = self._observation_normalizer(pol, **kw)
            if self.critic_observation is not None:  # (the privileged rows' own statistics; the reward is the first one's)
                self.critic_normalizer = RunningNormalizer(N, int(pol.critic_obs_dim), gamma=self.gamma, norm_reward=False, device=dev, **kw)
                self.critic_normalizer.attach(pol, tower="critic")
        self.episodes = EpisodeStatistics(N, window=self.window, device=dev)
        self.trainer = PpoTrainer(pol, **self._trainer_args)
        if self.process_group is not None:
            self.trainer.broadcast_parameters(0)
            if self.normalizer is not None:
                self.normalizer.broadcast_statistics(0)
            if self.critic_normalizer is not None:
                self.critic_normalizer.broadcast_statistics(0)
        cobs = self.critic_observation
        self.buffer = RolloutBuffer(T, N, obs_shape=(D,), action_shape=(A,), device=dev, gamma=self.gamma, gae_lambda=self.gae_lambda,
                                    critic_obs_shape=None if cobs is None else (int(cobs.dim),))
        self._agent.reset(seed=self.seed if self.process_group is None else None)
        if cobs is not None:
            cobs.reset(self._agent.raw_observation)  # (after the pipeline's and the events' resets: their first command, force and scales)
        if self.normalizer is not None:
            self.normalizer.reset(self._agent.observation)
        if self.critic_normalizer is not None:
            self.critic_normalizer.reset(cobs.observation)
        self._env_action = torch.empty(N, A, device=dev)
        self._starts = torch.ones(N, dtype=torch.uint8, device=dev)
        self._begin_rollouts()

    # the env's latest (raw) observation: the agent step's
    _obs = property(lambda self: self._agent.raw_observation, lambda self, obs: setattr(self._agent, "raw_observation", obs))

    def _rollout_step(self) -> None:
        """One step of every env into slot ``_slot``: `Ppo`'s own stages around the two halves of `AgentStep`. With an
        `AgentPipeline` the normaliser and the bootstrap see the stack and its terminal form."""
        t, buf, pol, starts, agent, cobs = self._slot, self.buffer, self.policy, self._starts, self._agent, self.critic_observation
        obs = agent.observation
        buf.episode_starts[t].copy_(starts)
        out = {"action": buf.actions[t], "value": buf.values[t], "log_prob": buf.log_probs[t], "env_action": self._env_action}
        if self.normalizer is not None:
            out["norm_obs"] = buf.observations[t]
        else:
            buf.observations[t].copy_(obs)
        if cobs is None:
            pol.act(obs, out=out)
        else:  # (the critic reads the privileged row; its normalised form is what the update trains on)
            if self.critic_normalizer is not None:
                out["norm_critic_obs"] = buf.critic_observations[t]
            else:
                buf.critic_observations[t].copy_(cobs.observation)
            pol.act(obs, out=out, critic_obs=cobs.observation)
        raw_next, reward, terminated, truncated, final_obs, _ = agent.apply(self._env_action)
        if cobs is not None:  # (after events.step: the force the next step applies, the next episode's scales)
            cobs.step(raw_next, terminated, truncated, final_obs=final_obs)
        self.episodes.step(reward, terminated, truncated)  # Monitor: the raw reward
        if self.bootstrap and final_obs is None:
            raise UpkieRuntimeError("bootstrap_time_limits needs info['final_obs'] (an env with autoreset_mode='same_step'); "
                                    "or build Ppo with bootstrap_time_limits=False")
        next_obs, final_obs = agent.observe()  # (what the normaliser and the bootstrap read)
        if self.normalizer is not None:
            self.normalizer.step(next_obs, reward, terminated, truncated, out={"reward": buf.rewards[t], "episode_starts": starts})
        else:
            buf.rewards[t].copy_(reward)
            torch.bitwise_or(terminated, truncated, out=starts)
        if self.critic_normalizer is not None:  # (the rows' statistics move as the observations' do; its returns are unused)
            self.critic_normalizer.step(cobs.observation, reward, terminated, truncated)
        if self.bootstrap:
            pol.bootstrap_time_limits(final_obs if cobs is None else cobs.final_observation, terminated, truncated, buf.rewards[t], self.gamma)
        self._advance_slot()

    def collect_rollouts(self) -> None:
        """``n_steps`` steps of every env into the buffer, then GAE (SB3's ``collect_rollouts``)."""
        super().collect_rollouts()
        buf = self.buffer
        buf.pos, buf.full = self.n_steps, True
        last = self._agent.observation if self.critic_observation is None else self.critic_observation.observation
        buf.compute_returns_and_advantage(last_values=self.policy.value(last), dones=self._starts)

    def train(self) -> None:
        """SB3's ``PPO.train`` on the collected rollout: `PpoTrainer.prepare`, then the update (a graph replay when
        ``graph``)."""
        tr = self.trainer
        tr.prepare(self.buffer)
        if not self.graph:
            tr.update(self.buffer)
        else:
            self._replay_update(lambda: tr.update(self.buffer), (self.policy.packed, tr.m, tr.v, tr.control, tr.stats))

    def _after_rollout(self) -> None:
        if self._curriculum_term is not None:  # (one launch: the ranges of the next rollout's draws)
            self.targets.curriculum_step(self.reward.term_last[self._curriculum_term], self.reward.finished)
        self.trainer.set_progress(self.progress_remaining)

    def _record(self) -> dict:
        record = {f"train/{k}": v for k, v in self.trainer.log().items()}
        record.update(self._rollout_record())
        if self.reward is not None:
            record.update({f"rollout/ep_rew_{name}_mean": mean for name, mean in self.reward.term_means().items()})
        if self.targets is not None:
            record.update({f"rollout/{name}": value for name, value in self.targets.log().items()})
        if hasattr(self.events, "log"):  # (a push curriculum's levels, live push settings; a plain stage adds nothing)
            record.update({f"rollout/{name}": value for name, value in self.events.log().items()})
        return record

    # ---- saving and loading
    # where a stage's `state_tensors` go under "tensors" in the file: stage -> (prefix, the names that differ from the stage's own)
    _FILE_NAMES = {"policy": ("", {}), "trainer": ("", {}), "episodes": ("", {"counters": "ep_counters", "means": "ep_means"}),
                   "pipeline": ("pipeline.", {}), "reward": ("reward.", {}), "events": ("events.", {}),
                   "critic_observation": ("critic_observation.", {}), "targets": ("targets.", {})}

    def _own_tensors(self) -> dict:
        return {"starts": self._starts}

    def _save_own(self, sd: dict) -> None:
        sd["trainer"] = self.trainer.host_state()
        if self.critic_normalizer is not None:  # (a run without a privileged critic writes the names it always did)
            sd["critic_normalizer"] = self.critic_normalizer.state_dict()

    def _restore_own(self, sd: dict) -> None:
        if self.critic_normalizer is not None:
            if sd.get("critic_normalizer") is None:
                raise ValueError("the file has no critic_normalizer: it was saved from a run without critic_observation")
            self.critic_normalizer.load_state_dict(sd["critic_normalizer"])
        self.trainer.load_host_state(sd["trainer"], self.progress_remaining)

    @classmethod
    def load(cls, path, env, policy, **kwargs):
        """A `Ppo` on fresh ``env`` and ``policy`` objects (same sizes, same keyword arguments as the saved one) that
        continues the saved run: ``learn(more, reset_num_timesteps=False)``."""
        return cls._load(path, env, policy, **kwargs)
