"""The learner half of PPO on the device: Stable-Baselines3's ``PPO.train`` for an `MlpActorCritic`, every epoch and
minibatch as HIP launches (csrc/ppo.hpp) that update the policy's packed weight buffer in place -- the buffer its
rollout kernel reads, so captured rollout graphs pick up the new weights with no re-pack and no host synchronisation.
include/upkie_hip.h states the arithmetic (SB3's, restated there)."""

import ctypes as C
from typing import Optional

import torch

from . import abi, lib
from .exceptions import UpkieRuntimeError

STAT_NAMES = ("policy_gradient_loss", "value_loss", "entropy_loss", "loss", "approx_kl", "clip_fraction", "grad_norm")


def trainable_offset(shape) -> int:
    """First trainable word of the packed buffer (csrc/policy_mlp.hpp): log_std's. The words before it -- obs_mean,
    obs_std, action_low, action_high -- are never written by the update; from it on every word is a parameter (log_std,
    the towers' weights and biases) or padding, which stays zero."""
    at = 16 * ((int(shape.act_dim) + 15) // 16)
    return 2 * ((int(shape.obs_dim) + 3) // 4 * 4) + 2 * at


class PpoTrainer:
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
    Give each rank's policy its own seed (e.g. ``seed + rank``): its noise is keyed by the local env index."""

    def __init__(self, policy, lr: float = 3e-4, n_epochs: int = 10, batch_size: int = 64, clip_range: float = 0.2,
                 clip_range_vf: Optional[float] = None, normalize_advantage: bool = True, ent_coef: float = 0.0, vf_coef: float = 0.5,
                 max_grad_norm: float = 0.5, obs_normalized: bool = False, seed: int = 0, process_group=None):
        from .policies import MlpActorCritic

        if not isinstance(policy, MlpActorCritic):
            raise TypeError("PpoTrainer trains an MlpActorCritic")
        if int(policy.shape.critic_layers) < 1:
            raise ValueError("PPO needs a critic: the policy has none")
        if int(n_epochs) < 1 or int(batch_size) < 1:
            raise ValueError("n_epochs and batch_size must be positive")
        if not clip_range > 0.0 or not max_grad_norm > 0.0:
            raise ValueError("clip_range and max_grad_norm must be positive")
        if clip_range_vf is not None and not clip_range_vf > 0.0:
            raise ValueError("clip_range_vf must be positive (or None)")
        self.policy = policy
        self.device = policy.device
        self.n_epochs, self.batch_size = int(n_epochs), int(batch_size)
        self.normalize_advantage = bool(normalize_advantage)
        self.obs_normalized = bool(obs_normalized)
        cfg = abi.UpkiePpoConfig()
        cfg.clip_range, cfg.clip_range_vf = float(clip_range), float(clip_range_vf) if clip_range_vf is not None else 0.0
        cfg.ent_coef, cfg.vf_coef, cfg.max_grad_norm = float(ent_coef), float(vf_coef), float(max_grad_norm)
        cfg.adam_beta1, cfg.adam_beta2, cfg.adam_eps = 0.9, 0.999, 1e-5  # (torch.optim.Adam as SB3 builds it: eps 1e-5)
        cfg.obs_normalized = int(self.obs_normalized)
        self.config = cfg
        self._lib = lib.load()
        if not hasattr(self._lib, "upkie_ppo_minibatch_update"):
            raise UpkieRuntimeError("this build of libupkie_hip.so has no upkie_ppo_minibatch_update")
        words = policy.packed.numel()
        f32 = dict(dtype=torch.float32, device=self.device)
        self.m = torch.zeros(words, **f32)
        self.v = torch.zeros(words, **f32)
        self.scalars = torch.tensor([float(lr), 0.0], dtype=torch.float64, device=self.device)  # lr, t
        self.generator = torch.Generator(device=self.device)
        self.generator.manual_seed(int(seed))
        self._total = None
        self._buffer = None  # (addresses of the buffer's observations, actions, values and log-probs)
        sizes = [t.numel() for t in policy.sources()]
        self._sizes = sizes
        self._flat = torch.zeros(sum(sizes) + 1, **f32)  # (sync_modules' scatter target)
        self.process_group = process_group
        self._grad_exchange = self._adv_exchange = None
        if process_group is not None:
            from .distributed import SlotExchange

            if not hasattr(self._lib, "upkie_ppo_minibatch_apply"):
                raise UpkieRuntimeError("this build of libupkie_hip.so has no upkie_ppo_minibatch_apply: rebuild it for a process group")
            self._grad_exchange = SlotExchange(int(self._lib.upkie_ppo_slot_bytes(C.byref(policy.shape))) // 4, self.device, process_group)

    # ---- buffers, allocated by the first train() (one rollout size per trainer)
    def _allocate(self, total: int) -> None:
        if self._total == total:
            return
        if self._total is not None:
            raise ValueError(f"this trainer serves rollouts of {self._total} samples (its buffers are sized by the first train()); "
                             f"build another for {total}")
        mb = min(self.batch_size, total)
        self.n_minibatches = (total + mb - 1) // mb
        nbytes = int(self._lib.upkie_ppo_workspace_bytes(C.byref(self.policy.shape), mb))
        if nbytes < 0:
            lib.check(nbytes, None)
        self.workspace = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
        self.perm = torch.empty((self.n_epochs, total), dtype=torch.int32, device=self.device)
        self.adv_stats = torch.zeros((self.n_epochs, self.n_minibatches, 2), dtype=torch.float64, device=self.device)
        self.stats = torch.zeros((self.n_epochs, self.n_minibatches, 7), dtype=torch.float32, device=self.device)
        self.advantages = torch.zeros(total, dtype=torch.float32, device=self.device)  # (fixed addresses: what update() reads)
        self.returns = torch.zeros(total, dtype=torch.float32, device=self.device)
        self._mb = mb
        self._total = total
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
        if not self.obs_normalized and getattr(self.policy, "_normalizer", None) is not None:
            raise UpkieRuntimeError("the policy reads a live RunningNormalizer: its statistics moved during the rollout, so train on the "
                                    "normalised observations the rollout stored (act(out={'norm_obs': ...})) with obs_normalized=True")
        for t in (buffer.observations, buffer.actions, buffer.values, buffer.log_probs, buffer.advantages, buffer.returns):
            if t.dtype is not torch.float32 or not t.is_contiguous():
                raise ValueError("the buffer's tensors must be contiguous float32")
        return total

    @staticmethod
    def _addresses(buffer):
        return tuple(t.data_ptr() for t in (buffer.observations, buffer.actions, buffer.values, buffer.log_probs))

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
        self.sync_modules()

    def shuffle(self) -> None:
        """One ``randperm`` per epoch into the persistent index buffer (outside any capture)."""
        if self._total is None:
            raise UpkieRuntimeError("call prepare(buffer) first (it sizes the buffers)")
        for e in range(self.n_epochs):
            self.perm[e].copy_(torch.randperm(self._total, generator=self.generator, device=self.device))

    def update(self, buffer, sync: bool = True) -> torch.Tensor:
        """Every epoch and minibatch on the current permutations (no randperm, no allocation, no host synchronisation:
        capturable), then `sync_modules` when ``sync``. Reads the advantages and returns of the last `prepare`."""
        total = self._check_buffer(buffer)
        if self._buffer is None:
            raise UpkieRuntimeError("call prepare(buffer) first: it copies the advantages and returns update() reads")
        if self._addresses(buffer) != self._buffer:
            raise ValueError("this trainer serves one rollout buffer (a captured update reads its tensors): build another trainer")
        lb, shape, cfg = self._lib, C.byref(self.policy.shape), C.byref(self.config)
        p = lambda t: t.data_ptr()  # noqa: E731
        obs, act = p(buffer.observations), p(buffer.actions)
        vals, logp, adv, ret = p(buffer.values), p(buffer.log_probs), p(self.advantages), p(self.returns)
        if self.process_group is not None:
            if torch.cuda.is_current_stream_capturing():
                raise UpkieRuntimeError("a PpoTrainer with a process group cannot be captured in a graph (every minibatch exchanges the "
                                        "gradients through a collective)")
            self._update_shared(total, shape, cfg, obs, act, vals, logp, adv, ret)
            if sync:
                self.sync_modules()
            return self.stats
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            for e in range(self.n_epochs):
                perm = self.perm[e]
                status = lb.upkie_ppo_advantage_stats(total, self._mb, p(perm), adv, int(self.normalize_advantage), p(self.adv_stats[e]), stream)
                if status < 0:
                    lib.check(status, None)
                for j in range(self.n_minibatches):
                    start = j * self._mb
                    status = lb.upkie_ppo_minibatch_update(
                        shape, cfg, total, start, min(self._mb, total - start), self._mb, p(perm), obs, act, vals, logp, adv, ret,
                        p(self.adv_stats[e, j]), p(self.policy.packed), p(self.m), p(self.v), p(self.scalars), p(self.workspace),
                        p(self.stats[e, j]), stream)
                    if status < 0:
                        lib.check(status, None)
        if sync:
            self.sync_modules()
        return self.stats

    def _update_shared(self, total, shape, cfg, obs, act, vals, logp, adv, ret) -> None:
        """`update`'s epochs and minibatches in the data-parallel form: the same launches split around the exchanges."""
        lb, gx, ax = self._lib, self._grad_exchange, self._adv_exchange
        p = lambda t: t.data_ptr()  # noqa: E731
        W, mb = gx.world, self._mb

        def ok(status):
            if status < 0:
                lib.check(status, None)

        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            for e in range(self.n_epochs):
                perm = p(self.perm[e])
                ok(lb.upkie_ppo_advantage_partials(total, mb, perm, adv, 0, None, W, p(ax.mine), stream))
                ax.exchange()
                ok(lb.upkie_ppo_advantage_partials(total, mb, perm, adv, 1, p(ax.slots), W, p(ax.mine), stream))
                ax.exchange()
                ok(lb.upkie_ppo_advantage_finish(total, mb, int(self.normalize_advantage), p(ax.slots), W, p(self.adv_stats[e]), stream))
                for j in range(self.n_minibatches):
                    start = j * mb
                    size = min(mb, total - start)
                    ok(lb.upkie_ppo_minibatch_gradient(shape, cfg, total, start, size, W * size, mb, perm, obs, act, vals, logp, adv, ret,
                                                       p(self.adv_stats[e, j]), p(self.policy.packed), p(self.workspace), p(gx.mine), stream))
                    gx.exchange()
                    ok(lb.upkie_ppo_minibatch_apply(shape, cfg, W * size, mb, p(gx.slots), W, p(self.policy.packed), p(self.m), p(self.v),
                                                    p(self.scalars), p(self.workspace), p(self.stats[e, j]), stream))

    def train(self, buffer, sync: bool = True) -> torch.Tensor:
        """`prepare` then `update`: SB3's ``PPO.train`` on one full rollout buffer. Returns ``[n_epochs, n_minibatches, 7]``
        (`STAT_NAMES`), on the device."""
        self.prepare(buffer)
        return self.update(buffer, sync)

    def set_lr(self, lr: float) -> None:
        """Write the learning rate (a device word: a captured update reads the new value)."""
        self.scalars[0].fill_(float(lr))

    def sync_modules(self) -> None:
        """Write the packed weights back into the tensors the policy was built from (the modules' parameters, or the
        tensors of `from_sb3_state_dict`): one scatter on the device, then a copy per tensor. The fixed sources
        (observation statistics, action bounds) are not written."""
        pol = self.policy
        self._flat.index_copy_(0, pol._index, pol.packed)  # (padding words, all mapped to the last slot, are zero)
        params = pol._params
        trainable = [params[-1]] + params[:-1]  # sources() order after the four fixed tensors
        start = sum(self._sizes[:4])
        with torch.no_grad():
            for t, n in zip(trainable, self._sizes[4:]):
                t.detach().view(-1).copy_(self._flat[start:start + n])
                start += n

    # ---- state
    def _unpack(self, packed: torch.Tensor):
        flat = torch.zeros(sum(self._sizes) + 1, dtype=torch.float32, device=self.device)
        flat.index_copy_(0, self.policy._index, packed)
        return [t.clone() for t in torch.split(flat[:-1], self._sizes)[4:]]

    def _pack(self, tensors, into: torch.Tensor) -> None:
        if len(tensors) != len(self._sizes) - 4:
            raise ValueError(f"need {len(self._sizes) - 4} tensors (log_std, then weight and bias per layer)")
        flat = [torch.zeros(n, dtype=torch.float32, device=self.device) for n in self._sizes[:4]]
        for t, n in zip(tensors, self._sizes[4:]):
            t = torch.as_tensor(t, dtype=torch.float32).to(self.device).reshape(-1)
            if t.numel() != n:
                raise ValueError(f"a tensor of {t.numel()} values where {n} belong")
            flat.append(t)
        torch.index_select(torch.cat(flat + [torch.zeros(1, dtype=torch.float32, device=self.device)]), 0, self.policy._index, out=into)

    def state_dict(self) -> dict:
        """Adam's state: ``m`` and ``v`` as lists in ``policy.sources()`` order of the trainable tensors (log_std, then
        weight and bias per layer of the actor and of the critic), the step count ``t`` and ``lr``."""
        return {"m": self._unpack(self.m), "v": self._unpack(self.v), "t": int(self.scalars[1].item()), "lr": float(self.scalars[0].item())}

    def load_state_dict(self, sd: dict) -> None:
        self._pack(sd["m"], self.m)
        self._pack(sd["v"], self.v)
        self.scalars.copy_(torch.tensor([float(sd["lr"]), float(sd["t"])], dtype=torch.float64))
