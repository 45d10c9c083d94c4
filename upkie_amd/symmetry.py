"""Mirror symmetry of the robot for the PPO update (rsl_rl's ``symmetry_cfg``): every stored sample gets a mirrored
partner -- data augmentation -- and a mirror loss pulls the policy's mean on the mirrored observation towards the
mirrored mean. The rollout is untouched: `PpoTrainer(symmetry=)` / `Ppo(symmetry=)` hand a `MirrorSymmetry` to
``upkie_ppo_minibatch_update_mirror`` (include/upkie_hip.h, "PPO update with mirror symmetry", states the arithmetic).

A mirror is a signed permutation per row kind: word ``k`` of a mirrored row is ``sign[k] * row[index[k]]``. Each must be
an involution (``index[index[k]] == k``, partners' signs equal; a fixed point may carry either sign). The tables are
validated here by name and again by the library, on the host, before any index reaches the device.

With a live normaliser the update trains on the normalised rows the rollout stored, so the mirror acts on NORMALISED
rows: a sign-flipped word whose running mean is not zero is mirrored about that mean, slightly off the true mirror."""

import math
from typing import Optional, Sequence

import numpy as np

# the Gyropod observation [position, pitch, yaw, ground velocity, pitch rate, yaw velocity] and action [ground velocity,
# yaw velocity] under a left/right mirror: pure sign flips (tests/test_symmetry.py pins them to the fp64 oracle)
GYROPOD_OBS_SIGN = (1.0, 1.0, -1.0, 1.0, 1.0, -1.0)
GYROPOD_ACT_SIGN = (1.0, -1.0)
FLIPPED_TARGETS = ("yaw_velocity",)  # `upkie_amd.targets.TaskTargets` names that change sign under the mirror


def _table(name: str, index, sign):
    """(int32 index, float32 sign) of one mirror, checked: range, involution, signs of +-1, partners' signs equal."""
    idx, sgn = np.asarray(index), np.asarray(sign, dtype=np.float64)
    if idx.ndim != 1 or sgn.shape != idx.shape or idx.size < 1:
        raise ValueError(f"{name}_index and {name}_sign must be one-dimensional and of the same, positive length")
    if not np.issubdtype(idx.dtype, np.integer):
        raise ValueError(f"{name}_index must hold integers")
    n = idx.size
    if (idx < 0).any() or (idx >= n).any():
        k = int(np.flatnonzero((idx < 0) | (idx >= n))[0])
        raise ValueError(f"{name}_index[{k}] = {int(idx[k])} is out of range [0, {n})")
    if not np.isin(sgn, (-1.0, 1.0)).all():
        k = int(np.flatnonzero(~np.isin(sgn, (-1.0, 1.0)))[0])
        raise ValueError(f"{name}_sign[{k}] = {sgn[k]} must be +1 or -1")
    if (idx[idx] != np.arange(n)).any():
        k = int(np.flatnonzero(idx[idx] != np.arange(n))[0])
        raise ValueError(f"{name}_index is not an involution: index[index[{k}]] = {int(idx[idx][k])}")
    if (sgn[idx] != sgn).any():
        k = int(np.flatnonzero(sgn[idx] != sgn)[0])
        raise ValueError(f"{name}_sign differs between the partners {k} and {int(idx[k])}: the mirror would not be an involution")
    return idx.astype(np.int32), sgn.astype(np.float32)


class MirrorSymmetry:
    """The mirror tables of the observation (``obs_index``, ``obs_sign``), the action and -- for an asymmetric policy --
    the critic's row, plus the two switches of the update: ``augment`` (the mirrored partners' surrogate and value terms
    join the loss, whose means then run over twice the samples) and ``mirror_coef >= 0`` (the weight of the mirror loss,
    which is computed and logged as ``train/mirror_loss`` whatever the weight). Symmetry is code, like a schedule: `Ppo.load`
    is given it again."""

    def __init__(self, obs_index, obs_sign, act_index, act_sign, critic_index=None, critic_sign=None, augment: bool = True,
                 mirror_coef: float = 0.0):
        self.obs_index, self.obs_sign = _table("obs", obs_index, obs_sign)
        self.act_index, self.act_sign = _table("act", act_index, act_sign)
        if (critic_index is None) != (critic_sign is None):
            raise ValueError("critic_index and critic_sign come together")
        self.critic_index = self.critic_sign = None
        if critic_index is not None:
            self.critic_index, self.critic_sign = _table("critic", critic_index, critic_sign)
        coef = float(mirror_coef)
        if not (coef >= 0.0 and math.isfinite(coef)):
            raise ValueError(f"mirror_coef must be finite and not negative, got {mirror_coef}")
        self.augment, self.mirror_coef = bool(augment), coef

    # ---- builders
    @classmethod
    def signs(cls, obs_sign: Sequence[float], act_sign: Sequence[float], critic_sign: Optional[Sequence[float]] = None, **kw):
        """The identity-permutation case: a mirror that only flips signs."""
        critic = {} if critic_sign is None else dict(critic_index=np.arange(len(critic_sign)), critic_sign=critic_sign)
        return cls(np.arange(len(obs_sign)), obs_sign, np.arange(len(act_sign)), act_sign, **critic, **kw)

    @classmethod
    def gyropod(cls, targets=None, **kw):
        """The Gyropod env's mirror: yaw, yaw velocity and the yaw command flip. ``targets`` (a `TaskTargets`, or its
        names) appends the target words; a target named ``yaw_velocity`` flips."""
        names = () if targets is None else tuple(getattr(targets, "names", targets))
        tail = tuple(-1.0 if str(n) in FLIPPED_TARGETS else 1.0 for n in names)
        return cls.signs(GYROPOD_OBS_SIGN + tail, GYROPOD_ACT_SIGN, **kw)

    def for_pipeline(self, pipeline):
        """This mirror (of one raw frame) for the policy behind an `AgentPipeline`: ``[obs | command]`` (the command when
        ``action_in_observation``) tiled over the ``stack`` frames."""
        D, A, S = int(pipeline.obs_dim), int(pipeline.act_dim), int(pipeline.stack)
        if self.obs_index.size != D or self.act_index.size != A:
            raise ValueError(f"the mirror is of {self.obs_index.size} observation and {self.act_index.size} action words, the pipeline's frame "
                             f"holds {D} and {A}")
        index, sign = self.obs_index.astype(np.int64), self.obs_sign
        if pipeline.action_in_observation:
            index, sign = np.concatenate([index, D + self.act_index]), np.concatenate([sign, self.act_sign])
        F = index.size
        return MirrorSymmetry(np.concatenate([f * F + index for f in range(S)]), np.tile(sign, S), self.act_index, self.act_sign,
                              self.critic_index, self.critic_sign, augment=self.augment, mirror_coef=self.mirror_coef)

    # ---- what the trainer needs
    def check_shape(self, shape) -> None:
        """Refuse, by name, tables that do not fit the policy's shape (the library repeats it)."""
        D, A, Dc = int(shape.obs_dim), int(shape.act_dim), int(getattr(shape, "critic_obs_dim", 0))
        if self.obs_index.size != D or self.act_index.size != A:
            raise ValueError(f"the mirror is of {self.obs_index.size} observation and {self.act_index.size} action words, the policy takes {D} "
                             f"and {A}")
        if Dc and self.critic_index is None:
            raise ValueError(f"the policy is asymmetric (its critic reads {Dc} words): the mirror needs critic_index and critic_sign")
        if not Dc and self.critic_index is not None:
            raise ValueError("the policy is symmetric (its critic reads the observation): critic_index and critic_sign are superfluous")
        if Dc and self.critic_index.size != Dc:
            raise ValueError(f"the mirror's critic tables are of {self.critic_index.size} words, the policy's critic takes {Dc}")

    def mirror_obs(self, rows):
        """``rows[..., k] -> obs_sign[k] * rows[..., obs_index[k]]`` (numpy or torch rows)."""
        return _apply(rows, self.obs_index, self.obs_sign)

    def mirror_action(self, rows):
        return _apply(rows, self.act_index, self.act_sign)

    def mirror_critic_obs(self, rows):
        return _apply(rows, self.critic_index, self.critic_sign)


def _apply(rows, index, sign):
    if isinstance(rows, np.ndarray):
        return rows[..., index] * sign.astype(rows.dtype)
    import torch

    return rows[..., torch.as_tensor(index, dtype=torch.long, device=rows.device)] * torch.as_tensor(sign, dtype=rows.dtype, device=rows.device)
