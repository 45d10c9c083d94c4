"""fp64 twin of the push curriculum (csrc/episode_events.hpp, the levelled instantiation; include/upkie_hip.h, "Push
curriculum"), built on the episode events' twin (tests/episode_events_reference.Twin: the Philox blocks, the link factors
and the push directions are its): steps 2 and 4 of a call restated with the level's rise and fall and the scaled norm
range. The upper end ``hi`` of a level below the top is taken in float32, as the header states it (the kernel's three
roundings); everything after it is fp64. Plain numpy, no device; `GPU_*` and `gpu_flags` are the inputs
tests/test_push_curriculum_gpu.py drives the kernel with, and tests/test_push_curriculum.py holds them to meet every
branch and to tell five one-line bugs from the stage."""

import numpy as np

from tests import episode_events_reference as R

MUTATIONS = ("promotion_on_termination", "start_uses_old_level", "episode_pushes_not_cleared", "demotion_wraps", "top_interpolated")
BRANCHES = ("promotion", "promotion_refused", "demotion", "clamp_at_0", "clamp_at_top", "start_on_ending_call")


def difficulty_of(level, levels: int):
    """float32: 1 at the top (which includes ``levels == 0``), else (float)level / (float)levels."""
    level = np.asarray(level)
    below = level < levels
    out = np.ones(level.shape, dtype=np.float32)
    if levels > 0:
        out[below] = level[below].astype(np.float32) / np.float32(levels)
    return out


def norm_high(level, levels: int, norm_min: float, norm_max: float, interpolate_top: bool = False):
    """fp64 array: ``norm_max`` itself at the top, else fma(norm_max - norm_min, (float)level / (float)levels, norm_min)
    in float32 (the product of two float32 is exact in fp64: one rounding of the sum, then the one to float32)."""
    level = np.asarray(level)
    out = np.full(level.shape, float(norm_max))
    inner = np.ones(level.shape, dtype=bool) if interpolate_top else level < levels
    if levels > 0 and inner.any():
        lo, span = np.float32(norm_min), np.float32(norm_max) - np.float32(norm_min)
        frac = np.minimum(level[inner], levels).astype(np.float32) / np.float32(levels)
        out[inner] = (span.astype(np.float64) * frac.astype(np.float64) + np.float64(lo)).astype(np.float32).astype(np.float64)
    return out


class LevelTwin(R.Twin):
    """`R.Twin` with a difficulty level per env. ``levels`` = L, ``start``, ``up``, ``down``, ``min_pushes`` as
    `upkie_amd.events.PushLevels`; ``mutation``: one of `MUTATIONS`. With ``levels=0`` every bit is `R.Twin`'s."""

    def __init__(self, model, num_envs, levels=0, start=0, up=0, down=0, min_pushes=1, mutation=None, **settings):
        assert mutation is None or mutation in MUTATIONS
        self.levels, self.start, self.up, self.down, self.min_pushes = int(levels), int(start), int(up), int(down), int(min_pushes)
        self.level_mutation = mutation
        self.level = np.full(int(num_envs), self.start, dtype=np.uint32)
        self.episode_pushes = np.zeros(int(num_envs), dtype=np.uint32)
        self.difficulty = difficulty_of(self.level, self.levels)
        super().__init__(model, num_envs, **settings)  # (ends with self.reset())

    def reset(self, mask=None):
        super().reset(mask)
        envs = np.arange(self.N) if mask is None else np.flatnonzero(np.asarray(mask))
        self.level[envs] = self.start
        self.episode_pushes[envs] = 0
        self.difficulty[envs] = difficulty_of(self.level[envs], self.levels)

    def set_push(self, prob=None, norm=None, steps=None):
        if prob is not None:
            self.threshold = int(np.floor(float(prob) * 2.0 ** 24 + 0.5))
        if norm is not None:
            self.norm_min, self.norm_max = float(norm[0]), float(norm[1])
        if steps is not None:
            self.steps_min, self.steps_max = int(steps[0]), int(steps[1])

    def set_levels(self, levels):
        self.level[:] = levels

    def step(self, terminated=None, truncated=None):
        """One call; returns `R.Twin.step`'s arrays and, per env: the branches of `BRANCHES` and ``start_level`` (the
        level a push started at; -1: no start)."""
        N, every, L, mutation = self.N, np.arange(self.N), self.levels, self.level_mutation
        term = np.zeros(N, dtype=bool) if terminated is None else np.asarray(terminated).astype(bool)
        trunc = np.zeros(N, dtype=bool) if truncated is None else np.asarray(truncated).astype(bool)
        done = term | trunc
        r = self._block(every, self.calls, R.STREAM_EVENTS)  # 1. unchanged: a level never changes which words an env draws
        self.calls += np.uint32(1)
        cut = done & (self.remaining > 1)
        level = np.minimum(self.level.astype(np.int64), L)  # (a level read above L is taken as L)
        before = level.copy()
        # 2. first the level: a fall demotes and wins over the time limit, a survived episode that was pushed promotes
        fell, survived = done & term, done & ~term
        promoted = survived & (self.episode_pushes >= self.min_pushes)
        if mutation == "promotion_on_termination":
            fell, promoted = np.zeros(N, dtype=bool), promoted | (done & term)
        happened = {"promotion": promoted, "promotion_refused": survived & ~promoted, "demotion": fell, "clamp_at_0": fell & (level < self.down),
                    "clamp_at_top": promoted & (level + self.up > L)}
        if mutation == "demotion_wraps":
            level[fell] = (level[fell] - self.down) & 0xFFFFFFFF  # (what the next read then takes as L)
        else:
            level[fell] -= np.minimum(level[fell], self.down)
        level[promoted] = np.minimum(level[promoted] + self.up, L)
        if mutation != "episode_pushes_not_cleared":
            self.episode_pushes[done] = 0
        ended = np.flatnonzero(done)  # ... then the existing step 2
        self.episodes[ended] += np.uint32(1)
        self.remaining[ended] = 0
        if self.variation > 0.0 and len(ended):
            self._redraw(ended, self.episodes[ended])
        self.remaining[self.remaining > 0] -= 1  # 3.
        free = self.remaining == 0  # 4.
        start = free & ((r[0] >> np.uint32(8)).astype(np.int64) < self.threshold)
        zero = free & ~start
        envs = np.flatnonzero(start)
        start_level = np.full(N, -1, dtype=np.int64)
        if len(envs):
            at = np.minimum((before if mutation == "start_uses_old_level" else level)[envs], L)  # the NEW level, also on an ending call
            start_level[envs] = at
            hi = norm_high(at, L, self.norm_min, self.norm_max, interpolate_top=mutation == "top_interpolated")
            q = self._block(envs, self.pushes[envs], R.STREAM_PUSH)
            u0, u1 = ((q[i] >> np.uint32(8)).astype(np.float64) * (1.0 / 16777216.0) for i in (0, 1))
            norm, phi = self.norm_min + (hi - self.norm_min) * u0, R.TWO_PI * u1
            self.force[:, envs] = np.stack([norm * np.cos(phi), norm * np.sin(phi), np.zeros(len(envs))])
            self.pushes[envs] += np.uint32(1)
            self.episode_pushes[envs] += np.uint32(1)
            span = max(self.steps_max - self.steps_min + 1, 1)
            self.remaining[envs] = self.steps_min + ((r[3][envs] >> np.uint32(8)) % np.uint32(span)).astype(np.int32)
        self.force[:, zero] = 0.0
        self.level[:] = level.astype(np.uint32)
        self.difficulty[:] = difficulty_of(np.minimum(level, L), L)
        happened.update({"start": start, "hold": ~free, "zero": zero, "cut": cut, "redrawn": done.copy(), "start_level": start_level,
                         "start_on_ending_call": start & done})
        return happened

    def snapshot(self):
        out = super().snapshot()
        out.update({"level": self.level.copy(), "episode_pushes": self.episode_pushes.copy(), "difficulty": self.difficulty.copy()})
        return out


# ---- the inputs of the kernel-against-twin test (tests/test_push_curriculum_gpu.py), stated once for both test files.
# The norms are float32 numbers chosen so that an interpolated top level misses the exact one: max - min = 19 + 2^-20 is a
# tie that rounds to 19 (even), and 19 + min = 20 + 2^-20 a tie that rounds to 20 (even), one ulp below max. (With 5 and
# 20, or any pair whose difference is a float32, fma(max - min, 1, min) IS max and that bug would not show.)
NORM_MIN, NORM_MAX = 1.0 + 2.0 ** -20, 20.0 + 2.0 ** -19
GPU_SETTINGS = dict(push_prob=0.25, push_norm=(NORM_MIN, NORM_MAX), push_steps=(1, 3), inertia_variation=0.3)
GPU_LEVELS = dict(levels=3, start=0, up=1, down=2, min_pushes=1)
GPU_SEED, GPU_CALLS, GPU_SIZES = R.GPU_SEED, R.GPU_CALLS, R.GPU_SIZES
END_PROB, LIMIT_PROB, BOTH_PROB = 0.3, 0.75, 0.1


def gpu_flags(num_envs: int, env_id_offset: int):
    """(terminated, truncated), each [GPU_CALLS, num_envs] uint8: an episode ends with probability END_PROB per env and
    call, at the time limit with probability LIMIT_PROB (else by a fall); BOTH_PROB of the ends carry both flags."""
    rng = np.random.default_rng([num_envs, env_id_offset % 2 ** 32, 17])
    done = rng.random((GPU_CALLS, num_envs)) < END_PROB
    by_limit = rng.random((GPU_CALLS, num_envs)) < LIMIT_PROB
    both = rng.random((GPU_CALLS, num_envs)) < BOTH_PROB
    return (done & (~by_limit | both)).astype(np.uint8), (done & (by_limit | both)).astype(np.uint8)
