"""fp64 twin of the task targets and their curriculum (csrc/task_targets.hpp; include/upkie_hip.h, "Task targets"): the
five steps of a call per env, the reset and the curriculum's decision, in numpy over whole batches, on
`episode_events_reference.philox4x32_10`. The one float32 operation the device does exactly -- ``high - low`` of two
float32 limits, one rounding -- is done in float32 here too; the fma after it is fp64 (the device rounds it once).
The curriculum's float32 clamps are float32 here (single operations, exactly rounded on both sides). Plain numpy, no
device; below the class are the inputs tests/test_task_targets_gpu.py drives the kernels with."""

import numpy as np

from tests.episode_events_reference import philox4x32_10

STREAM_TARGETS = 7
MUTATIONS = ("new_target_in_final_observation", "no_redraw_at_episode_end", "block_one_for_words_above_four", "countdown_after_decision",
             "final_obs_ignored")


class Twin:
    """The stage for ``num_envs`` envs with global ids ``env_id_offset + n`` under the sim's ``seed``. ``mutation``: one of
    `MUTATIONS`, a one-line bug the GPU test's inputs have to tell from the stage."""

    def __init__(self, num_envs: int, obs_dim: int, ranges, seed: int = 0, env_id_offset: int = 0, resample_steps=(1, 1),
                 stand_prob: float = 0.0, deadband=None, mutation=None):
        assert mutation is None or mutation in MUTATIONS
        self.N, self.D, self.G, self.mutation = int(num_envs), int(obs_dim), len(ranges), mutation
        self.key = (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
        ids = (int(env_id_offset) + np.arange(self.N, dtype=np.uint64)) & np.uint64(0xFFFFFFFFFFFFFFFF)
        self.env_lo, self.env_hi = (ids & np.uint64(0xFFFFFFFF)).astype(np.uint32), (ids >> np.uint64(32)).astype(np.uint32)
        self.threshold = int(np.floor(float(stand_prob) * 2.0 ** 24 + 0.5))  # llround
        self.steps_min, self.steps_max = int(resample_steps[0]), int(resample_steps[1])
        self.deadband = np.zeros(self.G) if deadband is None else np.asarray(deadband, dtype=np.float32).astype(np.float64)
        self.limits = np.asarray(ranges, dtype=np.float32).reshape(self.G, 2)
        N, R = self.N, self.D + self.G
        self.calls = np.zeros(N, dtype=np.uint32)
        self.remaining = np.zeros(N, dtype=np.int32)
        self.target = np.zeros((self.G, N))
        self.observation, self.final_observation = np.zeros((N, R)), np.zeros((N, R))

    def _block(self, envs, call, block):
        return philox4x32_10(self.env_lo[envs], self.env_hi[envs], call, np.uint32((STREAM_TARGETS << 24) | block), *self.key)

    def draw(self, envs, call, r):
        """Step 4 for ``envs`` whose schedule blocks are ``r`` (four arrays): (targets [G, len(envs)], hold lengths)."""
        span = self.steps_max - self.steps_min + 1
        hold = self.steps_min + ((r[3] >> np.uint32(8)) % np.uint32(span)).astype(np.int32)
        stand = (r[0] >> np.uint32(8)).astype(np.int64) < self.threshold  # (an integer compare; threshold 2^24: always)
        blocks = {}
        x = np.zeros((self.G, len(envs)))
        for g in range(self.G):
            blk = 1 if self.mutation == "block_one_for_words_above_four" else 1 + g // 4
            if blk not in blocks:
                blocks[blk] = self._block(envs, call, blk)
            u = (blocks[blk][g % 4] >> np.uint32(8)).astype(np.float64) * (1.0 / 16777216.0)
            low, high = self.limits[g]
            v = np.float64(np.float32(high - low)) * u + np.float64(low)  # (high - low: float32, as the device; then its one fma)
            v = np.where(np.abs(v) < self.deadband[g], 0.0, v)
            x[g] = np.where(stand, 0.0, v)
        return x, hold

    def reset(self, obs, mask=None):
        envs = np.arange(self.N) if mask is None else np.flatnonzero(np.asarray(mask))
        if not len(envs):
            return
        zero = np.zeros(len(envs), dtype=np.uint32)
        r = self._block(envs, zero, 0)
        self.target[:, envs], self.remaining[envs] = self.draw(envs, zero, r)
        self.calls[envs] = 1  # (the draw was the env's call 0)
        self.observation[envs] = np.concatenate([np.asarray(obs, dtype=np.float64)[envs], self.target[:, envs].T], axis=1)

    def step(self, next_obs, terminated=None, truncated=None, final_obs=None):
        """One call; returns what happened per env, as boolean arrays: ``done``, ``drawn`` (a new target), ``held``."""
        N, every = self.N, np.arange(self.N)
        next_obs = np.asarray(next_obs, dtype=np.float64)
        done = np.zeros(N, dtype=bool)
        for flag in (terminated, truncated):
            if flag is not None:
                done |= np.asarray(flag).astype(bool)
        call = self.calls.copy()
        r = self._block(every, call, 0)  # 1. every env, every call
        self.calls += np.uint32(1)
        old = self.target.copy()  # 2. the row of the step's outcome, under the target the policy was given
        outcome = next_obs.copy()
        if final_obs is not None and self.mutation != "final_obs_ignored":
            outcome[done] = np.asarray(final_obs, dtype=np.float64)[done]
        if self.mutation != "no_redraw_at_episode_end":
            self.remaining[done] = 0  # 3.
        count_down = (self.remaining > 0) & ~(done & (self.mutation != "no_redraw_at_episode_end"))
        if self.mutation != "countdown_after_decision":
            self.remaining[count_down] -= 1
        drawn = self.remaining == 0  # 4.
        envs = np.flatnonzero(drawn)
        if len(envs):
            self.target[:, envs], self.remaining[envs] = self.draw(envs, call[envs], [w[envs] for w in r])
        if self.mutation == "countdown_after_decision":
            self.remaining[count_down & ~drawn] -= 1
        tail = self.target if self.mutation == "new_target_in_final_observation" else old
        self.final_observation = np.concatenate([outcome, tail.T], axis=1)
        self.observation = np.concatenate([next_obs, self.target.T], axis=1)  # 5.
        return {"done": done, "drawn": drawn, "held": ~drawn}

    def snapshot(self):
        named = {"calls": self.calls, "remaining": self.remaining, "target": self.target, "observation": self.observation,
                 "final_observation": self.final_observation}
        return {k: v.copy() for k, v in named.items()}


def curriculum_step(limits, seen, score, finished, threshold, step, limit):
    """One look of the curriculum on ``limits`` [G, 2] float32 and ``seen`` [N] int32, both updated in place; returns
    whether the ranges moved. ``score`` [N] fp64, ``finished`` [N] int32; the sum is fp64 (exact for the tests' scores, so
    its order does not show)."""
    new = np.asarray(finished) != seen
    S, M = float(np.sum(np.asarray(score, dtype=np.float64)[new])), int(np.count_nonzero(new))
    seen[new] = np.asarray(finished)[new]
    if not (M > 0 and S > float(threshold) * M):
        return False
    for g in range(len(limits)):
        limits[g, 0] = max(np.float32(limits[g, 0] - np.float32(step[g])), np.float32(limit[g][0]))
        limits[g, 1] = min(np.float32(limits[g, 1] + np.float32(step[g])), np.float32(limit[g][1]))
    return True


# ---- the inputs of the kernel-against-twin tests (tests/test_task_targets_gpu.py), stated once for both test files
GPU_SEED, GPU_CALLS = 11, 40
GPU_SIZES = tuple((n, 1000) for n in (1, 63, 64, 65, 257)) + ((64, 2 ** 32 - 16),)  # (num_envs, env_id_offset); the last: a carry into the high id word
# (D, G): the smallest row; the last word of value block 1; the first of value block 2; a row that is no multiple of 4; the 256-word cap
GPU_WIDTHS = ((1, 1), (4, 4), (6, 5), (30, 2), (248, 8))
CURRICULUM_SIZES = (1, 64, 65, 257, 4097)  # one block of the curriculum's launch (2048 envs) and several


def gpu_settings(G: int) -> dict:
    """Ranges that differ per word and are not symmetric, a deadband on the even words, holds of 1-4 steps."""
    return dict(ranges=[(-0.5 - 0.25 * g, 1.0 + 0.125 * g) for g in range(G)], resample_steps=(1, 4), stand_prob=0.2,
                deadband=[0.125 if g % 2 == 0 else 0.0 for g in range(G)])


def gpu_flags(num_envs: int, env_id_offset: int):
    """(terminated, truncated), each [GPU_CALLS, num_envs] uint8: an episode ends with probability 0.1 per env and call,
    by either flag."""
    rng = np.random.default_rng([num_envs, env_id_offset % 2 ** 32, 7])
    done = rng.random((GPU_CALLS, num_envs)) < 0.1
    by_limit = rng.random((GPU_CALLS, num_envs)) < 0.5
    return (done & ~by_limit).astype(np.uint8), (done & by_limit).astype(np.uint8)


def gpu_observations(num_envs: int, obs_dim: int):
    """(reset obs [N, D], next_obs [GPU_CALLS, N, D], final_obs [GPU_CALLS, N, D]) float32, every word different."""
    rng = np.random.default_rng([num_envs, obs_dim, 8])
    block = rng.standard_normal((2 * GPU_CALLS + 1, num_envs, obs_dim)).astype(np.float32)
    return block[0], block[1:GPU_CALLS + 1], block[GPU_CALLS + 1:]


def curriculum_inputs(num_envs: int):
    """Six looks at threshold 10 with step 0.25 from (-0.5, 0.5) to the limit (-1.0, 1.125) per word of G = 2: (score [6, N]
    fp64, finished [6, N] int32). Scores are multiples of 1/1024 below 2^20 (every summation order is exact). Looks 0,
    2 and 3 are above the threshold (the third hits the limit on the low side, then the high side clamps), 1 below, 4 has
    no newly finished env, 5 is below again."""
    rng = np.random.default_rng([num_envs, 9])
    above = np.array([True, False, True, True, True, False])
    score = np.zeros((6, num_envs))
    finished = np.zeros((6, num_envs), dtype=np.int32)
    count = np.zeros(num_envs, dtype=np.int32)
    for k in range(6):
        new = rng.random(num_envs) < 0.6
        new[rng.integers(num_envs)] = True
        if k == 4:
            new[:] = False
        count = count + new.astype(np.int32)
        finished[k] = count
        base = 12.0 if above[k] else 8.0
        score[k] = base + rng.integers(-1024, 1025, num_envs) / 1024.0  # (in [base - 1, base + 1]: the mean is on base's side of 10)
        # the envs that did not finish carry scores that would flip the decision if they were counted
        score[k][~new] = -1000.0 if above[k] else 1000.0
    return score, finished


CURRICULUM_SETTINGS = dict(threshold=10.0, step=[0.25, 0.25], limit=[(-1.0, 1.125), (-1.0, 1.125)], ranges=[(-0.5, 0.5), (-0.5, 0.5)])
