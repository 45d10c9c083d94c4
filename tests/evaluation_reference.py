"""Twins of the evaluation tally (upkie_amd.evaluation.EpisodeTally, csrc/eval_episodes.hpp): the bookkeeping loop of
Stable-Baselines3's ``evaluate_policy`` restated in plain Python / numpy from its documented behaviour (SB3 is not
imported), the sizes and the scripted streams the tally is tested at, and a numpy model of the kernel's own order of
operations with the index mistakes a kernel could make, for the sharpness tests."""

import functools
from collections import namedtuple

import numpy as np

from tests.reduction_shapes import episodes_blocks, ordered_append

F32, F64 = np.float32, np.float64
EVAL_STAGE = 1024  # enum value of csrc/eval_episodes.hpp

EvalRow = namedtuple("EvalRow", "N E why")

EVAL_ROWS = [
    EvalRow(1, 1, "one env, one episode"),
    EvalRow(1, 3, "one env gives every episode"),
    EvalRow(37, 5, "N > E: only the last 5 envs count"),
    EvalRow(64, 64, "one wave, a quota of one each"),
    EvalRow(65, 200, "quotas 3 and 4 mixed"),
    EvalRow(257, 300, "blocks of 129 / 128"),
    EvalRow(4099, 1025, "17 blocks; two LDS stages, the second with one entry"),
    EvalRow(65537, 70000, "257 blocks; the last block holds one env"),
    EvalRow(262145, 262145, "the smallest N with more than 256 envs per block: second chunk with one live lane"),
]
EVAL_IDS = [f"N{r.N}-E{r.E}" for r in EVAL_ROWS]
TARGET_TABLE = [(3, 10), (7, 7), (37, 5), (1, 4), (64, 64), (65, 200), (262145, 262145), (5, 1)]  # N < E, N = E, N > E, N = 1


def targets(N, E):
    """SB3: ``episode_count_targets = [(n_eval_episodes + i) // n_envs for i in range(n_envs)]``."""
    return np.array([(E + i) // N for i in range(N)], dtype=np.int64)


def summarise(returns, lengths, limits):
    """The summary in the stated order: sequential fp64 sums in record order (``np.cumsum(...)[-1]``), the lengths' sum
    exact, the variances a second sequential pass over the rounded squares."""
    r = np.asarray(returns, dtype=F64)
    n = r.size
    mean_r = float(np.cumsum(r)[-1]) / n
    dr = r - mean_r
    var_r = float(np.cumsum(dr * dr)[-1]) / n
    mean_l = sum(int(x) for x in lengths) / n
    dl = np.asarray(lengths, dtype=F64) - mean_l
    var_l = float(np.cumsum(dl * dl)[-1]) / n
    return (mean_r, var_r, mean_l, var_l, float(r.min()), float(r.max()), sum(int(x) for x in limits) / n)


class EvaluateTwin:
    """SB3's ``evaluate_policy`` loop for N envs and E episodes: per env the list of its episode's rewards (Python
    floats, summed with ``sum`` when the episode ends, as ``current_rewards += reward`` does from 0.0), the per-env
    Python loop in env order, the record lists. ``rec_truncated`` is what Gymnasium's ``TimeLimit.truncated`` says:
    truncated and not terminated."""

    def __init__(self, N, E):
        self.N, self.E = int(N), int(E)
        self.target = targets(self.N, self.E)
        self.count = np.zeros(self.N, dtype=np.int64)
        self.rewards = [[] for _ in range(self.N)]
        self.rec_return, self.rec_length, self.rec_env, self.rec_truncated = [], [], [], []
        self.steps = 0

    def step(self, reward, terminated=None, truncated=None):
        N = self.N
        reward = np.asarray(reward, dtype=F32)
        term = np.zeros(N, dtype=bool) if terminated is None else np.asarray(terminated, dtype=bool)
        trunc = np.zeros(N, dtype=bool) if truncated is None else np.asarray(truncated, dtype=bool)
        if self.filled < self.E:
            self.steps += 1
        for i in range(N):
            if self.count[i] < self.target[i]:
                self.rewards[i].append(float(reward[i]))
                if term[i] or trunc[i]:
                    self.rec_return.append(sum(self.rewards[i]))
                    self.rec_length.append(len(self.rewards[i]))
                    self.rec_env.append(i)
                    self.rec_truncated.append(int(trunc[i] and not term[i]))
                    self.count[i] += 1
                    self.rewards[i] = []

    @property
    def filled(self):
        return len(self.rec_return)

    def running(self):
        return np.array([sum(r) for r in self.rewards], dtype=F64), np.array([len(r) for r in self.rewards], dtype=np.int64)

    def summary(self):
        assert self.filled == self.E
        return summarise(self.rec_return, self.rec_length, self.rec_truncated)


class BatchEvaluateTwin:
    """`EvaluateTwin` with the envs as numpy arrays (per-env fp64 sums added in step order from 0.0, the finished envs
    taken in env order): the same interface, for the sizes at which a Python loop over the envs is slow.
    tests/test_evaluation.py holds the two to each other."""

    def __init__(self, N, E):
        self.N, self.E = int(N), int(E)
        self.target = targets(self.N, self.E)
        self.count = np.zeros(self.N, dtype=np.int64)
        self.returns, self.lengths = np.zeros(self.N, dtype=F64), np.zeros(self.N, dtype=np.int64)
        self.rec_return, self.rec_length, self.rec_env, self.rec_truncated = [], [], [], []
        self.steps = 0

    def step(self, reward, terminated=None, truncated=None):
        N = self.N
        term = np.zeros(N, dtype=bool) if terminated is None else np.asarray(terminated, dtype=bool)
        trunc = np.zeros(N, dtype=bool) if truncated is None else np.asarray(truncated, dtype=bool)
        if self.filled < self.E:
            self.steps += 1
        live = self.count < self.target
        self.returns[live] += np.asarray(reward, dtype=F32).astype(F64)[live]
        self.lengths[live] += 1
        ended = np.flatnonzero(live & (term | trunc))  # (in env order)
        self.rec_return.extend(self.returns[ended].tolist())
        self.rec_length.extend(self.lengths[ended].tolist())
        self.rec_env.extend(ended.tolist())
        self.rec_truncated.extend((trunc & ~term)[ended].astype(int).tolist())
        self.count[ended] += 1
        self.returns[ended], self.lengths[ended] = 0.0, 0

    filled = EvaluateTwin.filled
    summary = EvaluateTwin.summary

    def running(self):
        return self.returns.copy(), self.lengths.copy()


def evaluate_twin(N, E):
    """`EvaluateTwin` walks the envs in Python: the batched twin above N = 5000."""
    return (BatchEvaluateTwin if N > 5000 else EvaluateTwin)(N, E)


# ---------------------------------------------------------------- the scripted stream
EvalScript = namedtuple("EvalScript", "rewards terminated truncated")
EVAL_STEPS = 12
#   0 nobody; 1 the last env; 2, 3 a random 30 % with both flags overlapping; 4 every env of one middle block (time limits; a
#   row of one block is full behind it); 5 every env, half of them with both flags; 6 a random 30 %; 7 nobody; 8 a random
#   30 %; 9, 10, 11 every env (the largest quota of the rows is 4: with step 5 these fill every row)


@functools.lru_cache(maxsize=None)
def eval_script(row):
    N = row.N
    blocks, rows = episodes_blocks(N)
    rng = np.random.default_rng([N, row.E, 7])
    T = EVAL_STEPS
    rewards = rng.normal(0.5, 1.0, size=(T, N)).astype(F32)
    term, trunc = np.zeros((T, N), dtype=bool), np.zeros((T, N), dtype=bool)
    trunc[1, N - 1] = True
    mid = blocks // 2
    trunc[4, mid * rows:min(N, (mid + 1) * rows)] = True
    for t in (2, 3, 6, 8):
        u = rng.random(N)
        term[t], trunc[t] = u < 0.2, (u >= 0.1) & (u < 0.3)
    term[5] = True
    trunc[5, ::2] = True
    trunc[9] = True
    term[10] = True
    trunc[11] = True
    term[11, 1::3] = True
    for a in (rewards, term, trunc):
        a.setflags(write=False)
    return EvalScript(rewards, term, trunc)


# ---------------------------------------------------------------- the kernel's own order
EVAL_MUTATIONS = ("last_env_dropped", "quota_compared_with_le", "appended_at_zero", "truncated_without_the_mask", "neighbour_of_an_empty_block")


class EvalOrderModel:
    """eval_step_kernel in numpy, with its workspace: every block's finished episodes appended to its segment (what an
    earlier step left behind a segment's end stays there) and found again in env order (`ordered_append`), the record
    written at filled + g under the bound E, the summary in the step that fills the list. `mutation`: one of
    `EVAL_MUTATIONS`, the same with one index mistake."""

    def __init__(self, N, E, mutation=None):
        assert mutation is None or mutation in EVAL_MUTATIONS
        self.N, self.E, self.mutation = N, E, mutation
        self.blocks, self.rows = episodes_blocks(N)
        self.target = ((E + np.arange(N, dtype=np.int64)) // N)
        self.count = np.zeros(N, dtype=np.int64)
        self.ep_return, self.ep_length = np.zeros(N, dtype=F64), np.zeros(N, dtype=np.int32)
        self.rec_return, self.rec_length = np.zeros(E, dtype=F64), np.zeros(E, dtype=np.int32)
        self.rec_env, self.rec_truncated = np.zeros(E, dtype=np.int32), np.zeros(E, dtype=np.uint8)
        self.fin_return, self.fin_length = np.zeros(N, dtype=F64), np.zeros(N, dtype=np.int32)
        self.fin_env, self.fin_truncated = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.uint8)
        self.filled, self.steps = 0, 0
        self.summary = None

    def step(self, reward, terminated=None, truncated=None):
        N, E, rows, blocks = self.N, self.E, self.rows, self.blocks
        term = np.zeros(N, dtype=bool) if terminated is None else np.asarray(terminated, dtype=bool)
        trunc = np.zeros(N, dtype=bool) if truncated is None else np.asarray(truncated, dtype=bool)
        live = self.count <= self.target if self.mutation == "quota_compared_with_le" else self.count < self.target
        if self.mutation == "last_env_dropped":  # (the last block stops one env early)
            live[N - 1:] = False
        ret = self.ep_return + np.asarray(reward, dtype=F32).astype(F64)
        length = self.ep_length + 1
        done = live & (term | trunc)
        limit = trunc if self.mutation == "truncated_without_the_mask" else trunc & ~term
        self.ep_return = np.where(live, np.where(done, 0.0, ret), self.ep_return)
        self.ep_length = np.where(live, np.where(done, 0, length), self.ep_length).astype(np.int32)
        self.count = self.count + done
        idx, at, _, total, src_of = ordered_append(done, rows, blocks, self.mutation)
        self.fin_return[at], self.fin_length[at], self.fin_env[at], self.fin_truncated[at] = ret[idx], length[idx], idx, limit[idx]
        g = np.arange(total)
        src = src_of(g)
        filled = self.filled
        slot = g if self.mutation == "appended_at_zero" else filled + g
        keep = slot < E
        slot, src = slot[keep], src[keep]
        self.rec_return[slot], self.rec_length[slot] = self.fin_return[src], self.fin_length[src]
        self.rec_env[slot], self.rec_truncated[slot] = self.fin_env[src], self.fin_truncated[src]
        self.filled = min(filled + total, E)
        if filled < E:
            self.steps += 1
            if self.filled == E:
                self.summary = summarise(self.rec_return, self.rec_length, self.rec_truncated)


def same_as_twin(model, twin):
    """Whether every value the GPU test compares has the twin's bits: the records so far, the counts, the fill, the steps,
    the running episodes and, once full, the summary."""
    k = twin.filled
    tr, tl = twin.running()
    same = (model.filled == k and model.steps == twin.steps and model.rec_return[:k].tolist() == list(twin.rec_return)
            and model.rec_length[:k].tolist() == list(twin.rec_length) and model.rec_env[:k].tolist() == list(twin.rec_env)
            and model.rec_truncated[:k].tolist() == list(twin.rec_truncated) and np.array_equal(model.count, twin.count)
            and np.array_equal(model.ep_return, tr) and np.array_equal(model.ep_length, tl))
    if same and k == twin.E:
        same = model.summary == twin.summary()
    return same


def run_eval_script(script, *runners, after=None):
    """Every step of `script` through each of `runners` (twins, models or the device object behind an adapter); `after(t)`
    is called behind every step."""
    for t in range(script.rewards.shape[0]):
        for r in runners:
            r.step(script.rewards[t], script.terminated[t], script.truncated[t])
        if after is not None:
            after(t)
