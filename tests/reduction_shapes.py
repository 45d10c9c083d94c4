"""The sizes the two ticketed reductions of the rollout side (csrc/episodes.hpp: episodes_step_kernel; csrc/vecnorm.hpp:
vecnorm_moments_kernel, vecnorm_merge_kernel) are tested at, and the builders the tests share, all plain numpy under seeds of
the row: the launch plans restated from the header comments, the scripted streams, a batched Monitor twin, and numpy models of
the kernels' own order of operations (with the mistakes a kernel could make, for the sharpness tests).

`EPISODE_ROWS` and `VECNORM_ROWS` hold the sizes of tests/test_time_limits_gpu.py and tests/test_vecnorm_gpu.py plus the rows
that reach the grid geometries those leave out; tests/test_reduction_matrix.py asserts that the tables cover what they claim,
tests/test_reduction_matrix_gpu.py runs every row on the device."""

import functools
from collections import deque, namedtuple

import numpy as np

from tests import vecnorm_reference as V

F32, F64 = np.float32, np.float64

# enum values of csrc/episodes.hpp and csrc/vecnorm.hpp
EPISODES_THREADS, EPISODES_MAX_BLOCKS, EPISODES_MAX_WINDOW, EPISODES_COUNTS_OFFSET, EPISODES_STAGE = 256, 1024, 65536, 256, 1024
VECNORM_THREADS, VECNORM_MAX_BLOCKS, VECNORM_PARTIAL_WORDS, VECNORM_PARTIALS_OFFSET, VECNORM_CHUNK = 256, 256, 8192, 256, 8


def _ceil(a, b):
    return -(-a // b)


# ================================================================ episode statistics
EpisodeRow = namedtuple("EpisodeRow", "N window why")

EPISODE_ROWS = [
    EpisodeRow(4096, 100, "tests/test_time_limits_gpu.py's: 16 full blocks"),
    EpisodeRow(4096, 1000, "tests/test_time_limits_gpu.py's: 16 full blocks"),
    EpisodeRow(37, 5, "tests/test_time_limits_gpu.py's: one block"),
    EpisodeRow(1, 1, "one env, a ring of one"),
    EpisodeRow(257, 300, "blocks of 129 and 128; window larger than N"),
    EpisodeRow(4099, 100, "17 blocks of 242, the last one 227"),
    EpisodeRow(65537, 1025, "257 blocks, so block 256 is thread 64's first; the last block holds one env; two stages, the second with "
                            "one entry"),
    EpisodeRow(262145, 2500, "the smallest N with rows > 256: 1021 blocks of 257, a second chunk with one live lane; the last block "
                             "has 5"),
    EpisodeRow(300001, 65536, "all 1024 blocks, rows 293; the largest window (64 stages)"),
]
EPISODE_EXISTING = [(4096, 100), (4096, 1000), (37, 5)]
EPISODE_IDS = [f"N{r.N}-w{r.window}" for r in EPISODE_ROWS]
GRAPHED_EPISODE_ROW = (65537, 1025)


def episodes_blocks(N):
    """`episodes_blocks`: (blocks, rows): one block per 256 envs, at most 1024, the envs spread evenly over them."""
    g = min(_ceil(N, EPISODES_THREADS), EPISODES_MAX_BLOCKS)
    rows = _ceil(N, g)
    return _ceil(N, rows), rows


def episodes_workspace_bytes(N):
    """The ticket's 256 bytes, 1024 counts, then a double and an int per env."""
    return EPISODES_COUNTS_OFFSET + EPISODES_MAX_BLOCKS * 4 + 12 * N


def episodes_plan(row):
    """What the kernel's loops do at this row: the grid, the last block's envs, the chunks of 256 a block walks and the live
    lanes of its last chunk, the stages of a full ring and the entries of the last one."""
    blocks, rows = episodes_blocks(row.N)
    chunks, stages = _ceil(rows, EPISODES_THREADS), _ceil(row.window, EPISODES_STAGE)
    return {"blocks": blocks, "rows": rows, "last_block": row.N - (blocks - 1) * rows, "chunks": chunks,
            "last_chunk_lanes": rows - (chunks - 1) * EPISODES_THREADS, "prefix_threads": _ceil(blocks, EPISODES_MAX_BLOCKS // EPISODES_THREADS),
            "stages": stages, "last_stage": row.window - (stages - 1) * EPISODES_STAGE}


EpisodeScript = namedtuple("EpisodeScript", "rewards terminated truncated given reset_after mask")
EPISODE_STEPS = 9
#   0 nobody; 1 the last env; 2 every env of one middle block; 3 every env; 4 the first env of each block (then the masked
#   reset); 5 a random 30 % with both flags overlapping; 6 env 0; 7 another random 30 %; 8 every env again (at a head that is
#   not 0). `given`: the flags the launch is handed, the other is None (and holds no True).
EPISODE_GIVEN = ("both", "truncated", "terminated", "both", "terminated", "both", "terminated", "truncated", "both")


@functools.lru_cache(maxsize=None)
def episode_script(row):
    N = row.N
    blocks, rows = episodes_blocks(N)
    rng = np.random.default_rng([N, row.window])
    T = EPISODE_STEPS
    rewards = rng.normal(0.5, 1.0, size=(T, N)).astype(F32)
    term, trunc = np.zeros((T, N), dtype=bool), np.zeros((T, N), dtype=bool)
    trunc[1, N - 1] = True
    mid = blocks // 2
    term[2, mid * rows:min(N, (mid + 1) * rows)] = True
    term[3] = True
    trunc[3, ::2] = True
    term[4, ::rows] = True
    u = rng.random(N)
    term[5], trunc[5] = u < 0.2, (u >= 0.1) & (u < 0.3)
    term[6, 0] = True
    trunc[7] = rng.random(N) < 0.3
    trunc[8] = True
    term[8, 1::3] = True
    for t, given in enumerate(EPISODE_GIVEN):
        assert given == "both" or not (term[t] if given == "truncated" else trunc[t]).any()
    mask = np.arange(N) % 7 == 0
    for a in (rewards, term, trunc, mask):
        a.setflags(write=False)
    return EpisodeScript(rewards, term, trunc, EPISODE_GIVEN, 4, mask)


def flags_of(script, t, envs=slice(None)):
    """(terminated, truncated) of step t as the launch and the twins are given them: None for the one that is left out."""
    given = script.given[t]
    return (script.terminated[t, envs] if given != "truncated" else None), (script.truncated[t, envs] if given != "terminated" else None)


def done_of(script, t):
    return script.terminated[t] | script.truncated[t]


class BatchMonitorTwin:
    """tests/episodes_reference.py's `MonitorTwin` with the envs as numpy arrays: per-env fp64 return sums added in step
    order, int lengths, the deque. The same interface (`ep_info_buffer` of {"r", "l"}, `total_episodes`, `means`,
    `safe_mean`, `running`), so that `_compare` of tests/test_time_limits_gpu.py takes either."""

    def __init__(self, num_envs, window=100):
        self.num_envs, self.window = int(num_envs), int(window)
        self.returns = np.zeros(self.num_envs, dtype=F64)
        self.lengths = np.zeros(self.num_envs, dtype=np.int64)
        self.ep_info_buffer = deque(maxlen=self.window)
        self.total_episodes = 0

    def step(self, reward, terminated=None, truncated=None):
        done = np.zeros(self.num_envs, dtype=bool)
        for flags in (terminated, truncated):
            if flags is not None:
                done |= np.asarray(flags, dtype=bool)
        self.returns += np.asarray(reward, dtype=F32).astype(F64)  # (0.0 + r0 + r1 + ...: Python's sum over Monitor.rewards)
        self.lengths += 1
        ended = np.flatnonzero(done)  # (in env order)
        kept = ended[-self.window:]  # (what a deque of maxlen window keeps of them)
        self.ep_info_buffer.extend({"r": r, "l": l} for r, l in zip(self.returns[kept].tolist(), self.lengths[kept].tolist()))
        self.total_episodes += int(ended.size)
        self.returns[ended], self.lengths[ended] = 0.0, 0

    def reset(self, mask=None):
        sel = slice(None) if mask is None else np.asarray(mask, dtype=bool)
        self.returns[sel], self.lengths[sel] = 0.0, 0

    def running(self):
        return self.returns.copy(), self.lengths.copy()

    def means(self):
        if not self.ep_info_buffer:
            return 0.0, 0.0
        n = len(self.ep_info_buffer)
        total = float(np.cumsum(np.array([e["r"] for e in self.ep_info_buffer], dtype=F64))[-1])  # (sequential, oldest first)
        return total / n, sum(e["l"] for e in self.ep_info_buffer) / n

    def safe_mean(self, key):
        values = [e[key] for e in self.ep_info_buffer]
        return np.nan if len(values) == 0 else float(np.mean(values))


def monitor_twin(row):
    """`MonitorTwin` walks the envs in Python: the batched twin above N = 5000."""
    from tests.episodes_reference import MonitorTwin

    return (BatchMonitorTwin if row.N > 5000 else MonitorTwin)(row.N, window=row.window)


def ordered_append(done, rows, blocks, mutation=None):
    """csrc/episode_append.hpp in numpy, for both order models: the finished envs `idx` in env order, their places `at` in the
    segment arrays, the exclusive prefix `offsets` of the blocks' counts, its end `total`, and `src(g)`, the place of
    finished episodes g (an array): in the last block with offsets[b] <= g, unless `mutation` is the search's mistake."""
    idx = np.flatnonzero(done)
    block = idx // rows
    offsets = np.concatenate([[0], np.cumsum(np.bincount(block, minlength=blocks))])
    at = block * rows + (np.arange(idx.size) - offsets[block])

    def src(g):
        lo = np.searchsorted(offsets[:blocks], g, side="right") - 1
        if mutation == "neighbour_of_an_empty_block":  # the first block with offsets[b] == g: an empty one, where there is one
            left = np.minimum(np.searchsorted(offsets[:blocks], g, side="left"), blocks - 1)
            lo = np.where(offsets[left] == g, left, lo)
        return lo * rows + (g - offsets[lo])
    return idx, at, offsets, int(offsets[blocks]), src


EPISODE_MUTATIONS = ("last_row_dropped", "neighbour_of_an_empty_block", "first_window_kept", "slot_without_the_wrap")


class EpisodesOrderModel:
    """episodes_step_kernel in numpy, with its workspace: every block's finished episodes appended to its segment (what an
    earlier step left behind a segment's end stays there) and found again in env order (`ordered_append`), the ring written
    at head + j wrapped, the means from the oldest entry. `mutation`: one of `EPISODE_MUTATIONS`, the same with one index
    mistake."""

    def __init__(self, N, window, mutation=None):
        assert mutation is None or mutation in EPISODE_MUTATIONS
        self.N, self.window, self.mutation = N, window, mutation
        self.blocks, self.rows = episodes_blocks(N)
        self.ep_return, self.ep_length = np.zeros(N, dtype=F64), np.zeros(N, dtype=np.int32)
        self.ring_return, self.ring_length = np.zeros(2 * window, dtype=F64), np.zeros(2 * window, dtype=np.int32)  # (behind [window): nowhere)
        self.fin_return, self.fin_length = np.zeros(N, dtype=F64), np.zeros(N, dtype=np.int32)
        self.total, self.head, self.fill = 0, 0, 0
        self.means = (0.0, 0.0)
        self.last = {}

    def step(self, reward, terminated=None, truncated=None):
        N, window, rows, blocks = self.N, self.window, self.rows, self.blocks
        live = N - 1 if self.mutation == "last_row_dropped" else N  # (the last block stops one env early)
        done = np.zeros(N, dtype=bool)
        for flags in (terminated, truncated):
            if flags is not None:
                done |= np.asarray(flags, dtype=bool)
        done[live:] = False
        ret = self.ep_return + np.asarray(reward, dtype=F32).astype(F64)
        length = self.ep_length + 1
        self.ep_return[:live] = np.where(done, 0.0, ret)[:live]
        self.ep_length[:live] = np.where(done, 0, length)[:live]
        idx, at, offsets, total, src_of = ordered_append(done, rows, blocks, self.mutation)
        self.fin_return[at], self.fin_length[at] = ret[idx], length[idx]
        keep = min(total, window)
        first = 0 if self.mutation == "first_window_kept" else total - keep
        src = src_of(first + np.arange(keep))
        slot = self.head + np.arange(keep)
        if self.mutation != "slot_without_the_wrap":
            slot = np.where(slot < window, slot, slot - window)
        self.ring_return[slot], self.ring_length[slot] = self.fin_return[src], self.fin_length[src]
        self.last = {"total": total, "keep": keep, "head": self.head, "counts": np.diff(offsets)}
        self.fill = min(self.fill + keep, window)
        self.head = (self.head + keep) % window
        self.total += total
        r, l = self.ring()
        self.means = (float(np.cumsum(r)[-1]) / self.fill, int(l.astype(np.int64).sum()) / self.fill) if self.fill else (0.0, 0.0)

    def reset(self, mask=None):
        sel = slice(None) if mask is None else np.asarray(mask, dtype=bool)
        self.ep_return[sel], self.ep_length[sel] = 0.0, 0

    def ring(self):
        """(returns, lengths) of the ring, oldest first."""
        order = ((self.head - self.fill) % self.window + np.arange(self.fill)) % self.window
        return self.ring_return[order], self.ring_length[order]


def same_as_twin(model, twin):
    """Whether every value `_compare` checks has the twin's bits."""
    r, l = model.ring()
    want = list(twin.ep_info_buffer)
    tr, tl = twin.running()
    return (r.tolist() == [e["r"] for e in want] and l.tolist() == [e["l"] for e in want] and model.total == twin.total_episodes
            and model.means == twin.means() and np.array_equal(model.ep_return, tr) and np.array_equal(model.ep_length, tl))


def run_episode_script(script, *runners, envs=slice(None), after=None):
    """Every step and the masked reset of `script` through each of `runners` (twins or models over the envs `envs`);
    `after(t)` is called behind every step."""
    for t in range(len(script.given)):
        term, trunc = flags_of(script, t, envs)
        for r in runners:
            r.step(script.rewards[t, envs], term, trunc)
        if t == script.reset_after:
            for r in runners:
                r.reset(script.mask[envs])
        if after is not None:
            after(t)


# ================================================================ the running normaliser
VecnormRow = namedtuple("VecnormRow", "N D why")

VECNORM_ROWS = [
    VecnormRow(4096, 4, "tests/test_vecnorm_gpu.py's"),
    VecnormRow(1, 3, "tests/test_vecnorm_gpu.py's: one env"),
    VecnormRow(1001, 5, "tests/test_vecnorm_gpu.py's: 51 slots, one idle thread"),
    VecnormRow(333, 256, "tests/test_vecnorm_gpu.py's: cols = 257"),
    VecnormRow(65536, 30, "tests/test_vecnorm_gpu.py's: the cap 132 binds"),
    VecnormRow(257, 1, "blocks 129 / 128"),
    VecnormRow(513, 3, "85 slots, an odd tree; 3 blocks, so an odd last-block tree"),
    VecnormRow(4097, 85, "slots = 3"),
    VecnormRow(4097, 86, "slots = 2, 84 idle threads; 9 partials per last-block slot"),
    VecnormRow(2049, 128, "slots = 2, no idle thread; last-block slots = 1"),
    VecnormRow(600, 129, "slots = 1, 127 idle, no tree"),
    VecnormRow(8191, 255, "cols = 256; cap 16 binds; rows 512; the last block has 511, so a last chunk of 7"),
    VecnormRow(3841, 256, "cap 15 binds; rows 257, so a returns lane has 2 rows; two last-block groups"),
    VecnormRow(70001, 7, "256 blocks; rows 274; 32 last-block slots with 8 partials each"),
    VecnormRow(65537, 1, "256 blocks, the last with 2 envs"),
]
VECNORM_EXISTING = [(4096, 4), (1, 3), (1001, 5), (333, 256), (65536, 30)]
VECNORM_IDS = [f"{r.N}x{r.D}" for r in VECNORM_ROWS]
VECNORM_STEPS = 6
FORMS = ("two_launch", "one_launch", "reset_first", "no_norm_obs")
# the shards of the data-parallel form in one process: (D, envs per shard)
SHARDED = [(85, (257,)), (85, (257, 1)), (85, (257, 1, 513)), (86, (4097, 4097))]


def vecnorm_blocks(N, D):
    """`vecnorm_blocks`: (blocks, rows, cap): one block per 256 envs, at most 256 and at most 8192 / (2 (D + 1))."""
    cap = min(max(VECNORM_PARTIAL_WORDS // (2 * (D + 1)), 1), VECNORM_MAX_BLOCKS)
    g = min(_ceil(N, VECNORM_THREADS), cap)
    rows = _ceil(N, g)
    return _ceil(N, rows), rows, cap


def vecnorm_workspace_bytes(N, D):
    return VECNORM_PARTIALS_OFFSET + vecnorm_blocks(N, D)[0] * 2 * (D + 1) * 8


def column_groups(obs_cols, ret_col):
    """The column groups a block takes in turn: (first column, columns, is the returns'): the observation columns at most 256
    at a time, then the returns column alone."""
    groups = [(c0, min(obs_cols - c0, VECNORM_THREADS), False) for c0 in range(0, obs_cols, VECNORM_THREADS)]
    return groups + ([(obs_cols, 1, True)] if ret_col else [])


def lane_rows(envs, slots):
    """Rows of lane slot p = 0 .. slots - 1 of a block with `envs` envs: p, p + slots, ..."""
    return np.maximum(0, -(-(envs - np.arange(slots)) // slots))


def group_plan(envs, g):
    """The in-block plan of a group of g columns in a block of `envs` envs: slots, idle threads, the most rows a lane
    takes, and the sizes of the lanes' last chunks of 8."""
    slots = VECNORM_THREADS // g
    rows = lane_rows(envs, slots)
    return {"g": g, "slots": slots, "idle": VECNORM_THREADS - g * slots, "lane_rows": int(rows.max()),
            "last_chunks": sorted({int((k - 1) % VECNORM_CHUNK + 1) for k in rows if k > 0})}


def last_block_plan(blocks, cols):
    """The last block's plan: per group of at most 256 columns (g, slots = min(blocks, 256 / g), most partials per slot)."""
    plans = []
    for c0 in range(0, cols, VECNORM_THREADS):
        g = min(cols - c0, VECNORM_THREADS)
        slots = min(blocks, VECNORM_THREADS // g)
        plans.append({"g": g, "slots": slots, "partials": _ceil(blocks, slots)})
    return plans


def vecnorm_plan(row, form="two_launch"):
    """Everything about launch A at this row: the grid, the columns of the step launch of `form`, the in-block plan of every
    group in a full block and in the last block, and the last block's own plan."""
    blocks, rows, cap = vecnorm_blocks(row.N, row.D)
    obs_cols = 0 if form == "no_norm_obs" else row.D
    last = row.N - (blocks - 1) * rows
    groups = column_groups(obs_cols, 1)
    return {"blocks": blocks, "rows": rows, "cap": cap, "cap_binds": _ceil(row.N, VECNORM_THREADS) > cap, "last_block_envs": last,
            "cols": obs_cols + 1, "full": [group_plan(rows, g) for _, g, _ in groups], "short": [group_plan(last, g) for _, g, _ in groups],
            "last_block": last_block_plan(blocks, obs_cols + 1)}


@functools.lru_cache(maxsize=2)
def vecnorm_inputs(N, D, T=VECNORM_STEPS):
    """T steps as `_inputs` of tests/test_vecnorm_gpu.py (column 0: mean 1e3, std 0.1; about 2 % done), with step 1 in
    which nothing is done and step 3 in which everything is."""
    rng = np.random.default_rng([N, D])
    obs = rng.normal(loc=rng.normal(size=D), scale=rng.uniform(0.5, 3.0, size=D), size=(T, N, D)).astype(F32)
    obs[:, :, 0] = rng.normal(loc=1e3, scale=0.1, size=(T, N)).astype(F32)
    reward = rng.normal(loc=0.5, scale=2.0, size=(T, N)).astype(F32)
    term = (rng.random((T, N)) < 0.01).astype(np.uint8)
    trunc = (rng.random((T, N)) < 0.01).astype(np.uint8)
    term[1], trunc[1] = 0, 0
    term[3], trunc[3, ::2] = 1, 1
    for a in (obs, reward, term, trunc):
        a.setflags(write=False)
    return obs, reward, term, trunc


def twin_of(N, D, form):
    return V.VecNormalizeTwin(N, D, norm_obs=form != "no_norm_obs", norm_reward=form != "one_launch")


def _ulps(a, b):
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return np.max(np.abs(a.astype(F64) - b.astype(F64)) / np.spacing(np.maximum(np.abs(a), np.abs(b))), initial=0.0)


def stats_ratios(got, twin):
    """error / bound of every statistic `_check_stats` of tests/test_vecnorm_gpu.py checks, under its bounds: 1e-9 of
    |mean| + std on a mean, 1e-9 relative on a variance, 1e-12 (relative + absolute) on the returns, one ulp on the fp32
    mirrors, the counts exactly (inf where they differ). `got`: obs_mean, obs_var, obs_count, ret (mean, var, count),
    returns, and mean_f32 / std_f32 where there are mirrors."""
    def ratio(err, bound):
        err, bound = np.asarray(err, dtype=F64), np.asarray(bound, dtype=F64)
        with np.errstate(divide="ignore", invalid="ignore"):
            return float(np.max(np.where(err > 0, err / bound, 0.0), initial=0.0))

    o, r = twin.obs_rms, twin.ret_rms
    out = {"obs_mean": ratio(np.abs(got["obs_mean"] - o.mean), 1e-9 * (np.abs(o.mean) + np.sqrt(o.var))),
           "obs_var": ratio(np.abs(got["obs_var"] - o.var), 1e-9 * o.var),
           "ret_mean": ratio(abs(got["ret"][0] - r.mean), 1e-9 * (abs(r.mean) + np.sqrt(r.var))),
           "ret_var": ratio(abs(got["ret"][1] - r.var), 1e-9 * r.var),
           "counts": 0.0 if got["ret"][2] == r.count and got["obs_count"] == o.count else np.inf,
           "returns": ratio(np.abs(got["returns"] - twin.returns), 1e-12 + 1e-12 * np.abs(twin.returns))}
    if "mean_f32" in got:
        m32, s32 = twin.mirrors()
        out["mirrors"] = float(max(_ulps(got["mean_f32"], m32), _ulps(got["std_f32"], s32)))
    return out


VECNORM_MUTATIONS = ("short_block_counted_as_rows", "last_row_dropped", "last_partial_skipped", "returns_second_row_skipped")


def _chan(n, mean, m2, nb, mb, m2b):
    """`chan_merge`, elementwise: b passes where n == 0, nothing moves where nb == 0."""
    n, mean, m2, nb, mb, m2b = np.broadcast_arrays(n, mean, m2, nb, mb, m2b)
    with np.errstate(divide="ignore", invalid="ignore"):
        tot = n + nb
        delta = mb - mean
        merged_mean = mean + delta * (nb / tot)
        merged_m2 = m2 + (m2b + delta * delta * (n * nb / tot))
    keep, take = nb == 0, (n == 0) & (nb != 0)
    pick = lambda a, b, c: np.where(keep, a, np.where(take, b, c))  # noqa: E731
    return pick(n, nb, tot), pick(mean, mb, merged_mean), pick(m2, m2b, merged_m2)


def _tree(n, mean, m2):
    """`vecnorm_lds_tree` over axis -2 (the slots): slot p takes slot p + half in, half = ceil(live / 2), until one is left."""
    live = n.shape[-2]
    while live > 1:
        half = (live + 1) >> 1
        k = live - half
        a = _chan(n[..., :k, :], mean[..., :k, :], m2[..., :k, :], n[..., half:live, :], mean[..., half:live, :], m2[..., half:live, :])
        n, mean, m2 = (np.concatenate([x, y[..., k:half, :]], axis=-2) for x, y in zip(a, (n, mean, m2)))
        live = half
    return n[..., 0, :], mean[..., 0, :], m2[..., 0, :]


def _block_moments(x, envs, first_row_only=False):
    """The partial (mean [B, g], M2 [B, g]) of B blocks of `envs` envs each over a group of g columns (x: [B, envs, g] fp64)
    in the kernel's order: lane p takes rows p, p + slots, ..., 8 at a time, each chunk two-pass, Chan per lane, the tree."""
    B, _, g = x.shape
    slots = VECNORM_THREADS // g
    rows = lane_rows(envs, slots)
    if first_row_only:
        rows = np.minimum(rows, 1)
    K = max(int(rows.max()), 1)
    padded = np.zeros((B, K * slots, g), dtype=F64)
    take = min(envs, K * slots)
    padded[:, :take] = x[:, :take]
    lanes = padded.reshape(B, K, slots, g)
    n, mean, m2 = (np.zeros((B, slots, g), dtype=F64) for _ in range(3))
    for k0 in range(0, K, VECNORM_CHUNK):
        count = np.clip(rows - k0, 0, VECNORM_CHUNK)[None, :, None].astype(F64)
        chunk = [lanes[:, k0 + j] if k0 + j < K else np.zeros((B, slots, g)) for j in range(VECNORM_CHUNK)]
        total = np.zeros((B, slots, g), dtype=F64)
        for j in range(VECNORM_CHUNK):
            total = total + np.where(j < count, chunk[j], 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            cm = total / count
        q = np.zeros((B, slots, g), dtype=F64)
        for j in range(VECNORM_CHUNK):
            d = np.where(j < count, chunk[j] - cm, 0.0)
            q = q + d * d
        n, mean, m2 = _chan(n, mean, m2, count, np.where(count > 0, cm, 0.0), q)
    _, mean, m2 = _tree(n, mean, m2)
    return mean, m2


class VecnormOrderModel:
    """vecnorm_moments_kernel's statistics in numpy fp64, in the documented order: chunks of 8 reduced two-pass, Chan per
    lane, the fixed LDS tree, one partial per block, the last block's merge of the partials p, p + slots, ... and its tree,
    then RunningMeanStd's update as the kernel writes it. `mutation`: one of `VECNORM_MUTATIONS`."""

    def __init__(self, N, D, gamma=0.99, epsilon=1e-8, norm_obs=True, mutation=None):
        assert mutation is None or mutation in VECNORM_MUTATIONS
        self.N, self.D, self.gamma, self.epsilon, self.norm_obs, self.mutation = N, D, gamma, epsilon, norm_obs, mutation
        self.blocks, self.rows, _ = vecnorm_blocks(N, D)
        self.obs_mean, self.obs_var, self.obs_count = np.zeros(D), np.ones(D), 1e-4
        self.ret = [0.0, 1.0, 1e-4]
        self.returns = np.zeros(N, dtype=F64)

    def _batch(self, x, returns):
        """(n, mean, M2) per column of the whole batch x [N, g]."""
        N, rows, blocks = self.N, self.rows, self.blocks
        full, short = (blocks - 1) * rows, N - (blocks - 1) * rows
        g = x.shape[1]
        one = returns and self.mutation == "returns_second_row_skipped"
        mean, m2 = np.zeros((blocks, g)), np.zeros((blocks, g))
        if blocks > 1:
            mean[:-1], m2[:-1] = _block_moments(x[:full].reshape(blocks - 1, rows, g), rows, one)
        last = x[full:][None]
        if self.mutation == "last_row_dropped":
            last = last[:, :short - 1]
        mean[-1:], m2[-1:] = _block_moments(last, last.shape[1], one) if last.shape[1] else (0.0, 0.0)
        counts = np.full(blocks, float(rows))
        counts[-1] = float(rows if self.mutation == "short_block_counted_as_rows" else short)
        return counts, mean, m2

    def _merge(self, counts, mean, m2):
        """The last block: per group of at most 256 columns, slot p merges the partials p, p + slots, ..., then the tree."""
        blocks, cols = mean.shape
        out = [np.zeros(cols) for _ in range(3)]
        for c0 in range(0, cols, VECNORM_THREADS):
            g = min(cols - c0, VECNORM_THREADS)
            slots = min(blocks, VECNORM_THREADS // g)
            n, a, b = (np.zeros((slots, g)) for _ in range(3))
            per_slot = -(-(blocks - np.arange(slots)) // slots)
            for i in range(_ceil(blocks, slots)):
                idx = np.arange(slots) + i * slots
                live = idx < blocks
                if self.mutation == "last_partial_skipped":
                    live &= (i < per_slot - 1) | (per_slot == 1)
                idx = np.minimum(idx, blocks - 1)
                n, a, b = _chan(n, a, b, np.where(live, counts[idx], 0.0)[:, None], mean[idx, c0:c0 + g], m2[idx, c0:c0 + g])
            for dst, src in zip(out, _tree(n, a, b)):
                dst[c0:c0 + g] = src
        return out

    @staticmethod
    def _update(mean, var, count, bn, bm, bm2):
        delta, tot = bm - mean, count + bn
        return mean + delta * bn / tot, (var * count + bm2 + delta * delta * count * bn / tot) / tot

    def _launch(self, obs, x_ret):
        parts = []
        if obs is not None and self.norm_obs:
            parts += [self._batch(np.asarray(obs, dtype=F32).astype(F64)[:, c0:c0 + g], False) for c0, g, _ in column_groups(self.D, 0)]
        if x_ret is not None:
            parts.append(self._batch(x_ret[:, None], True))
        if not parts:
            return
        counts = parts[0][0]
        bn, bm, bm2 = self._merge(counts, np.concatenate([p[1] for p in parts], axis=1), np.concatenate([p[2] for p in parts], axis=1))
        if obs is not None and self.norm_obs:
            D = self.D
            self.obs_mean, self.obs_var = self._update(self.obs_mean, self.obs_var, self.obs_count, bn[:D], bm[:D], bm2[:D])
            self.obs_count += float(self.N)
        if x_ret is not None:
            self.ret[0], self.ret[1] = (float(v) for v in self._update(self.ret[0], self.ret[1], self.ret[2], bn[-1], bm[-1], bm2[-1]))
            self.ret[2] += float(self.N)

    def reset(self, obs):
        self._launch(obs, None)
        self.returns[:] = 0.0

    def step(self, obs, reward, terminated, truncated):
        done = np.asarray(terminated, dtype=bool) | np.asarray(truncated, dtype=bool)
        x = self.returns * self.gamma + np.asarray(reward, dtype=F32).astype(F64)
        self._launch(obs, x)
        kept = np.ones(self.N, dtype=bool)
        if self.mutation == "returns_second_row_skipped":  # (a returns lane stops behind its first row: the others keep their return)
            kept = (np.arange(self.N) % self.rows) < VECNORM_THREADS
        if self.mutation == "last_row_dropped":
            kept[-1] = False
        self.returns = np.where(kept, np.where(done, 0.0, x), self.returns)

    def stats(self):
        return {"obs_mean": self.obs_mean, "obs_var": self.obs_var, "obs_count": self.obs_count, "ret": tuple(self.ret), "returns": self.returns,
                "mean_f32": self.obs_mean.astype(F32), "std_f32": np.sqrt(self.obs_var + self.epsilon).astype(F32)}


def run_vecnorm_model(row, form, mutation=None):
    """The order model and the twin side by side over the row's steps in `form`: the worst error / bound per statistic
    over the steps ({name: ratio})."""
    obs, reward, term, trunc = vecnorm_inputs(row.N, row.D)
    model = VecnormOrderModel(row.N, row.D, norm_obs=form != "no_norm_obs", mutation=mutation)
    twin = twin_of(row.N, row.D, form)
    worst = {}

    def look():
        for k, v in stats_ratios(model.stats(), twin).items():
            worst[k] = max(worst.get(k, 0.0), v)

    if form == "reset_first":
        model.reset(obs[-1])
        twin.reset(obs[-1])
        look()
    for t in range(obs.shape[0]):
        model.step(obs[t], reward[t], term[t], trunc[t])
        twin.step(obs[t], reward[t], term[t], trunc[t])
        look()
    return worst
