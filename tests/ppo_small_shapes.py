"""The sizes the small kernels around the PPO gradient launch are tested at -- launch 0 and its data-parallel pair 0a / 0b
(`ppo_adv_stats_kernel`, `ppo_adv_partials_kernel`, `ppo_adv_finish_kernel`), `ppo_explained_variance_kernel`, launch B and
launch C (`ppo_fold_kernel`, `ppo_adam_kernel`; csrc/ppo.hpp) and `gae_kernel` (csrc/rollout.hpp) -- and what the tests share,
all plain numpy under seeds of the row: synthetic inputs, the plans restated from the headers, fp64 twins (`math.fsum`,
tests/ppo_reference.py's `adam_step`, tests/ppo_learn_reference.py's `explained_variance`, oracle/rollout_oracle.py's `gae`),
numpy models of the kernels' own order of operations with the mistakes a kernel could make (for the sharpness tests), and the
bounds, each stated once with its derivation.

tests/test_ppo_small_matrix.py asserts without a GPU that the tables cover what their `why`s claim and that the checks are
sharp; tests/test_ppo_small_matrix_gpu.py runs every row on the device. The gradient launch (launch A) has its own table,
tests/mlp_shapes.py."""

import functools
import math
from collections import namedtuple

import numpy as np

from oracle.rollout_oracle import gae as oracle_gae
from tests import ppo_reference as R
from tests.mlp_shapes import dims
from tests.ppo_learn_reference import explained_variance  # noqa: F401  (tests/test_ppo_small_matrix.py holds `ev_twin` to it)
from upkie_amd.policies import mlp_shape, pack_index

F32, F64 = np.float32, np.float64
U = 2.0 ** -53  # unit roundoff of fp64
H32 = 2.0 ** -24  # unit roundoff of fp32: a value stored as fp32 is within H32 |x| of what was to be stored

# enum values and loop shapes of csrc/ppo.hpp (tests/test_ppo_small_matrix.py reads them back from the header)
PPO_ADV_THREADS, PPO_SWEEP_LOADS, PPO_THREADS, PPO_STATS, FOLD_UNROLL = 1024, 8, 256, 4, 32
SWEEP = PPO_SWEEP_LOADS * PPO_ADV_THREADS  # samples one iteration of ppo_adv_pass / ppo_ev_pass takes: 8192
GAE_THREADS, GAE_UNROLL = 256, 8
SHARD_WORLDS = (1, 2, 3)  # the data-parallel forms run in one process with this many equal shards


def _ceil(a, b):
    return -(-a // b)


def sum_bound(terms, n=None):
    """An fp64 sum of n terms in ANY order is within n 2^-53 sum |term| of the exact sum (Higham, Accuracy and Stability of
    Numerical Algorithms, 4.2: (n - 1) u to first order for every summation tree; n u covers the higher orders for every n
    here). Every bound below on a device sum is this one, carried through the expressions that follow the sum."""
    terms = np.asarray(terms, dtype=F64)
    return (terms.size if n is None else n) * U * math.fsum(np.abs(terms).tolist())


def _tree(a):
    """`lds_tree_sum`: word t += word t + h, h = THREADS / 2 ... 1, over the last axis."""
    a = np.array(a, dtype=F64)
    h = a.shape[-1] // 2
    while h:
        a[..., :h] += a[..., h:2 * h]
        h //= 2
    return a[..., 0]


def _sweep_sum(x, sweeps=None):
    """`ppo_adv_pass` / `ppo_ev_pass` on the values x of samples 0 .. n - 1: thread t adds x[t], x[t + 1024], ... in that
    order (8 per iteration of its loop), then the 1024-word tree. `sweeps`: the loop stops after that many iterations."""
    x = np.asarray(x, dtype=F64)
    rows = _ceil(max(x.size, 1), PPO_ADV_THREADS)
    a = np.zeros(rows * PPO_ADV_THREADS)
    a[:x.size] = x
    a = a.reshape(rows, PPO_ADV_THREADS)
    if sweeps is not None:
        a = a[:sweeps * PPO_SWEEP_LOADS]
    s = np.zeros(PPO_ADV_THREADS)
    for row in a:
        s = s + row
    return float(_tree(s))


def _mean_and_squares(x):
    """(mean, sum of squared deviations, bound on a device mean, bound on a device sum of squares) of the fp64 values x, the
    exact sums by `math.fsum`.

    Mean: the device's sum is within n u sum|x| of the exact one, the division rounds once, and the twin's own mean is
    rounded twice: e = u sum|x| + 3 u |mean|. Squares: about a mean that is off by e the sum grows by n e^2 - 2 e sum(x - m),
    and sum(x - m) about the twin's mean is at most n u |mean|; each deviation and each square rounds once on either side
    (8 u Q in all) and the sum of n squares is within n u Q: bound = (n + 8) u Q + 2 n e^2 + 2 e n u |mean|."""
    n = x.size
    mean = math.fsum(x.tolist()) / n
    dev = x - mean
    q = math.fsum((dev * dev).tolist())
    e = U * math.fsum(np.abs(x).tolist()) + 3.0 * U * abs(mean)
    return mean, q, e, (n + 8) * U * q + 2.0 * n * e * e + 2.0 * e * n * U * abs(mean)


def ratio(err, bound):
    """error / bound, 0 where both are 0, inf where the error is not finite or exceeds a zero bound."""
    err, bound = np.asarray(err, dtype=F64), np.asarray(bound, dtype=F64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bound)
    r = np.where(np.isfinite(r), r, np.inf)
    return float(np.max(r, initial=0.0))


# ================================================================ launch 0, 0a, 0b: advantage statistics
AdvRow = namedtuple("AdvRow", "total batch why")

ADV_ROWS = [
    AdvRow(2, 2, "the smallest minibatch that is normalised"),
    AdvRow(3, 3, "three samples: one live lane more than the n = 2 path"),
    AdvRow(1023, 1023, "one thread of the block idle"),
    AdvRow(1024, 1024, "every thread one sample"),
    AdvRow(1025, 1025, "thread 0 takes a second sample"),
    AdvRow(8191, 8191, "one sample short of a full sweep of 8 x 1024"),
    AdvRow(8192, 8192, "exactly one full sweep"),
    AdvRow(8193, 8193, "a second sweep with one live lane"),
    AdvRow(16385, 16385, "a third sweep with one live lane"),
    AdvRow(2 * 8193 + 1, 8193, "M = 3 with two-sweep minibatches; the last minibatch has exactly 1 sample: (0, 1)"),
    AdvRow(2 * 1025 + 2, 1025, "M = 3, the last minibatch has 2 samples"),
    AdvRow(1024 + 1023, 1024, "M = 2, the last minibatch has batch - 1"),
    AdvRow(1, 1, "one sample in all: (0, 1)"),
    AdvRow(256 * 3 + 2, 3, "M = 257: launch 0b's second block has one live thread; the last minibatch has 2 samples"),
    AdvRow(65537, 65537, "a workload-sized minibatch (B T / 4 of examples/ppo_learn.py) plus one: nine sweeps"),
]
ADV_IDS = [f"{r.total}-{r.batch}" for r in ADV_ROWS]
ADV_GUARD = 4  # words behind `out` that must stay as they were


def adv_plan(row):
    """What the kernels' loops do at this row: M, every minibatch's size, the sweeps of the largest, launch 0b's blocks."""
    M = _ceil(row.total, row.batch)
    sizes = [min(row.batch, row.total - j * row.batch) for j in range(M)]
    return {"M": M, "sizes": sizes, "last": sizes[-1], "sweeps": _ceil(max(sizes), SWEEP), "finish_blocks": _ceil(M, PPO_THREADS),
            "finish_last_block_threads": M - (_ceil(M, PPO_THREADS) - 1) * PPO_THREADS}


@functools.lru_cache(maxsize=None)
def adv_inputs(row, shard=0):
    """(advantages fp32 with mean 1e3 and standard deviation 1, a shuffle of range(total) as int32) of one shard."""
    rng = np.random.default_rng([row.total, row.batch, shard])
    adv = rng.normal(1e3, 1.0, size=row.total).astype(F32)
    perm = rng.permutation(row.total).astype(np.int32)
    adv.setflags(write=False)
    perm.setflags(write=False)
    return adv, perm


@functools.lru_cache(maxsize=None)
def adv_twin(row, world=1, normalize=1):
    """(out [M, 2], bound [M, 2]): (mean, std + 1e-8) of minibatch j over the union of `world` shards, unbiased, by exact
    sums; (0, 1) exactly without normalisation or with fewer than 2 samples.

    std = sqrt(Q / (n - 1)) + 1e-8: the relative bound of Q halves under the root, and the division, the root and the sum
    round once on either side: bound = std (bound(Q) / (2 Q) + 6 u)."""
    plan = adv_plan(row)
    out, bound = np.zeros((plan["M"], 2)), np.zeros((plan["M"], 2))
    for j, n in enumerate(plan["sizes"]):
        start = j * row.batch
        x = np.concatenate([a[p[start:start + n]] for a, p in (adv_inputs(row, s) for s in range(world))]).astype(F64)
        if not normalize or x.size < 2:
            out[j] = 0.0, 1.0
            continue
        mean, q, e, qb = _mean_and_squares(x)
        std = math.sqrt(q / (x.size - 1)) + 1e-8
        assert q > 0.0
        out[j] = mean, std
        bound[j] = e, std * (0.5 * qb / q + 6.0 * U)
    return out, bound


ADV_MUTATIONS = ("sweep_once", "guard_minus_one", "guard_plus_one", "last_takes_batch", "start_at_j_times_n", "ddof_0", "one_pass",
                 "perm_ignored", "mean_over_n", "slot_stride_M")


def adv_mutation_shows(row, world, mutation):
    """Whether the plan lets the mistake move an output of this row run with `world` shards (n: a shard's minibatch); None
    where the plan alone cannot tell."""
    plan = adv_plan(row)
    sizes = plan["sizes"]
    normalised = [n for n in sizes if world * n >= 2]
    short = plan["M"] > 1 and plan["last"] < row.batch
    return {
        "sweep_once": any(n > SWEEP for n in normalised),
        "guard_minus_one": bool(normalised),
        "guard_plus_one": bool(normalised),
        "last_takes_batch": short,  # (a one-sample last block becomes a normalised one)
        "start_at_j_times_n": short and world * plan["last"] >= 2,
        "ddof_0": bool(normalised),
        # sum x^2 - (sum x)^2 / n over 2 or 4 fp32 values near 1e3 is exact in 53 bits (squares of 24-bit words, the square
        # of a 26-bit sum, a division by a power of two); from 33 values on the sum of 48-bit squares cannot be; between the
        # two it depends on the values' low bits (None: no claim)
        "one_pass": True if any(world * n > 32 for n in sizes) else False if all(world * n in (1, 2, 4) for n in sizes) else None,
        "perm_ignored": plan["M"] > 1 and bool(normalised),  # (with one minibatch the same samples in another order)
        "mean_over_n": world > 1 and bool(normalised),
        "slot_stride_M": world > 1 and bool(normalised),
    }[mutation]


def adv_model(row, world=1, normalize=1, mutation=None):
    """Launches 0a (phase 0), 0a (phase 1) and 0b on `world` shards in fp64 numpy in the kernels' order; with one shard this
    is launch 0's arithmetic. `mutation`: one of `ADV_MUTATIONS`. A read past an array's end gives 0."""
    assert mutation is None or mutation in ADV_MUTATIONS
    M = _ceil(row.total, row.batch)
    stride = M if mutation == "slot_stride_M" else 2 * M
    slots = np.zeros(world * 2 * M + 2 * M)
    squares = np.zeros((world, M))  # (one_pass only: the sums of x^2)

    def block(j):
        start = j * row.batch
        n = min(row.batch, row.total - start)
        if mutation == "last_takes_batch":
            n = row.batch
        if mutation == "start_at_j_times_n":
            start = j * n
        return start, n

    def samples(shard, start, n):
        adv, perm = adv_inputs(row, shard)
        live = n + {"guard_minus_one": -1, "guard_plus_one": 1}.get(mutation, 0)
        at = start + np.arange(max(live, 0))
        inside = at < row.total
        at = np.minimum(at, row.total - 1)
        index = at if mutation == "perm_ignored" else perm[at]
        return np.where(inside, adv[index].astype(F64), 0.0)

    sweeps = 1 if mutation == "sweep_once" else None
    for r in range(world):
        for j in range(M):
            x = samples(r, *block(j))
            slots[r * 2 * M + j] = _sweep_sum(x, sweeps)
            squares[r, j] = _sweep_sum(x * x, sweeps)
    for r in range(world):
        for j in range(M):
            start, n = block(j)
            g = slots[j]
            for s in range(1, world):
                g += slots[s * stride + j]
            mean = g / (n if mutation == "mean_over_n" else float(world) * n)
            x = samples(r, start, n) - mean
            slots[r * 2 * M + M + j] = _sweep_sum(x * x, sweeps)
    out = np.zeros((M, 2))
    for j in range(M):
        _, n = block(j)
        cnt = float(world) * n
        if not normalize or cnt < 2.0:
            out[j] = 0.0, 1.0
            continue
        g, q = slots[j], slots[M + j]
        for s in range(1, world):
            g, q = g + slots[s * stride + j], q + slots[s * stride + M + j]
        mean = g / cnt
        if mutation == "one_pass":
            q = float(squares[:, j].sum()) - g * g / cnt
        with np.errstate(invalid="ignore"):
            out[j] = mean, np.sqrt(q / (cnt if mutation == "ddof_0" else cnt - 1.0)) + 1e-8
    return out


def adv_ratio(got, row, world=1, normalize=1):
    """The worst error / bound of an [M, 2] result against the twin; where the twin says (0, 1) the bits must be those."""
    want, bound = adv_twin(row, world, normalize)
    return ratio(np.abs(np.asarray(got, dtype=F64) - want), bound)


# ================================================================ explained variance
EvRow = namedtuple("EvRow", "n kind why")

EV_ROWS = [
    EvRow(1, "plain", "one sample: Var(returns) = 0, NaN"),
    EvRow(2, "plain", "two samples"),
    EvRow(1025, "plain", "thread 0 takes a second sample"),
    EvRow(8192, "plain", "exactly one full sweep"),
    EvRow(8193, "plain", "a second sweep with one live lane"),
    EvRow(16385, "plain", "a third sweep with one live lane"),
    EvRow(262151, "plain", "a rollout-sized buffer, odd: 33 sweeps, the last with 7 samples"),
    EvRow(8193, "constant", "constant returns: NaN"),
    EvRow(8193, "equal", "values equal to returns: exactly 1.0"),
    EvRow(8193, "mean_1e3", "returns with mean 1e3: a one-pass variance loses 6 digits"),
]
EV_IDS = [f"{r.n}-{r.kind}" for r in EV_ROWS]
EV_KINDS = ("plain", "constant", "equal", "mean_1e3")


@functools.lru_cache(maxsize=None)
def ev_inputs(row, shard=0):
    """(returns, values) fp32 of one shard."""
    rng = np.random.default_rng([row.n, EV_KINDS.index(row.kind), shard])
    ret = rng.normal(1e3 if row.kind == "mean_1e3" else 0.5, 2.0, size=row.n).astype(F32)
    val = (ret.astype(F64) * (1.0 if row.kind == "mean_1e3" else 0.8) + rng.normal(0.0, 0.7, size=row.n)).astype(F32)
    if row.kind == "constant":
        ret[:] = 1.5
    if row.kind == "equal":
        val = ret.copy()
    ret.setflags(write=False)
    val.setflags(write=False)
    return ret, val


@functools.lru_cache(maxsize=None)
def ev_twin(row, world=1):
    """(1 - Var(returns - values) / Var(returns), its bound) over the union of `world` shards, population variances by
    exact sums, NaN when Var(returns) == 0. returns - values is one fp64 subtraction on both sides: the same bits.

    Both variances divide by the same count, so the ratio is Qd / Qy: bound = (Qd / Qy) (bound(Qd) / Qd + bound(Qy) / Qy +
    6 u) + 2 u max(1, |result|) for the two divisions, the subtraction and the twin's own three roundings."""
    parts = [ev_inputs(row, s) for s in range(world)]
    y = np.concatenate([r for r, _ in parts]).astype(F64)
    d = y - np.concatenate([v for _, v in parts]).astype(F64)
    _, qy, _, qyb = _mean_and_squares(y)
    _, qd, _, qdb = _mean_and_squares(d)
    if qy / y.size == 0.0:
        return float("nan"), 0.0
    value = 1.0 - (qd / y.size) / (qy / y.size)
    rel = (qdb / qd if qd else 0.0) + qyb / qy + 6.0 * U
    return value, (qd / qy) * rel + 2.0 * U * max(1.0, abs(value))


EV_MUTATIONS = ("sweep_once", "guard_minus_one", "guard_plus_one", "mean_over_n")


def ev_mutation_shows(row, world, mutation):
    if row.kind in ("constant", "equal") or world * row.n < 3:
        return False  # (the special inputs are held to exact values; two samples less one are constant returns)
    return {"sweep_once": row.n > SWEEP, "guard_minus_one": True, "guard_plus_one": True, "mean_over_n": world > 1}[mutation]


def ev_model(row, world=1, mutation=None):
    """Phases 0, 1 and 2 on `world` shards (phase -1 with one) in fp64 numpy in the kernel's order."""
    assert mutation is None or mutation in EV_MUTATIONS
    sweeps = 1 if mutation == "sweep_once" else None
    live = row.n + {"guard_minus_one": -1, "guard_plus_one": 1}.get(mutation, 0)

    def samples(shard):
        ret, val = (np.concatenate([a.astype(F64), [0.0]])[:live] for a in ev_inputs(row, shard))
        return ret, ret - val

    cnt = float(world) * row.n
    sy = sd = qy = qd = 0.0
    for r in range(world):
        y, d = samples(r)
        sy, sd = sy + _sweep_sum(y, sweeps), sd + _sweep_sum(d, sweeps)
    over = float(row.n) if mutation == "mean_over_n" else cnt
    for r in range(world):
        y, d = samples(r)
        qy, qd = qy + _sweep_sum((y - sy / over) ** 2, sweeps), qd + _sweep_sum((d - sd / over) ** 2, sweeps)
    var_y, var_d = qy / cnt, qd / cnt
    return float("nan") if var_y == 0.0 else 1.0 - var_d / var_y


def ev_ratio(got, row, world=1):
    want, bound = ev_twin(row, world)
    if math.isnan(want) or math.isnan(got):
        return 0.0 if math.isnan(want) and math.isnan(got) else float("inf")
    if row.kind == "equal":
        return 0.0 if got == 1.0 else float("inf")
    return ratio(abs(got - want), bound)


# ================================================================ launch B and launch C: fold, clip, Adam
FoldRow = namedtuple("FoldRow", "obs_dim actor act_dim critic world why")

FOLD_SHAPES = [
    ((1, (1,), 1, (1,)), "the smallest shape: 600 trainable words, 3 fold blocks"),
    ((3, (16,), 2, (16,)), "one full tile per layer"),
    ((5, (40, 24), 3, (40, 24)), "train_off 48; 26 blocks, the last with 20 words"),
    ((30, (256, 256, 128), 36, (256, 256, 128)), "870 blocks: the last block's sum over the blocks' squares is long"),
]
FOLD_WORLDS = {1: "the scalar tail alone", 2: "two slots", 31: "the longest tail without a body", 32: "one unrolled body, no tail",
               33: "a body and a one-slot tail", 64: "two bodies, no tail", 65: "two bodies and a one-slot tail"}
FOLD_ROWS = [FoldRow(*shape, world, f"{why}; {FOLD_WORLDS[world]}")
             for i, (shape, why) in enumerate(FOLD_SHAPES) for world in (FOLD_WORLDS if i < 2 else (1, 33))]
FOLD_IDS = [f"{r.obs_dim}-{list(r.actor)}-{r.act_dim}-w{r.world}".replace(" ", "") for r in FOLD_ROWS]
FOLD_APPLIES = 3  # consecutive applies per row: t = 1, 2, 3
FOLD_NORMS = (2.0, 0.1, 0.8)  # the norm of each apply's folded gradient: above, below and above max_grad_norm
FOLD_MAX_MINIBATCH = 64  # sizes the workspace (its partials are not used by an apply: the slots are)
GRAPHED_FOLD_ROW = (5, 33)  # (obs_dim, world)
CONTROLLED_FOLD_ROW = (3, 2)
# the configuration as UpkiePpoConfig stores it (fp32) and the twin's constants: the same values as fp64
CFG32 = {k: F32(v) for k, v in dict(ent_coef=0.01, vf_coef=0.5, max_grad_norm=0.5, beta1=0.9, beta2=0.999, eps=1e-5).items()}
CFG = {k: float(v) for k, v in CFG32.items()}
LR = 3e-4
HALF_LOG_2PI = 0.91893853320467274
SMALL_TENSOR = 16  # words; see `adam_bounds`


def fold_shape(row):
    return mlp_shape(dims(row.obs_dim, row.actor, row.act_dim), dims(row.obs_dim, row.critic, 1), "tanh")


def fold_count(row):
    """`global_minibatch_size` of the row's applies: a number no other count of the row equals."""
    return 1000 + row.world


@functools.lru_cache(maxsize=None)
def fold_plan(row):
    """tests/ppo_reference.py's plan of the shape, the slot layout (`ppo_slot_stats_at`, `ppo_slot_words`), the workspace
    offsets of an apply, launch B's loop at this `world`, and the map of the trainable words: `tensor[i]` is the source
    tensor of trainable word i (0 log_std, then weight and bias per layer, actor then critic), -1 for padding."""
    shape = fold_shape(row)
    p = dict(R.plan(shape))
    words = p["train_words"]
    sizes = [row.obs_dim, row.obs_dim, row.act_dim, row.act_dim, row.act_dim]
    for d_in, widths, d_out in ((row.obs_dim, row.actor, row.act_dim), (row.obs_dim, row.critic, 1)):
        for out, n in dims(d_in, widths, d_out):
            sizes += [out * n, out]
    index = pack_index(shape, sizes)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    tensor = np.searchsorted(starts, index, side="right") - 1 - 4
    tensor[index == starts[-1]] = -1
    assert index.size == p["train_off"] + words and (tensor[:p["train_off"]] < 0).all()
    grid = R.grid(p, FOLD_MAX_MINIBATCH)
    grad_at = R.HEADER_BYTES + 4 * grid * words + 8 * grid * R.STATS
    p.update(words=int(index.size), tensor=tensor[p["train_off"]:], tensors=len(sizes) - 4, slot_stats_at=(words + 1) & ~1,
             slot_words=((words + 1) & ~1) + 2 * PPO_STATS, last_block=words - (p["fold_blocks"] - 1) * PPO_THREADS,
             body=row.world // FOLD_UNROLL * FOLD_UNROLL, tail=row.world % FOLD_UNROLL, grad_at=grad_at, sq_at=grad_at + 4 * words,
             workspace_bytes=R.workspace_bytes(p, FOLD_MAX_MINIBATCH))
    p["tensor"].setflags(write=False)
    return p


FoldInputs = namedtuple("FoldInputs", "slots sums packed m v")


@functools.lru_cache(maxsize=8)
def fold_inputs(row):
    """slots [applies, world, slot_words] fp32: per slot a synthetic gradient (padding words zero, as launch A leaves them)
    scaled so that the folded norm is `FOLD_NORMS` (up to fp32 rounding and the entropy term), then PPO_STATS fp64 loss sums; `sums` [applies, world, 4] holds
    those again as fp64. packed, m, v [words] fp32: the fixed words random, the trainable ones non-zero on the real words
    (m and v of the size a clipped gradient leaves) and zero on padding; m and v before `train_off` hold 7, which nothing
    may touch."""
    p = fold_plan(row)
    rng = np.random.default_rng([row.obs_dim, row.act_dim, row.world, len(row.actor)])
    real = p["tensor"] >= 0
    n_real, words, W = int(real.sum()), p["train_words"], row.world
    slots = np.zeros((FOLD_APPLIES, W, p["slot_words"]), dtype=F32)
    sums = np.zeros((FOLD_APPLIES, W, PPO_STATS))
    count = fold_count(row)
    for k in range(FOLD_APPLIES):
        g = np.where(real, rng.normal(0.0, 1.0, size=(W, words)), 0.0)
        slots[k, :, :words] = g * (FOLD_NORMS[k] / np.linalg.norm(g.sum(axis=0)))
        sums[k, :, 0] = rng.normal(0.1, 1.0, size=W) * count / W
        sums[k, :, 1] = np.abs(rng.normal(0.0, 1.0, size=W)) * count / W
        sums[k, :, 2] = np.abs(rng.normal(0.0, 0.004, size=W)) * count / W
        sums[k, :, 3] = rng.integers(0, count // W + 1, size=W)
        for r in range(W):
            slots[k, r, p["slot_stats_at"]:].view(F64)[:] = sums[k, r]
    scale = CFG["max_grad_norm"] / math.sqrt(n_real)
    packed, m, v = (np.zeros(p["words"], dtype=F32) for _ in range(3))
    packed[:p["train_off"]] = rng.normal(0.0, 1.0, size=p["train_off"])
    m[:p["train_off"]] = v[:p["train_off"]] = 7.0
    packed[p["train_off"]:] = np.where(real, rng.normal(0.0, 0.3, size=words), 0.0)
    packed[p["train_off"]:p["train_off"] + row.act_dim] = rng.normal(-0.5, 0.1, size=row.act_dim)  # log_std
    m[p["train_off"]:] = np.where(real, rng.normal(0.0, scale, size=words), 0.0)
    v[p["train_off"]:] = np.where(real, rng.uniform(0.5, 1.5, size=words) * scale * scale, 0.0)
    for a in (slots, sums, packed, m, v):
        a.setflags(write=False)
    return FoldInputs(slots, sums, packed, m, v)


FOLD_MUTATIONS = ("tail_dropped", "tail_first", "entropy_on_no_word", "entropy_on_one_word_more", "norm_before_entropy", "coef_not_applied",
                  "t_for_t_plus_1", "bc2_inside_the_root", "m_v_written_at_i", "stats_over_world")


def fold_mutation_shows(row, mutation):
    p = fold_plan(row)
    return {"tail_dropped": p["tail"] > 0, "tail_first": p["tail"] > 0 and p["body"] > 0}.get(mutation, True)


def fold_gradient(row, k, mutation=None):
    """Launch B's gradient of apply k: word i of the slots summed in slot order in fp32 from 0 (plain adds: nothing can
    contract, so the device's words have these bits), less ent_coef on log_std's words. Also the sum before the entropy
    term."""
    p, slots = fold_plan(row), fold_inputs(row).slots[k]
    order = list(range(row.world))
    if mutation == "tail_dropped":
        order = order[:p["body"]]
    if mutation == "tail_first":
        order = order[p["body"]:] + order[:p["body"]]
    s = np.zeros(p["train_words"], dtype=F32)
    for b in order:
        s = s + slots[b, :p["train_words"]]
    assert s.dtype == F32
    folded = s.copy()
    on = {"entropy_on_no_word": 0, "entropy_on_one_word_more": row.act_dim + 1}.get(mutation, row.act_dim)
    s[:on] = s[:on] - CFG32["ent_coef"]
    return s, folded


def fold_statistics(row, k, grad, log_std, exact=True, divisor=None, sums=None):
    """The statistics row [7] of apply k in fp64 (policy loss, value loss, entropy loss, loss, approx_kl, clip fraction,
    ||g||) from the slots' loss sums, the current log_std words and the folded gradient `grad`: by exact sums, or
    (`exact=False`) in launch B's order: the squares per block of 256 through the tree and then in block order, the loss
    sums in slot order. With the exact sums, also the bound of every entry. `sums` [world, 4]: loss sums other than the
    row's own (the controlled form's test writes its own approx_kl)."""
    sums = fold_inputs(row).sums[k] if sums is None else np.asarray(sums, dtype=F64)
    n = float(fold_count(row) if divisor is None else divisor)
    g = np.asarray(grad, dtype=F32).astype(F64)
    ent_terms = 0.5 + HALF_LOG_2PI + np.asarray(log_std, dtype=F32).astype(F64)
    if exact:
        total = [math.fsum(sums[:, c].tolist()) for c in range(PPO_STATS)]
        square = math.fsum((g * g).tolist())
        entropy = math.fsum(ent_terms.tolist())
    else:
        total = [float(np.cumsum(sums[:, c])[-1]) for c in range(PPO_STATS)]
        blocks = _ceil(g.size, PPO_THREADS)
        sq = np.zeros(blocks * PPO_THREADS)
        sq[:g.size] = g * g
        square = float(np.cumsum(_tree(sq.reshape(blocks, PPO_THREADS)))[-1])
        entropy = float(np.cumsum(ent_terms)[-1])
    pg, vl, ent_loss = -total[0] / n, total[1] / n, -entropy
    loss = pg + CFG["ent_coef"] * ent_loss + CFG["vf_coef"] * vl
    stats = np.array([pg, vl, ent_loss, loss, total[2] / n, total[3] / n, math.sqrt(square)])
    if not exact:
        return stats
    # every sum by `sum_bound`, a division or a root once more on either side; the loss adds its three terms' bounds and
    # rounds four times on either side; the root halves the relative bound of the sum of squares
    b = [sum_bound(sums[:, c]) / n + 2.0 * U * abs(s) for c, s in zip(range(PPO_STATS), (pg, vl, total[2] / n, total[3] / n))]
    b_ent = sum_bound(ent_terms) + 2.0 * U * abs(entropy)
    b_loss = b[0] + CFG["ent_coef"] * b_ent + CFG["vf_coef"] * b[1] + 8.0 * U * (abs(pg) + abs(CFG["ent_coef"] * ent_loss) + abs(CFG["vf_coef"] * vl))
    b_norm = stats[6] * (0.5 * sum_bound(g * g) / square + 2.0 * U) if square else 0.0
    bound64 = np.array([b[0], b[1], b_ent, b_loss, b[2], b[3], b_norm])
    # the row is stored as fp32: half an ulp more, and the smallest subnormal where that is nothing
    return stats, bound64 + H32 * (1.0 + 2.0 ** -20) * np.abs(stats) + 2.0 ** -149


def adam_twin(row, grad, packed, m, v, t):
    """tests/ppo_reference.py's `adam_step` on the trainable words: (packed, m, v, t) after it, fp64, from the fp32 state and
    gradient as they are, with the configuration's fp32 constants as fp64 values."""
    off = fold_plan(row)["train_off"]
    as64 = lambda a: np.asarray(a, dtype=F32).astype(F64)  # noqa: E731
    p1, m1, v1, t1 = R.adam_step([as64(packed)[off:]], [as64(grad)], [as64(m)[off:]], [as64(v)[off:]], int(t), CFG["max_grad_norm"], LR,
                                 CFG["beta1"], CFG["beta2"], CFG["eps"])
    return p1[0], m1[0], v1[0], t1


def _per_tensor(p, got, want):
    """Relative Frobenius distance of every source tensor's words."""
    out = np.zeros(p["tensors"])
    for i in range(p["tensors"]):
        at = p["tensor"] == i
        out[i] = np.linalg.norm(got[at] - want[at]) / max(np.linalg.norm(want[at]), 1e-300)
    return out


@functools.lru_cache(maxsize=None)
def adam_bounds(row):
    """Per apply the bounds {"m", "v", "delta"} -> [tensors] on the relative Frobenius distance of a tensor's m, v and weight
    delta (word after - word before) from `adam_twin`, the measured distances they come from, and the floors of the small
    tensors: bound = 4 max(measured, floor).

    The rule of tests/mlp_shapes.py: four times the distance of torch fp32 from the fp64 twin on the same row. Here:
    `torch.optim.Adam(eps=1e-5)` behind `clip_grad_norm_(0.5)` in fp32 on the CPU, from the row's m, v and words, fed the
    row's folded gradients for the three applies, each step held to the twin on torch's own state before it. A tensor of
    fewer than `SMALL_TENSOR` words (the smallest shape has only one-word tensors) is a handful of draws of a rounding
    error, and a draw can be 0; there the distance is at least what storing the result in fp32 alone costs, whoever
    computes it: half an ulp of every word, 2^-24 relative for m and v, 2^-24 ||word|| / ||delta|| for the delta."""
    import torch

    p, inp = fold_plan(row), fold_inputs(row)
    off = p["train_off"]
    param = torch.tensor(inp.packed[off:].copy(), requires_grad=True)
    opt = torch.optim.Adam([param], lr=LR, betas=(0.9, 0.999), eps=1e-5)
    opt.state[param] = {"step": torch.tensor(0.0), "exp_avg": torch.tensor(inp.m[off:].copy()), "exp_avg_sq": torch.tensor(inp.v[off:].copy())}
    small = np.array([(p["tensor"] == i).sum() < SMALL_TENSOR for i in range(p["tensors"])])
    bounds, measured, floors = [], [], []
    for k in range(FOLD_APPLIES):
        grad, _ = fold_gradient(row, k)
        state = opt.state[param]
        before = [np.concatenate([np.zeros(off, dtype=F32), x.detach().numpy().copy()]) for x in (param, state["exp_avg"], state["exp_avg_sq"])]
        param.grad = torch.tensor(grad.copy())
        torch.nn.utils.clip_grad_norm_([param], float(CFG["max_grad_norm"]))
        opt.step()
        p1, m1, v1, _ = adam_twin(row, grad, *before, k)
        p0 = before[0][off:].astype(F64)
        after = [x.detach().numpy().astype(F64) for x in (param, state["exp_avg"], state["exp_avg_sq"])]
        dist = {"m": _per_tensor(p, after[1], m1), "v": _per_tensor(p, after[2], v1), "delta": _per_tensor(p, after[0] - p0, p1 - p0)}
        grid = {"m": np.full(p["tensors"], H32), "v": np.full(p["tensors"], H32),
                "delta": np.array([H32 * np.linalg.norm(p1[p["tensor"] == i]) / np.linalg.norm((p1 - p0)[p["tensor"] == i]) for i in range(p["tensors"])])}
        measured.append(dist)
        floors.append({q: np.where(small, grid[q], 0.0) for q in dist})
        bounds.append({q: 4.0 * np.maximum(dist[q], floors[-1][q]) for q in dist})
    return bounds, measured, floors


def apply_model(row, k, state, mutation=None):
    """Launch B and launch C of apply k on `state` = (packed, m, v, t) in the kernels' own arithmetic: the fold in fp32, the
    sums in fp64 in launch B's order, coef, the step size and sqrt(1 - beta2^t) rounded to fp32 as the header holds them,
    Adam in fp32. Returns (gradient, statistics row fp32, (packed, m, v, t) after). `mutation`: one of `FOLD_MUTATIONS`."""
    assert mutation is None or mutation in FOLD_MUTATIONS
    p = fold_plan(row)
    off, words = p["train_off"], p["train_words"]
    packed, m, v = (np.array(a, dtype=F32) for a in state[:3])
    t = int(state[3])
    grad, folded = fold_gradient(row, k, mutation)
    divisor = row.world if mutation == "stats_over_world" else None
    stats = fold_statistics(row, k, folded if mutation == "norm_before_entropy" else grad, packed[off:off + row.act_dim], exact=False, divisor=divisor)
    coef = F32(min(1.0, CFG["max_grad_norm"] / (stats[6] + 1e-6)))
    t += 1
    tt = t - 1 if mutation == "t_for_t_plus_1" else t
    b1, b2, eps = CFG32["beta1"], CFG32["beta2"], CFG32["eps"]
    with np.errstate(divide="ignore", invalid="ignore"):
        step = F32(F64(LR) / F64(1.0 - CFG["beta1"] ** tt))
        bc2 = F32(np.sqrt(F64(1.0 - CFG["beta2"] ** tt)))
        g = grad if mutation == "coef_not_applied" else grad * coef
        m1 = b1 * m[off:] + (F32(1.0) - b1) * g
        v1 = b2 * v[off:] + (F32(1.0) - b2) * g * g
        denom = np.sqrt(v1 / bc2) + eps if mutation == "bc2_inside_the_root" else np.sqrt(v1) / bc2 + eps
        packed[off:] = packed[off:] - step * (m1 / denom)
    at = 0 if mutation == "m_v_written_at_i" else off
    m[at:at + words], v[at:at + words] = m1, v1
    assert packed.dtype == m.dtype == v.dtype == F32
    return grad, stats.astype(F32), (packed, m, v, t)


def apply_ratios(row, k, before, gradient, stats, after, sums=None, stepped=True):
    """Every check on one apply, for the device's outputs and the models' alike, as error / bound (inf where bits that must
    be equal are not): `before` and `after` = (packed, m, v, t) around the apply, `gradient` the workspace's folded gradient,
    `stats` the row [7]. The twins are fed the state before the apply and the exact folded gradient. `stepped=False`: an
    apply of the controlled form that stops before its step writes the gradient and the row and leaves t and every word of
    packed, m and v as they were."""
    p, inp = fold_plan(row), fold_inputs(row)
    off = p["train_off"]
    want_grad, _ = fold_gradient(row, k)
    want_stats, stats_bound = fold_statistics(row, k, want_grad, np.asarray(before[0])[off:off + row.act_dim], sums=sums)
    p1, m1, v1, t1 = adam_twin(row, want_grad, *before[:3], before[3])
    bounds = adam_bounds(row)[0][k]
    packed, m, v = (np.asarray(a, dtype=F32) for a in after[:3])
    pad = p["tensor"] < 0
    same = lambda a, b: 0.0 if np.array_equal(np.asarray(a, dtype=F32).view(np.uint32), np.asarray(b, dtype=F32).view(np.uint32)) else float("inf")  # noqa: E731
    p0 = np.asarray(before[0], dtype=F32)[off:].astype(F64)
    if not stepped:
        return {"gradient": same(gradient, want_grad), "stats": ratio(np.abs(np.asarray(stats, dtype=F64) - want_stats), stats_bound),
                "unchanged": max([same(a, b) for a, b in zip(after[:3], before[:3])] + [0.0 if int(after[3]) == int(before[3]) else float("inf")])}
    out = {"gradient": same(gradient, want_grad),
           "stats": ratio(np.abs(np.asarray(stats, dtype=F64) - want_stats), stats_bound),
           "t": 0.0 if int(after[3]) == t1 else float("inf"),
           "padding": 0.0 if not (packed[off:][pad].any() or m[off:][pad].any() or v[off:][pad].any()) else float("inf"),
           "fixed": max(same(packed[:off], inp.packed[:off]), same(m[:off], inp.m[:off]), same(v[:off], inp.v[:off]))}
    for name, got, want in (("m", m[off:].astype(F64), m1), ("v", v[off:].astype(F64), v1), ("delta", packed[off:].astype(F64) - p0, p1 - p0)):
        out[name] = ratio(_per_tensor(p, got, want), bounds[name])
    return out


def run_apply_model(row, mutation=None):
    """The three applies of a row through `apply_model`: per apply the ratios of `apply_ratios`, and the coefficients."""
    inp = fold_inputs(row)
    state = (inp.packed, inp.m, inp.v, 0)
    ratios, coefs = [], []
    for k in range(FOLD_APPLIES):
        grad, stats, after = apply_model(row, k, state, mutation)
        ratios.append(apply_ratios(row, k, state, grad, stats, after))
        coefs.append(min(1.0, CFG["max_grad_norm"] / (float(stats[6]) + 1e-6)))
        state = after
    return ratios, coefs


# ================================================================ generalized advantage estimation
GaeRow = namedtuple("GaeRow", "T N gamma lam starts why")

GAE_ROWS = [
    GaeRow(1, 257, 0.99, 0.95, "dense", "one step: only the remainder loop, only last_values and last_dones"),
    GaeRow(2, 257, 1.0, 1.0, "dense", "two steps; no discount, so nothing hides a wrong factor"),
    GaeRow(7, 257, 0.9, 0.0, "dense", "T % 8 = 7: the longest remainder and no unrolled body; lambda = 0"),
    GaeRow(8, 257, 0.99, 0.95, "dense", "T % 8 = 0: one unrolled body, no remainder"),
    GaeRow(9, 257, 1.0, 1.0, "dense", "T % 8 = 1: a body and a remainder of one"),
    GaeRow(17, 257, 0.9, 0.0, "dense", "two bodies and a remainder of one"),
    GaeRow(9, 1, 0.99, 0.95, "dense", "one env: one live lane"),
    GaeRow(9, 255, 0.9, 0.0, "dense", "one block, its last lane idle"),
    GaeRow(9, 256, 1.0, 1.0, "dense", "exactly one block"),
    GaeRow(9, 513, 0.99, 0.95, "dense", "three blocks, the last with one env"),
    GaeRow(17, 256, 0.99, 0.95, "every_step", "an episode start at every step: no advantage is carried"),
]
GAE_IDS = [f"T{r.T}-N{r.N}-{r.starts}" for r in GAE_ROWS]
GAE_RTOL, GAE_ATOL = 1e-5, 2e-5  # tests/test_rollout.py's
GAE_GUARD = 64  # NaN words before and after each output


@functools.lru_cache(maxsize=None)
def gae_inputs(row):
    """rewards, values [T, N] fp32, episode_starts [T, N] bytes (p = 0.3, or all set), last_values [N], last_dones [N]."""
    rng = np.random.default_rng([row.T, row.N, len(row.starts)])
    rewards = rng.normal(0.5, 1.0, size=(row.T, row.N)).astype(F32)
    values = rng.normal(0.0, 1.0, size=(row.T, row.N)).astype(F32)
    starts = (rng.random((row.T, row.N)) < 0.3).astype(np.uint8) if row.starts == "dense" else np.ones((row.T, row.N), dtype=np.uint8)
    last_values = rng.normal(0.0, 1.0, size=row.N).astype(F32)
    last_dones = (np.arange(row.N) % 2 == 0).astype(np.uint8) if row.N > 1 else np.ones(1, dtype=np.uint8)
    out = (rewards, values, starts, last_values, last_dones)
    for a in out:
        a.setflags(write=False)
    return out


def gae_twin(row):
    return oracle_gae(*gae_inputs(row), row.gamma, row.lam)


GAE_MUTATIONS = ("start_t_for_start_t_plus_1", "last_dones_ignored", "returns_with_next_value", "remainder_skipped", "lambda_without_non_terminal")


def gae_mutation_shows(row, mutation):
    _, _, starts, _, last_dones = gae_inputs(row)
    shifted = np.concatenate([starts[1:], last_dones[None]])  # start_{t+1} of every step
    return {"start_t_for_start_t_plus_1": bool((starts[:-1] != shifted[:-1]).any()),  # (T = 1 has only last_dones; all-set starts are equal)
            "last_dones_ignored": bool(last_dones.any()),
            "returns_with_next_value": True,
            "remainder_skipped": row.T % GAE_UNROLL != 0,
            # the carried advantage is zero behind the last step, and lambda = 0 carries nothing
            "lambda_without_non_terminal": row.lam != 0.0 and row.T > 1 and bool(shifted[:-1].any())}[mutation]


def gae_model(row, mutation=None):
    """gae_kernel's loop in fp64 numpy, one env per column, t counting down. Outputs start as NaN (the GPU test's guard
    value): a step the loop skips stays NaN."""
    assert mutation is None or mutation in GAE_MUTATIONS
    rewards, values, starts, last_values, last_dones = (np.asarray(a, dtype=F64) for a in gae_inputs(row))
    adv, ret = np.full((row.T, row.N), np.nan), np.full((row.T, row.N), np.nan)
    next_value = last_values
    non_terminal = np.ones(row.N) if mutation == "last_dones_ignored" else 1.0 - last_dones
    carried = np.zeros(row.N)
    stop = row.T % GAE_UNROLL if mutation == "remainder_skipped" else 0
    for t in range(row.T - 1, stop - 1, -1):
        if mutation == "start_t_for_start_t_plus_1" and t < row.T - 1:
            non_terminal = 1.0 - starts[t]
        v = values[t]
        delta = rewards[t] + row.gamma * next_value * non_terminal - v
        carried = delta + row.gamma * row.lam * (1.0 if mutation == "lambda_without_non_terminal" else non_terminal) * carried
        adv[t] = carried
        ret[t] = carried + (next_value if mutation == "returns_with_next_value" else v)
        next_value, non_terminal = v, 1.0 - starts[t]
    return adv, ret


def gae_ratio(got_adv, got_ret, row):
    """The worst |got - want| / (atol + rtol |want|) over both outputs (inf for a NaN)."""
    worst = 0.0
    for got, want in zip((got_adv, got_ret), gae_twin(row)):
        worst = max(worst, ratio(np.abs(np.asarray(got, dtype=F64) - want), GAE_ATOL + GAE_RTOL * np.abs(want)))
    return worst

