"""The tables of tests/ppo_small_shapes.py without a GPU: the constants are the headers', the plans are tests/ppo_reference.py's
and the library's, the tables cover what their `why`s claim, the twins agree with the project's references, fp64 in the
kernels' documented order uses a small fraction of every bound, and each mistake a kernel could make moves a checked value
past its bound (or breaks bit equality) on every row whose geometry lets it show -- with the same functions
tests/test_ppo_small_matrix_gpu.py applies to the device's outputs."""

import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from tests import ppo_reference as R
from tests import ppo_small_shapes as S
from upkie_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADV = pytest.mark.parametrize("row", S.ADV_ROWS, ids=S.ADV_IDS)
EV = pytest.mark.parametrize("row", S.EV_ROWS, ids=S.EV_IDS)
FOLD = pytest.mark.parametrize("row", S.FOLD_ROWS, ids=S.FOLD_IDS)
GAE = pytest.mark.parametrize("row", S.GAE_ROWS, ids=S.GAE_IDS)
# fp64 in the kernel's own order stays below this share of a bound (the most is at minibatches of 2 and 3 samples, whose
# bounds are a dozen roundings; from 1000 samples on it is below 1e-3)
MODEL_FRACTION = 0.25


@pytest.fixture(scope="module")
def library():
    lib.build()
    return lib.load()


def _source(name):
    with open(os.path.join(ROOT, "upkie_amd", "csrc", name)) as f:
        return f.read()


# ---------------------------------------------------------------- the constants and the plans
def test_constants_are_the_headers():
    ppo, reduce, rollout = _source("ppo.hpp"), _source("block_reduce.hpp"), _source("rollout.hpp")
    assert int(re.search(r"PPO_ADV_THREADS = (\d+),", ppo).group(1)) == S.PPO_ADV_THREADS
    assert int(re.search(r"PPO_THREADS = (\d+),", ppo).group(1)) == S.PPO_THREADS == R.FOLD_THREADS
    assert int(re.search(r"PPO_STATS = (\d+),", ppo).group(1)) == S.PPO_STATS == R.STATS
    sweeps = re.findall(r"i0 \+= (\d+) \* PPO_ADV_THREADS", ppo)
    assert sweeps == [str(S.PPO_SWEEP_LOADS)] * 2, "ppo_adv_pass and ppo_ev_pass take 8 x 1024 samples per iteration"
    assert f"b + {S.FOLD_UNROLL} <= grid; b += {S.FOLD_UNROLL}" in reduce
    gae = rollout[rollout.index("void gae_kernel"):rollout.index("linear_policy_kernel")]
    assert f"#pragma unroll {S.GAE_UNROLL}\n  for (int t = T - 1; t >= 0; --t)" in gae and f"__launch_bounds__({S.GAE_THREADS}) void gae_kernel" in rollout


def test_tables_hold_the_sizes_the_issue_names():
    for ids in (S.ADV_IDS, S.EV_IDS, S.FOLD_IDS, S.GAE_IDS):
        assert len(set(ids)) == len(ids)
    single = {r.batch for r in S.ADV_ROWS if r.total == r.batch}
    assert {1, 2, 3, 1023, 1024, 1025, 8191, 8192, 8193, 16385, 65536 + 1} <= single
    assert {r.n for r in S.EV_ROWS if r.kind == "plain"} == {1, 2, 1025, 8192, 8193, 16385, 262151}
    assert {r.kind for r in S.EV_ROWS} == set(S.EV_KINDS)
    shapes = [(r.obs_dim, tuple(r.actor), r.act_dim, tuple(r.critic)) for r in S.FOLD_ROWS]
    worlds = lambda s: {r.world for r, x in zip(S.FOLD_ROWS, shapes) if x == s}  # noqa: E731
    assert worlds((1, (1,), 1, (1,))) == worlds((3, (16,), 2, (16,))) == {1, 2, 31, 32, 33, 64, 65}
    assert worlds((5, (40, 24), 3, (40, 24))) == worlds((30, (256, 256, 128), 36, (256, 256, 128))) == {1, 33}
    assert {r.T for r in S.GAE_ROWS if r.N == 257} == {1, 2, 7, 8, 9, 17} and {r.N for r in S.GAE_ROWS if r.T == 9} == {1, 255, 256, 257, 513}
    assert {(r.gamma, r.lam) for r in S.GAE_ROWS} == {(0.99, 0.95), (1.0, 1.0), (0.9, 0.0)}
    assert any(r.starts == "every_step" for r in S.GAE_ROWS)
    assert any((r.obs_dim, r.world) == S.GRAPHED_FOLD_ROW for r in S.FOLD_ROWS) and any((r.obs_dim, r.world) == S.CONTROLLED_FOLD_ROW for r in S.FOLD_ROWS)


@FOLD
def test_fold_plan_is_the_references_and_the_librarys(row, library):
    shape, p = S.fold_shape(row), S.fold_plan(row)
    ref = R.plan(shape)
    assert all(p[k] == ref[k] for k in ref)
    assert library.upkie_ppo_workspace_bytes(C.byref(shape), S.FOLD_MAX_MINIBATCH) == p["workspace_bytes"] == p["sq_at"] + 8 * p["fold_blocks"]
    assert library.upkie_ppo_slot_bytes(C.byref(shape)) == 4 * p["slot_words"]
    assert library.upkie_mlp_packed_words(C.byref(shape)) == p["words"] == p["train_off"] + p["train_words"]
    assert p["grad_at"] % 8 == 0 and p["slot_words"] % 2 == 0
    # every layer's packed block is a multiple of four words, so launch B' never pads a slot: its `at != train_words` branch
    # cannot be reached by a valid shape
    assert p["train_words"] % 2 == 0 and p["slot_stats_at"] == p["train_words"]
    assert p["fold_blocks"] > 1, "no valid shape fits one fold block: the ticket always has more than one holder"
    assert (p["tensor"] >= 0).sum() < p["train_words"], "every row has padding words"
    assert set(p["tensor"][p["tensor"] >= 0]) == set(range(p["tensors"]))


def test_the_issues_fold_figures_are_the_plans():
    plans = {(r.obs_dim, r.world): S.fold_plan(r) for r in S.FOLD_ROWS}
    assert (plans[1, 1]["train_words"], plans[1, 1]["fold_blocks"]) == (600, 3)
    assert (plans[5, 1]["train_off"], plans[5, 1]["fold_blocks"], plans[5, 1]["last_block"]) == (48, 26, 20)
    assert plans[30, 1]["fold_blocks"] == 870
    assert min(p["fold_blocks"] for p in plans.values()) == 3


def test_advantage_slot_bytes_are_the_librarys(library):
    for row in S.ADV_ROWS:
        assert library.upkie_ppo_advantage_slot_bytes(row.total, row.batch) == 16 * S.adv_plan(row)["M"]


# ---------------------------------------------------------------- the tables cover what they claim
def test_advantage_table_covers_the_geometry():
    plans = [S.adv_plan(r) for r in S.ADV_ROWS]
    sizes = {n for p in plans for n in p["sizes"]}
    for edge in (S.PPO_ADV_THREADS, S.SWEEP):
        assert {edge - 1, edge, edge + 1} <= sizes, "a minibatch on each side of 1024 and of 8192"
    assert {1, 2, 3} <= {p["sweeps"] for p in plans} and max(p["sweeps"] for p in plans) == 9
    assert any(p["M"] >= 3 and r.batch == 8193 and p["last"] == 1 for r, p in zip(S.ADV_ROWS, plans)), "a one-sample last block behind two-sweep ones"
    assert any(p["M"] > 1 and p["last"] == 2 for p in plans) and any(p["M"] > 1 and p["last"] == r.batch - 1 for r, p in zip(S.ADV_ROWS, plans))
    assert any(p["M"] == 1 and p["last"] == 1 for p in plans)
    assert any(p["M"] == 257 and r.batch == 3 and p["finish_blocks"] == 2 and p["finish_last_block_threads"] == 1 for r, p in zip(S.ADV_ROWS, plans))
    for row in S.ADV_ROWS:
        adv, perm = S.adv_inputs(row)
        assert adv.dtype == np.float32 and perm.dtype == np.int32 and np.array_equal(np.sort(perm), np.arange(row.total))
        assert row.total < 8 or not np.array_equal(perm, np.arange(row.total)), "a real shuffle"
        assert row.total < 1000 or (abs(adv.mean() - 1e3) < 0.2 and abs(adv.std() - 1.0) < 0.1)


def test_fold_table_covers_the_geometry():
    plans = [S.fold_plan(r) for r in S.FOLD_ROWS]
    worlds = {r.world for r in S.FOLD_ROWS}
    assert {31, 32, 33} <= worlds and {64, 65} <= worlds and any(32 < w < 64 for w in worlds), "a world on each side of 32 and of 64"
    assert any(p["body"] == 0 and p["tail"] == 31 for p in plans) and any(p["body"] == 64 and p["tail"] == 1 for p in plans)
    assert any(p["body"] and not p["tail"] for p in plans)
    assert any(0 < p["last_block"] < S.PPO_THREADS for p in plans), "a last fold block that is partly filled"
    assert all(p["train_off"] > 0 for p in plans) and len({p["train_off"] for p in plans}) >= 3
    for row in S.FOLD_ROWS:
        ratios, coefs = S.run_apply_model(row)
        assert coefs[0] < 1.0 and coefs[1] == 1.0 and coefs[2] < 1.0, "an apply above max_grad_norm and one below"
    inp, p = S.fold_inputs(S.FOLD_ROWS[0]), S.fold_plan(S.FOLD_ROWS[0])
    real = p["tensor"] >= 0
    assert (inp.m[p["train_off"]:][real] != 0).all() and (inp.v[p["train_off"]:][real] > 0).all() and S.CFG["ent_coef"] != 0.0
    assert not inp.slots[:, :, :p["train_words"]][:, :, ~real].any(), "the padding words of a slot's gradient are zero"
    assert np.array_equal(inp.slots[1, 0, p["slot_stats_at"]:].view(np.float64), inp.sums[1, 0])


def test_gae_table_covers_the_geometry():
    assert {0, 1, 7} <= {r.T % S.GAE_UNROLL for r in S.GAE_ROWS} and any(r.T < S.GAE_UNROLL for r in S.GAE_ROWS) and any(r.T > 2 * S.GAE_UNROLL for r in S.GAE_ROWS)
    assert {-1, 0, 1} <= {r.N - S.GAE_THREADS for r in S.GAE_ROWS} and any(r.N > 2 * S.GAE_THREADS for r in S.GAE_ROWS)
    first_row_set = 0
    for row in S.GAE_ROWS:
        _, _, starts, _, last_dones = S.gae_inputs(row)
        if row.starts == "dense" and row.N > 1:
            assert 0.2 < starts.mean() < 0.4 and 0 < last_dones.sum() < row.N, "dense starts, mixed last_dones"
            first_row_set += bool(starts[0].any()) and not starts[0].all()
        if row.starts == "every_step":
            assert starts.all()
    assert first_row_set >= 5, "row t = 0 is sometimes set"


# ---------------------------------------------------------------- the twins are the project's references
@EV
def test_explained_variance_twin_is_the_references(row):
    for world in S.SHARD_WORLDS:
        parts = [S.ev_inputs(row, s) for s in range(world)]
        ref = S.explained_variance(np.concatenate([v for _, v in parts]), np.concatenate([r for r, _ in parts]))
        if row.kind == "constant":
            continue  # (np.var of a constant is not exactly zero for every count: the kernel's sums of equal fp32 words are)
        assert S.ev_ratio(ref, row, world) <= 1.0, (world, ref, S.ev_twin(row, world))
    want, _ = S.ev_twin(row)
    assert math.isnan(want) == (row.kind == "constant" or row.n == 1) and (row.kind != "equal" or want == 1.0)


def test_advantage_twin_is_numpys():
    for row in S.ADV_ROWS:
        adv, perm = S.adv_inputs(row)
        want, _ = S.adv_twin(row)
        for j, n in enumerate(S.adv_plan(row)["sizes"]):
            x = adv[perm[j * row.batch:j * row.batch + n]].astype(np.float64)
            ref = (x.mean(), x.std(ddof=1) + 1e-8) if n > 1 else (0.0, 1.0)
            np.testing.assert_allclose(want[j], ref, rtol=1e-11)
        assert np.array_equal(S.adv_twin(row, normalize=0)[0], np.tile([0.0, 1.0], (len(want), 1)))


def test_gae_model_is_the_oracle():
    for row in S.GAE_ROWS:
        adv, ret = S.gae_model(row)
        for got, want in zip((adv, ret), S.gae_twin(row)):
            np.testing.assert_allclose(got, want, rtol=1e-13, atol=1e-13)


# ---------------------------------------------------------------- the bounds are attainable in the kernels' order
@ADV
def test_advantage_order_model_uses_a_small_fraction_of_the_bound(row):
    worst = 0.0
    for world in S.SHARD_WORLDS:
        for normalize in (0, 1):
            got = S.adv_model(row, world, normalize)
            worst = max(worst, S.adv_ratio(got, row, world, normalize))
            want, _ = S.adv_twin(row, world, normalize)
            exact = (want[:, 1] == 1.0) & (want[:, 0] == 0.0)
            assert np.array_equal(got[exact], want[exact]), "(0, 1) exactly"
    print(f"matrix model advantage {row.total}/{row.batch}: worst error / bound {worst:.2e}")
    assert worst <= MODEL_FRACTION


@EV
def test_explained_variance_order_model_uses_a_small_fraction_of_the_bound(row):
    worst = max(S.ev_ratio(S.ev_model(row, world), row, world) for world in S.SHARD_WORLDS)
    print(f"matrix model explained variance {row.n} {row.kind}: worst error / bound {worst:.2e}")
    assert worst <= MODEL_FRACTION


@FOLD
def test_apply_model_meets_the_bounds(row):
    """The fold is the expected bits by construction, the fp64 sums in launch B's order use a small fraction of the bound of
    the statistics row (beyond the half ulp of its fp32 store, which is most of that bound), and Adam in numpy fp32 (one
    rounding per operation, nothing fused) is inside the bounds that come from torch's."""
    ratios, _ = S.run_apply_model(row)
    worst = {k: max(r[k] for r in ratios) for k in ratios[0]}
    p = S.fold_plan(row)
    sums = 0.0
    for k in range(S.FOLD_APPLIES):
        grad, _ = S.fold_gradient(row, k)
        log_std = S.fold_inputs(row).packed[p["train_off"]:p["train_off"] + row.act_dim]
        want, bound = S.fold_statistics(row, k, grad, log_std)
        got = S.fold_statistics(row, k, grad, log_std, exact=False)
        sums = max(sums, S.ratio(np.abs(got - want), bound - S.H32 * (1.0 + 2.0 ** -20) * np.abs(want)))
    print(f"matrix model apply {S.FOLD_IDS[S.FOLD_ROWS.index(row)]}: fp64 sums in launch B's order {sums:.2e} of their bound; fp32 model: "
          + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert sums <= MODEL_FRACTION
    assert worst["gradient"] == worst["t"] == worst["padding"] == worst["fixed"] == 0.0 and max(worst.values()) <= 1.0, worst


@FOLD
def test_adam_bounds_come_from_torch_fp32(row):
    """The measured distances of torch fp32 from the twin (profiles/ppo_small_kernels.txt holds these lines) and what the
    bounds are allowed to be: four times them, and on the tensors of fewer than 16 words at least four fp32 roundings."""
    p = S.fold_plan(row)
    bounds, measured, floors = S.adam_bounds(row)
    small = np.array([(p["tensor"] == i).sum() < S.SMALL_TENSOR for i in range(p["tensors"])])
    for k in range(S.FOLD_APPLIES):
        for q in ("m", "v", "delta"):
            assert np.array_equal(bounds[k][q], 4.0 * np.maximum(measured[k][q], floors[k][q])) and not floors[k][q][~small].any()
            assert (measured[k][q][~small] < 1e-3).all(), "torch fp32 is itself close to the twin"
    figures = lambda a: f"{a.min():.1e}..{a.max():.1e}"  # noqa: E731
    line = "; ".join(f"t={k + 1} " + " ".join(f"{q} {figures(measured[k][q])}" for q in ("m", "v", "delta")) for k in range(S.FOLD_APPLIES))
    floor = " ".join(f"{q} {figures(floors[0][q][small])}" for q in ("m", "v", "delta")) if small.any() else "none"
    print(f"matrix torch-fp32 adam {S.FOLD_IDS[S.FOLD_ROWS.index(row)]} ({p['tensors']} tensors, {int(small.sum())} below {S.SMALL_TENSOR} words): "
          f"relative distance per tensor, least..most: {line}; floors of the small tensors at t=1: {floor}")


# ---------------------------------------------------------------- sharpness
@pytest.mark.parametrize("mutation", S.ADV_MUTATIONS)
def test_the_advantage_checks_would_notice(mutation):
    """On every row and shard count whose plan lets the mistake show, the wrong model is past a bound (or (0, 1) is not
    exact); where the plan says it cannot show, it does not."""
    bites = 0
    for row in S.ADV_ROWS:
        for world in S.SHARD_WORLDS:
            shows = S.adv_mutation_shows(row, world, mutation)
            apart = S.adv_ratio(S.adv_model(row, world, 1, mutation), row, world)
            assert shows is None or (apart > 1.0) == shows, (row, world, apart)
            bites += bool(shows)
    assert bites >= 3, mutation


@pytest.mark.parametrize("mutation", S.EV_MUTATIONS)
def test_the_explained_variance_checks_would_notice(mutation):
    bites = 0
    for row in S.EV_ROWS:
        for world in S.SHARD_WORLDS:
            if not S.ev_mutation_shows(row, world, mutation):
                continue
            apart = S.ev_ratio(S.ev_model(row, world, mutation), row, world)
            assert apart > 1.0, (row, world, apart)
            bites += 1
    assert bites >= 3, mutation


@FOLD
def test_the_apply_checks_would_notice(row):
    """Every mistake of `FOLD_MUTATIONS` on this row: past a bound or a broken bit on some apply where the plan lets it
    show, inside every bound where it cannot."""
    for mutation in S.FOLD_MUTATIONS:
        ratios, _ = S.run_apply_model(row, mutation)
        apart = max(max(r.values()) for r in ratios)
        assert (apart > 1.0) == S.fold_mutation_shows(row, mutation), (mutation, ratios)
        if mutation in ("tail_dropped", "tail_first", "entropy_on_no_word", "entropy_on_one_word_more") and apart > 1.0:
            assert ratios[0]["gradient"] == float("inf"), "the fold's bits"
        if mutation == "coef_not_applied":
            assert max(ratios[0].values()) > 1.0 and max(ratios[0][q] for q in ("gradient", "stats", "t", "padding", "fixed")) <= 1.0, "Adam's words alone"


def test_every_apply_mistake_bites():
    for mutation in S.FOLD_MUTATIONS:
        assert sum(S.fold_mutation_shows(r, mutation) for r in S.FOLD_ROWS) >= 3, mutation


@pytest.mark.parametrize("mutation", S.GAE_MUTATIONS)
def test_the_gae_checks_would_notice(mutation):
    bites = 0
    for row in S.GAE_ROWS:
        shows = S.gae_mutation_shows(row, mutation)
        apart = S.gae_ratio(*S.gae_model(row, mutation), row)
        assert (apart > 1.0) == shows, (row, apart)
        bites += shows
    assert bites >= 3, mutation


@GAE
def test_gae_in_fp32_meets_the_tolerance(row):
    """The recurrence in numpy fp32 (what the kernel computes, up to fused multiply-adds) against the fp64 oracle."""
    rewards, values, starts, last_values, last_dones = S.gae_inputs(row)
    f = np.float32
    adv, ret = np.zeros((row.T, row.N), dtype=f), np.zeros((row.T, row.N), dtype=f)
    nv, nt, carried = last_values, (1 - last_dones).astype(f), np.zeros(row.N, dtype=f)
    for t in range(row.T - 1, -1, -1):
        delta = rewards[t] + f(row.gamma) * nv * nt - values[t]
        carried = delta + f(row.gamma) * f(row.lam) * nt * carried
        adv[t], ret[t] = carried, carried + values[t]
        nv, nt = values[t], (1 - starts[t]).astype(f)
    worst = S.gae_ratio(adv, ret, row)
    print(f"matrix model gae T {row.T} N {row.N}: fp32 recurrence at {worst:.3f} of rtol {S.GAE_RTOL} atol {S.GAE_ATOL}")
    assert worst <= 0.5
