"""The tables of tests/reduction_shapes.py without a GPU: their launch plans are the headers' (`episodes_blocks`,
`episodes_workspace_bytes`, `vecnorm_blocks`, through tests/host_harness.hip, and `upkie_vecnorm_workspace_bytes`), the tables
cover the grid geometries tests/test_reduction_matrix_gpu.py claims to run, the scripted streams exercise what they should, the
batched Monitor twin is `MonitorTwin` bit for bit, the GPU tests are sharp (a twin that is wrong the way a kernel could be
moves a checked value by more than the tolerance applied there), and their bounds are attainable in the kernel's own order of
operations."""

import ctypes as C
import itertools

import numpy as np
import pytest

from tests import reduction_shapes as S
from tests.episodes_reference import MonitorTwin
from tests.test_device_arithmetic_on_host import harness  # noqa: F401  (the fixture that builds the harness)

EPISODES = pytest.mark.parametrize("row", S.EPISODE_ROWS, ids=S.EPISODE_IDS)
VECNORM = pytest.mark.parametrize("row", S.VECNORM_ROWS, ids=S.VECNORM_IDS)
NEW_VECNORM = [r for r in S.VECNORM_ROWS if (r.N, r.D) not in S.VECNORM_EXISTING]
EP_PLANS = [S.episodes_plan(r) for r in S.EPISODE_ROWS]
SIZES = list(itertools.product((1, 2, 255, 256, 257, 511, 100003, 1 << 20), (1, 2, 127, 128, 129, 255, 256)))


def test_tables_keep_the_existing_sizes_and_have_unique_rows():
    assert all(e in [(r.N, r.window) for r in S.EPISODE_ROWS] for e in S.EPISODE_EXISTING)
    assert all(e in [(r.N, r.D) for r in S.VECNORM_ROWS] for e in S.VECNORM_EXISTING)
    assert len(set(S.EPISODE_IDS)) == len(S.EPISODE_IDS) and len(set(S.VECNORM_IDS)) == len(S.VECNORM_IDS)
    assert S.GRAPHED_EPISODE_ROW in [(r.N, r.window) for r in S.EPISODE_ROWS]
    assert all(1 <= r.window <= S.EPISODES_MAX_WINDOW for r in S.EPISODE_ROWS) and all(1 <= r.D <= 256 for r in S.VECNORM_ROWS)


# ---------------------------------------------------------------- the plans are the headers'
def test_plans_are_the_headers(harness):  # noqa: F811
    from upkie_amd import lib

    harness.harness_episodes_workspace_bytes.restype = C.c_int64
    library = lib.load()
    rows = C.c_int()
    for n in sorted({r.N for r in S.EPISODE_ROWS} | {n for n, _ in SIZES}):
        assert (harness.harness_episodes_blocks(n, C.byref(rows)), rows.value) == S.episodes_blocks(n), n
        assert harness.harness_episodes_workspace_bytes(n) == S.episodes_workspace_bytes(n) == library.upkie_episodes_workspace_bytes(n)
        blocks, per = S.episodes_blocks(n)
        assert blocks <= S.EPISODES_MAX_BLOCKS and (blocks - 1) * per < n <= blocks * per, "every block owns at least one env"
        carve = (C.c_int64 * 6)()
        harness.harness_episode_append_offsets(n, carve)
        assert list(carve) == [256, 256 + 4096] + [256 + 4096 + k * n for k in (0, 8, 12, 16)], n
    for n, d in [(r.N, r.D) for r in S.VECNORM_ROWS] + SIZES + [(sum(shards), d) for d, shards in S.SHARDED]:
        blocks, per, cap = S.vecnorm_blocks(n, d)
        assert (harness.harness_vecnorm_blocks(n, d, C.byref(rows)), rows.value) == (blocks, per), (n, d)
        assert library.upkie_vecnorm_workspace_bytes(n, d) == 256 + blocks * 2 * (d + 1) * 8 == S.vecnorm_workspace_bytes(n, d)
        assert blocks <= cap <= S.VECNORM_MAX_BLOCKS and blocks * 2 * (d + 1) <= S.VECNORM_PARTIAL_WORDS, "the partials stay within 64 KB"
        assert (blocks - 1) * per < n <= blocks * per, "every block owns at least one env"


def test_the_issues_figures_are_the_formulas():
    """The geometry each row's `why` names, recomputed."""
    ep = {(r.N, r.window): p for r, p in zip(S.EPISODE_ROWS, EP_PLANS)}
    assert (ep[257, 300]["blocks"], ep[257, 300]["rows"], ep[257, 300]["last_block"]) == (2, 129, 128)
    assert (ep[4099, 100]["blocks"], ep[4099, 100]["rows"], ep[4099, 100]["last_block"]) == (17, 242, 227)
    p = ep[65537, 1025]
    assert (p["blocks"], p["last_block"], p["prefix_threads"], p["stages"], p["last_stage"]) == (257, 1, 65, 2, 1)
    p = ep[262145, 2500]
    assert (p["blocks"], p["rows"], p["chunks"], p["last_chunk_lanes"], p["last_block"]) == (1021, 257, 2, 1, 5)
    assert S.episodes_blocks(262144)[1] == 256, "262145 is the smallest N with rows > 256"
    p = ep[300001, 65536]
    assert (p["blocks"], p["rows"], p["stages"], p["last_stage"]) == (1024, 293, 64, 1024)
    vn = {(r.N, r.D): S.vecnorm_plan(r) for r in S.VECNORM_ROWS}
    assert (vn[257, 1]["blocks"], vn[257, 1]["rows"], vn[257, 1]["last_block_envs"]) == (2, 129, 128)
    p = vn[513, 3]
    assert (p["full"][0]["slots"], p["full"][0]["idle"], p["blocks"], p["last_block"][0]["slots"]) == (85, 1, 3, 3)
    assert vn[4097, 85]["full"][0]["slots"] == 3 and vn[4097, 85]["full"][0]["idle"] == 1
    p = vn[4097, 86]
    assert (p["full"][0]["slots"], p["full"][0]["idle"], p["blocks"], p["last_block"][0]["slots"], p["last_block"][0]["partials"]) == (2, 84, 17, 2, 9)
    p = vn[2049, 128]
    assert (p["full"][0]["slots"], p["full"][0]["idle"], p["last_block"][0]["slots"], p["last_block"][0]["partials"]) == (2, 0, 1, p["blocks"])
    assert p["blocks"] > 1
    assert (vn[600, 129]["full"][0]["slots"], vn[600, 129]["full"][0]["idle"]) == (1, 127)
    p = vn[8191, 255]
    assert (p["cols"], p["cap"], p["cap_binds"], p["rows"], p["last_block_envs"], p["short"][0]["last_chunks"]) == (256, 16, True, 512, 511, [7])
    assert len(p["last_block"]) == 1 and p["last_block"][0]["g"] == 256
    p = vn[3841, 256]
    assert (p["cols"], p["cap"], p["cap_binds"], p["rows"], p["full"][1]["lane_rows"]) == (257, 15, True, 257, 2)
    assert [q["g"] for q in p["last_block"]] == [256, 1]
    p = vn[70001, 7]
    assert (p["blocks"], p["rows"], p["last_block"][0]["slots"], p["last_block"][0]["partials"]) == (256, 274, 32, 8)
    assert (vn[65537, 1]["blocks"], vn[65537, 1]["last_block_envs"]) == (256, 2)


# ---------------------------------------------------------------- the tables cover the geometry
def test_episode_table_covers_the_geometry():
    rows = list(zip(S.EPISODE_ROWS, EP_PLANS))
    assert any(p["rows"] > 256 and p["chunks"] == 2 and p["last_chunk_lanes"] == 1 for _, p in rows), "a second chunk with one live lane"
    assert any(p["rows"] > 256 and p["blocks"] == S.EPISODES_MAX_BLOCKS for _, p in rows), "the block cap with chunked blocks"
    assert any(256 < p["blocks"] < 1024 and p["last_block"] == 1 for _, p in rows), "own[1..3] live in the prefix; a one-env last block"
    assert any(0 < p["last_block"] < p["rows"] for _, p in rows), "a short last block"
    assert any(r.window > 1024 and r.window % S.EPISODES_STAGE for r, _ in rows)
    assert any(r.window == S.EPISODES_MAX_WINDOW for r, _ in rows)
    assert any(r.window > r.N for r, _ in rows)
    assert any(p["blocks"] == 1 for _, p in rows) and any(r.N == 1 and r.window == 1 for r, _ in rows)


def test_vecnorm_table_covers_the_geometry():
    plans = [S.vecnorm_plan(r) for r in S.VECNORM_ROWS]
    groups = [g for p in plans for g in p["full"] + p["short"]]
    assert {1, 2, 3, 85, 256} <= {g["slots"] for g in groups}
    assert {0, 1, 84, 127} <= {g["idle"] for g in groups}
    assert any(p["cap_binds"] and p["rows"] > 256 for p in plans), "the cap binds and a lane takes more than one row"
    assert any(p["blocks"] == S.VECNORM_MAX_BLOCKS for p in plans)
    assert any(p["full"][-1]["lane_rows"] == 2 for p in plans), "a returns lane with 2 rows"
    assert {256, 257} <= {p["cols"] for p in plans}
    partials = {q["partials"] for p in plans for q in p["last_block"]}
    assert 1 in partials and max(partials) > 8
    assert any(q["slots"] == 1 and q["partials"] > 1 for p in plans for q in p["last_block"]), "the strided walk over partials at slots = 1"
    assert any(len(p["last_block"]) == 2 for p in plans) and any(q["slots"] % 2 and q["slots"] > 1 for p in plans for q in p["last_block"])
    assert any(c < S.VECNORM_CHUNK for g in groups if g["slots"] == 1 for c in g["last_chunks"]), "a last chunk shorter than 8 behind full ones"
    assert any(0 < p["last_block_envs"] < p["rows"] for p in plans)
    # the reset (cols = D) and norm_obs=False (cols = 1) launches run at every row: multi-block ones among them
    assert sum(p["blocks"] > 1 for p in plans) >= 10
    assert all(S.vecnorm_plan(r, "no_norm_obs")["cols"] == 1 for r in S.VECNORM_ROWS)
    for d, shards in S.SHARDED:
        assert 1 <= len(shards) <= 3
    assert {len(shards) for _, shards in S.SHARDED} == {1, 2, 3} and any(len(set(shards)) > 1 for _, shards in S.SHARDED)


# ---------------------------------------------------------------- the scripts exercise what they should
@EPISODES
def test_scripts_exercise_what_they_should(row):
    """A step with more finishers than the window needs N > window and a non-empty block between empty ones three blocks:
    the rows that have them must show them; every row wraps its ring."""
    s, plan = S.episode_script(row), S.episodes_plan(row)
    blocks, rows = plan["blocks"], plan["rows"]
    T = len(s.given)
    assert T <= 10 and s.rewards.dtype == np.float32 and s.rewards.shape == (T, row.N)
    totals = [int(S.done_of(s, t).sum()) for t in range(T)]
    assert totals[0] == 0 and row.N in totals
    assert any(S.done_of(s, t)[-1] and totals[t] == 1 for t in range(T)), "only the last env"
    assert any(S.done_of(s, t)[0] and totals[t] == 1 for t in range(T)), "only env 0"
    assert any((s.terminated[t] & s.truncated[t]).any() and (s.terminated[t] ^ s.truncated[t]).any() for t in range(T)) or row.N == 1
    assert 0 <= s.reset_after < T - 1 and s.mask.any() and (row.N == 1 or not s.mask.all())
    if row.N > row.window:
        assert max(totals) > row.window and sum(t > row.window for t in totals) >= 2, "keep = window, twice: the second at a head that moved"
    counts = [np.add.reduceat(S.done_of(s, t).astype(np.int64), np.arange(0, row.N, rows)) for t in range(T)]
    assert all(len(c) == blocks for c in counts)
    if blocks >= 3:
        assert any(c[b] == min(rows, row.N - b * rows) and c.sum() == c[b] and 0 < b < blocks - 1 for c in counts for b in [blocks // 2]), \
            "every env of one middle block and no other"
        assert any((c == 1).all() for c in counts), "the first env of each block"
    if blocks >= 2:
        assert any(c[b] == 0 and c[b + 1] > 0 for c in counts for b in range(blocks - 1)), "an empty block before a non-empty one"
    # the ring wraps, and the means are taken over a ring whose oldest entry is not slot 0
    model = S.EpisodesOrderModel(row.N, row.window)
    wraps = []
    S.run_episode_script(s, model, after=lambda t: wraps.append(model.last["head"] + model.last["keep"] > row.window or
                                                                (model.last["keep"] and model.last["head"] + model.last["keep"] == row.window)))
    assert any(wraps), "head + keep reaches past the ring's end"
    assert model.fill == row.window


# ---------------------------------------------------------------- the batched twin is the twin, and so is the order model
@EPISODES
def test_batch_monitor_twin_is_the_monitor_twin_bit_for_bit(row):
    n = row.N if row.N <= 5000 else 3000
    s = S.episode_script(row)
    envs = slice(0, n)
    batch, twin = S.BatchMonitorTwin(n, row.window), MonitorTwin(n, row.window)

    def same(t):
        assert list(batch.ep_info_buffer) == list(twin.ep_info_buffer), t
        assert batch.total_episodes == twin.total_episodes and batch.means() == twin.means(), t
        assert batch.safe_mean("r") == twin.safe_mean("r") or not twin.ep_info_buffer
        for a, b in zip(batch.running(), twin.running()):
            assert np.array_equal(a, b), t

    S.run_episode_script(s, batch, twin, envs=envs, after=same)
    assert twin.total_episodes > n


@EPISODES
def test_episodes_order_model_is_the_twin_bit_for_bit(row):
    """The kernel's order (segments, prefix, search, wrapped slots) gives the deque's bits at every row: what the
    mutations below depart from."""
    s = S.episode_script(row)
    model, twin = S.EpisodesOrderModel(row.N, row.window), S.BatchMonitorTwin(row.N, row.window)

    def same(t):
        assert S.same_as_twin(model, twin), t

    S.run_episode_script(s, model, twin, after=same)


# ---------------------------------------------------------------- sharpness
def _caught(row, mutation):
    s = S.episode_script(row)
    model, twin = S.EpisodesOrderModel(row.N, row.window, mutation=mutation), S.BatchMonitorTwin(row.N, row.window)
    seen = []
    S.run_episode_script(s, model, twin, after=lambda t: seen.append(not S.same_as_twin(model, twin)))
    return any(seen)


@EPISODES
def test_the_episode_checks_would_notice(row):
    """Bit for bit means any bit: each wrong model differs from the twin in a value `_compare` reads, behind some step,
    at every row whose geometry lets the mistake show."""
    plan = S.episodes_plan(row)
    assert _caught(row, "last_row_dropped")
    assert _caught(row, "slot_without_the_wrap") == (row.window > 1), "(a ring of one has its head at 0 for ever)"
    assert _caught(row, "first_window_kept") == (row.N > row.window)
    assert _caught(row, "neighbour_of_an_empty_block") == (plan["blocks"] >= 2)


def test_every_episode_mistake_is_caught_by_a_new_row():
    new = [r for r in S.EPISODE_ROWS if (r.N, r.window) not in S.EPISODE_EXISTING]
    for mutation in S.EPISODE_MUTATIONS:
        assert any(_caught(r, mutation) for r in new[:4]), mutation


def _applies(row, mutation):
    p = S.vecnorm_plan(row)
    return {"short_block_counted_as_rows": p["last_block_envs"] < p["rows"], "last_row_dropped": True,
            "last_partial_skipped": any(q["partials"] > 1 for q in p["last_block"]),
            "returns_second_row_skipped": p["rows"] > S.VECNORM_THREADS}[mutation]


@pytest.mark.parametrize("mutation", S.VECNORM_MUTATIONS)
def test_the_normaliser_checks_would_notice(mutation):
    """On every new row whose geometry lets the mistake show, the wrong model is more than one of `_check_stats`'s bounds
    away from the twin."""
    rows = [r for r in NEW_VECNORM if _applies(r, mutation)]
    assert len(rows) >= 2, "a row is missing"
    for row in rows:
        apart = S.run_vecnorm_model(row, "two_launch", mutation)
        assert max(apart.values()) > 1.0, (row, apart)
        if mutation == "returns_second_row_skipped":
            assert apart["returns"] > 1.0 and max(apart["ret_mean"], apart["ret_var"]) > 1.0 and apart["obs_mean"] <= 0.1


# ---------------------------------------------------------------- the bounds are attainable in the kernel's order
@VECNORM
def test_bounds_are_attainable_in_the_kernels_order(row):
    """fp64 in the documented order (chunks of 8 two-pass, Chan per lane, the LDS tree, partials merged p, p + slots, ...)
    stays within a tenth of every bound of `_check_stats` against the twin, behind every step, with and without the reset
    launch and with the returns column alone."""
    worst = {}
    for form in ("reset_first", "no_norm_obs"):
        for k, v in S.run_vecnorm_model(row, form).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"matrix model {row.N}x{row.D}: worst error / bound: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert worst.pop("mirrors") <= 1.0  # (ulps: whole numbers)
    assert max(worst.values()) <= 0.1, worst
