"""The shape matrix of tests/agent_pipeline_shapes.py without a GPU: its plan is the header's (`pipeline_sizes`,
`pipeline_blocks`, through tests/host_harness.hip), the table covers the wavefront geometries
tests/test_agent_pipeline_matrix_gpu.py claims to run, the scripted masks exercise what they should at every batch size, the
batched twin is the per-env `Twin` bit for bit on every row, and the GPU test is sharp: a twin that is wrong the way a kernel
could be moves a checked value by more than the tolerance the GPU test applies there."""

import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from tests import agent_pipeline_reference as P
from tests import agent_pipeline_shapes as S
from tests.test_device_arithmetic_on_host import harness  # noqa: F401  (the fixture that builds the harness)

ROWS = pytest.mark.parametrize("row", S.MATRIX, ids=S.IDS)
PLANS = [S.plan(r) for r in S.MATRIX]


def test_matrix_keeps_the_existing_shapes_and_has_unique_rows():
    shapes = [(r.K, r.D, r.A) for r in S.MATRIX if r.in_obs]
    assert all(e in shapes for e in S.EXISTING)
    assert len(set(S.IDS)) == len(S.IDS) and len(set(S.CASE_IDS)) == len(S.CASE_IDS)


# ---------------------------------------------------------------- the plan is the header's
@ROWS
def test_plan_is_the_headers(row, harness):  # noqa: F811
    out = (C.c_int * 4)()
    assert harness.harness_pipeline_sizes(row.D, row.A, row.K, int(row.in_obs), out) == 1
    p = S.plan(row)
    assert list(out) == [p["F"], p["S"], p["group"], p["group_act"]]
    assert p["used"] == p["group"] * p["S"] <= S.WAVE_WORDS < p["used"] + p["S"]
    for n in S.batch_sizes(row) + [2, 63, 64, 100003]:
        for group in (p["group"], p["group_act"]):
            assert harness.harness_pipeline_blocks(n, group) == S.blocks(n, group), (n, group)
    assert harness.harness_pipeline_sizes(row.D, 65, 1, 0, out) == 0 and harness.harness_pipeline_sizes(257, 1, 1, 0, out) == 0


@ROWS
def test_batch_sizes_reach_every_kind_of_grid(row):
    p, ns = S.plan(row), S.batch_sizes(row)
    g, ga = p["group"], p["group_act"]
    assert 1 in ns and ga + 1 in ns and (g == 1 or g - 1 in ns)
    assert any(n % (S.WAVES * g) == 0 for n in ns), "whole blocks of observe"
    assert any(n % (S.WAVES * g) == 1 and n > 1 for n in ns), "a last block whose only live wave holds one env"
    assert any(n % 2 and S.blocks(n, g) >= 2 and S.blocks(n, ga) >= 2 for n in ns)
    assert max(ns) <= 1100, "the twin stays quick"
    assert S.reset_after(row) + row.K < S.steps_of(row) - 1 and S.reset_after(row) < S.stage_steps(row) - 1


# ---------------------------------------------------------------- the table covers the geometry
def test_table_covers_the_geometry():
    used, groups, words = {p["used"] for p in PLANS}, {p["group"] for p in PLANS}, {p["S"] for p in PLANS}
    assert {129, 195, 240, 255, 256} <= used
    assert {1, 2, 3, 4} <= groups and max(groups) > 4
    assert {1, 64, 65, 256} <= words
    assert any(r.K == 1 for r in S.MATRIX) and any(r.K == p["S"] and r.K > 1 for r, p in zip(S.MATRIX, PLANS))
    assert any(r.A > p["S"] for r, p in zip(S.MATRIX, PLANS)), "the strided zeroing loop runs more than once"
    assert any(64 % r.A == 0 for r in S.MATRIX) and any(64 % r.A for r in S.MATRIX)
    one = [r for r, p in zip(S.MATRIX, PLANS) if p["group_act"] == 1]
    assert any(r.A == 64 for r in one) and any(r.A < 64 for r in one), "one env per shape_action wave, with and without idle lanes"
    assert max((r.A - 1) >> 2 for r in S.MATRIX) >= 15
    assert max((r.D - 1) >> 2 for r in S.MATRIX) == 63 and P.FINAL_BLOCK + max((r.D - 1) >> 2 for r in S.MATRIX) == 127
    assert {r.in_obs for r in S.MATRIX} == {True, False}
    for r in S.MATRIX:  # the largest block of a row is drawn with a sigma that is not 0
        sig_a, sig_o = S.sigmas_of(r)
        assert any(s > 0 for s in sig_a[4 * ((r.A - 1) >> 2):]) and any(s > 0 for s in sig_o[4 * ((r.D - 1) >> 2):])
        assert (r.A < 3 or 0.0 in sig_a) and (r.D < 3 or 0.0 in sig_o), "some sigmas are 0"


# ---------------------------------------------------------------- the masks exercise what they should
def _mixed(flags, group):
    """Some wave (`group` consecutive envs) holds an env with the flag and one without."""
    n = len(flags)
    return any(0 < flags[w:w + group].sum() < len(flags[w:w + group]) for w in range(0, n, group))


@pytest.mark.parametrize("row, n", S.CASES, ids=S.CASE_IDS)
@pytest.mark.parametrize("stages", [False, True])
def test_masks_exercise_what_they_should(row, n, stages):
    s, p = S.script(row, n, stages), S.plan(row)
    term, trunc = s.terminated, s.truncated
    done = term | trunc
    assert s.steps == S.steps_of(row) and done.shape == (s.steps, n)
    assert not done[0].any(), "a step in which no env ends"
    assert (done.sum(axis=0) >= 2).any(), "an env ends twice"
    assert (term & ~trunc).any() and (trunc & ~term).any() and (term & trunc).any()
    alive = 0
    longest = max((alive := 0 if d else alive + 1) for d in done[:, 0])
    assert done[:, 0].any() and longest >= row.K, "env 0 (the whole batch at N = 1) ends and later holds K frames of one episode"
    assert s.mask.any()
    # env 0 goes into the masked reset, and into its last end, with K frames of one episode in its stack: the frame of
    # the restart and one per step since
    r = s.reset_after
    assert s.mask[0] and done[r - row.K + 1, 0] and not done[r - row.K + 2:r + 1, 0].any()
    assert done[-1, 0] and not done[r + 1:-1, 0].any() and s.steps - 1 - (r + 1) >= row.K
    if n > 1:
        # a wavefront of observe with one env has nobody else in it: there the neighbour is the next wave of the block
        group = p["group"] if min(p["group"], n) > 1 else S.WAVES
        beside = "wave" if group == p["group"] else "block"
        assert any(_mixed(done[t], group) for t in range(s.steps)), f"an env ends beside one of its {beside} that does not"
        assert _mixed(s.mask, group), f"the masked reset hits some envs of a {beside} and misses others"
        for masks in ("terminated", "truncated"):
            assert any(_mixed(S.done_of(s, t, masks), group) for t in range(s.steps))
    big = S.script(row, max(S.batch_sizes(row)), stages)
    assert all(np.array_equal(a[..., :n, :] if a.ndim == 3 else a[..., :n] if a.dtype == bool else a[:n], b)
               for a, b in zip(big[:-2], s[:-2])), "an env reads the same inputs at every batch size"


# ---------------------------------------------------------------- the batched twin is the twin
def test_vectorised_philox_is_the_oracles():
    envs, calls = np.array([0, 1, 777, 0xFFFFFFFF, 12345678]), np.array([0, 0xFFFFFFFF, 5, 1 << 31, 99])
    for seed in (0, (7 << 32) | 12345, 0xFFFFFFFFFFFFFFFF):
        for block in (0, 1, 63, 64, 127):
            words = P.philox_words(envs, calls, block, seed)
            for i, (e, c) in enumerate(zip(envs, calls)):
                want = O.philox([int(e), int(c), 0, (P.STREAM_PIPELINE << 24) | block], [seed & 0xFFFFFFFF, seed >> 32])
                assert [int(w) for w in words[i]] == [int(w) for w in want]
    z = P.philox_normals(envs, calls, 7, 64, 11)
    assert all(z[i, k] == P.philox_normal(int(e), int(c), 64 + (k >> 2), k & 3, 11) for i, (e, c) in enumerate(zip(envs, calls)) for k in range(7))


@ROWS
@pytest.mark.parametrize("stages", [False, True])
def test_batch_twin_is_the_twin_bit_for_bit(row, stages):
    """Three envs of the row's script (0 and 1, whose ends are scripted, and the last), through both resets, every step and
    a poisoned action word; the last counter starts one call before its wrap."""
    n = max(S.batch_sizes(row))
    envs = sorted({0, min(1, n - 1), n - 1})
    s = S.script(row, n, stages)
    low, high, dt, kw = S.settings(row, stages)
    batch = P.BatchTwin(len(envs), row.D, low, high, dt, envs=envs, **kw)
    twins = [P.Twin(e, row.D, low, high, dt, **kw) for e in envs]
    batch.calls[-1] = twins[-1].calls = 0xFFFFFFFE if stages else 0
    steps = sorted(set(range(min(s.steps, 7))) | {s.reset_after, s.steps - 1})

    def same():
        for i, tw in enumerate(twins):
            assert np.array_equal(batch.stack[i], tw.stack) and np.array_equal(batch.prev_command[i], tw.prev_command)
            assert np.array_equal(batch.command[i], tw.command) and int(batch.calls[i]) == tw.calls & 0xFFFFFFFF
            if tw.final is not None:
                assert np.array_equal(batch.final[i], tw.final)

    batch.reset(s.first[envs])
    for e, tw in zip(envs, twins):
        tw.reset(s.first[e])
    same()
    for t in steps:
        action = s.actions[t][envs].copy()
        if t == 3:
            action[0, -1], action[-1, 0] = np.nan, np.inf
        done = S.done_of(s, t)[envs]
        batch.shape_action(action)
        batch.observe(s.next_obs[t][envs], done, s.final_obs[t][envs])
        for i, (e, tw) in enumerate(zip(envs, twins)):
            tw.shape_action(action[i])
            tw.observe(s.next_obs[t][e], bool(done[i]), s.final_obs[t][e])
        same()
        if t == s.reset_after:
            batch.reset(s.again[envs], s.mask[envs])
            for e, tw in zip(envs, twins):
                if s.mask[e]:
                    tw.reset(s.again[e])
            same()
    assert any(tw.final is not None for tw in twins)
    assert (batch.calls > 0).all() == stages


@ROWS
def test_an_envs_run_does_not_depend_on_the_batch(row):
    """The twin's, noise on: the GPU test holds the device to the same."""
    ns = S.batch_sizes(row)
    small, large = ns[1], min(ns[-1], 70)
    if small >= large:
        small = 1
    runs = [S.run_twin(S.twin(row, n, True), S.script(row, n, True)._replace(steps=S.stage_steps(row))) for n in (small, large)]
    for a, b in zip(*runs):
        assert np.array_equal(a, b[:small] if a.ndim < 3 else b[:, :small])


# ---------------------------------------------------------------- sharpness
def _one_step_apart(row, mutation, stages, n=8):
    """The worst |right - wrong| / bound per checked place when a twin with `mutation` takes every step from the right
    twin's state: {place: ratio} (without noise the bound is 0: the ratio is inf where anything moved)."""
    n = min(n, max(S.batch_sizes(row)))
    s = S.script(row, n, stages)
    right, wrong = S.twin(row, n, stages), S.twin(row, n, stages, mutation=mutation)
    worst = {"command": 0.0, "frame": 0.0, "terminal": 0.0, "older_frames": 0.0, "prev_command": 0.0}

    def ratio(place, a, b, bound):
        diff = np.abs(a.astype(np.float64) - b.astype(np.float64))
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(diff > 0, diff / bound, 0.0)
        worst[place] = max(worst[place], float(r.max())) if r.size else worst[place]

    right.reset(s.first)
    for t in range(min(s.steps, 8)):
        for k in ("prev_command", "command", "stack", "final", "calls"):
            setattr(wrong, k, getattr(right, k).copy())
        calls = right.calls.copy()
        _, z = right.shape_action_exact(s.actions[t])
        a, b = right.shape_action(s.actions[t]), wrong.shape_action(s.actions[t])
        ratio("command", a, b, S.command_bound(row, z) if stages else 0.0)
        wrong.command, wrong.prev_command, calls = right.command.copy(), right.prev_command.copy(), right.calls.copy()
        done = S.done_of(s, t)
        bounds = []
        for obs, terminal in ((s.next_obs[t], False), (s.final_obs[t], True)):
            exact, z = right.frame_exact(obs, calls, terminal)
            bounds.append(S.observation_bound(row, exact, z) if stages else 0.0)
        right.observe(s.next_obs[t], done, s.final_obs[t])
        wrong.observe(s.next_obs[t], done, s.final_obs[t])
        ratio("frame", right.stack[:, -1, :row.D], wrong.stack[:, -1, :row.D], bounds[0])
        ratio("older_frames", right.stack[:, :-1], wrong.stack[:, :-1], 0.0)  # (copied or zero: the GPU test demands the bits)
        ratio("prev_command", right.prev_command, wrong.prev_command, 0.0)
        if done.any():
            pick = lambda b: b[done] if isinstance(b, np.ndarray) else b  # noqa: E731
            ratio("terminal", right.final[done, -1, :row.D], wrong.final[done, -1, :row.D], pick(bounds[1]))
    return worst


@ROWS
def test_the_gpu_tests_would_notice(row):
    """Each wrong twin is more than one tolerance away from the right one at the place the GPU test checks, with every
    stage on; the two that move data are seen by the bit-for-bit test as well."""
    apart = _one_step_apart(row, "last_observation_column", True)
    assert apart["frame"] > 1.0 and apart["terminal"] > 1.0 and apart["command"] == 0.0
    apart = _one_step_apart(row, "last_action", True)
    assert apart["command"] > 1.0
    apart = _one_step_apart(row, "swapped_terminal_draws", True)
    assert apart["frame"] > 1.0 and apart["terminal"] > 1.0, "the terminal frame's draws are not the new frame's"
    apart = _one_step_apart(row, "action_block_zero", True)
    assert apart["command"] > 1.0 if row.A >= 5 else apart["command"] == 0.0
    assert _one_step_apart(row, "last_observation_column", False)["frame"] == np.inf
    assert _one_step_apart(row, "last_action", False)["command"] == np.inf
    # the two restarts of an ended env, which the kernel does with a select and a strided loop
    for stages in (False, True):
        assert _one_step_apart(row, "restart_keeps_old_frames", stages)["older_frames"] == (np.inf if row.K > 1 else 0.0)
        assert _one_step_apart(row, "prev_command_zeroed_once", stages)["prev_command"] == (np.inf if row.A > S.plan(row)["S"] else 0.0)


@ROWS
def test_the_terminal_frame_has_draws_of_its_own(row):
    """Every column of every env, at the first calls and at the last: what lets the GPU test's bound on the terminal frame
    tell the blocks 64 + (d >> 2) from the new frame's."""
    n = min(max(S.batch_sizes(row)), 64)
    tw, obs = S.twin(row, n, True), np.zeros((n, row.D), dtype=S.F32)
    for call in (0, 1, 2, 0xFFFFFFFF):
        calls = np.full(n, call, dtype=np.int64)
        assert (tw.frame_exact(obs, calls)[1] != tw.frame_exact(obs, calls, terminal=True)[1]).all()
