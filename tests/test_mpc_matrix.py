"""The shape matrix of tests/mpc_shapes.py without a GPU: its geometry is the header's own (`mpc_index`, the tile and
K-step counts, the grid and its XCD remap, read from the sources), the table covers the classes
tests/test_mpc_matrix_gpu.py claims to run and loses a class when the row that alone covers it is deleted, the scripted
inputs decide what they should (from the fp64 checker alone: every default-settings row lies within 2e-3 a_max of the exact
QP and its saturating steps saturate a part of the plan), the twin of `step_env` is `oracle_mpc_step` on the envs that are
not done, and every mutation of the twin fails the comparison that the GPU test applies."""

import functools
import os
import re

import numpy as np
import pytest

from tests import mpc_reference as R
from tests import mpc_shapes as S
from upkie_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = pytest.mark.parametrize("row", S.MATRIX, ids=S.IDS)
DEFAULT_ROWS = [r for r in S.MATRIX if S.default_settings(r)]


def _source(name):
    with open(os.path.join(ROOT, "upkie_amd", "csrc", name)) as f:
        return f.read()


def _c_int(expression, **names):
    """A C expression over non-negative ints in Python."""
    return eval(expression.replace("/", "//"), {"__builtins__": {}}, names)  # noqa: S307  (the project's own header)


# ---------------------------------------------------------------- the geometry is the header's
def test_geometry_is_the_headers():
    hpp, abi_unit = _source("mpc.hpp"), _source("upkie_hip.hip")
    index = re.search(r"int mpc_index\(int t, int g, int r\) \{ return ([^;]+); \}", hpp).group(1)
    for t in range(4):
        for g in range(4):
            for r in range(4):
                assert _c_int(index, t=t, g=g, r=r) == S.mpc_index(t, g, r)
    assert sorted(S.mpc_index(t, g, r) for t in range(4) for g in range(4) for r in range(4)) == list(range(64))
    kj = re.search(r"constexpr int KJ = ([^;]+);\s*// 32-wide K-steps", hpp).group(1)
    tiles = re.search(r"mpc->tiles = ([^;]+);", abi_unit).group(1).replace("config->nb_timesteps", "N")
    grid = re.search(r"dim3 grid\(\(unsigned\)\(([^;]+)\)\), block\(64\);", abi_unit).group(1).replace("mpc->dev.num_envs", "B")
    for N in range(1, 65):
        assert _c_int(tiles, N=N) == S.tiles(N)
    for T in range(1, 5):
        assert _c_int(kj, T=T) == S.k_steps(T)
    for B in list(range(1, 300)) + [500, 16384]:
        assert _c_int(grid, B=B) == S.grid(B)
    # the remap, the same line in every MPC kernel, and the env of a column
    remap = "if ((gridDim.x & 7u) == 0u) block = (block & 7u) * (gridDim.x >> 3) + (block >> 3);"
    assert hpp.count(remap) == 3 and "(int)block * 16" in hpp
    for B in (128, 256, 500):  # a permutation of the blocks
        n = S.grid(B)
        assert S.remapped(B) and sorted((b & 7) * (n >> 3) + (b >> 3) for b in range(n)) == list(range(n))
    # the single-launch path is taken exactly when one tile holds the horizon
    assert "lanes_of(sim, MODE_BASE_VELOCITY) >= 2 && mpc->tiles == 1" in abi_unit
    cfg = abi.default_mpc_config(1, 50)
    assert (cfg.fall_pitch, cfg.max_ground_velocity, cfg.max_ground_accel) == (S.FALL_PITCH, S.V_MAX, S.A_MAX)


def test_matrix_keeps_the_existing_cases_and_has_unique_rows():
    assert len(set(S.IDS)) == len(S.IDS) == len(S.MATRIX)
    plain = [(r.N, r.B) for r in S.MATRIX if r.entry == "step" and S.default_settings(r)]
    assert all(e in plain for e in S.EXISTING)
    settings = [(r.N, r.rho, r.relaxation, r.leg_length) for r in S.MATRIX if r.B == 256]
    assert settings == S.EXISTING_SETTINGS
    assert all(1 <= r.N <= 64 and 1 <= r.B <= 500 and r.entry in ("step", "step_env") and r.why for r in S.MATRIX)


# ---------------------------------------------------------------- the table covers the classes
def _classes(rows):
    """The classes a set of rows runs: {name: rows}."""
    geo = [(r, S.geometry(r)) for r in rows]
    out = {f"T = {T}": [r for r, g in geo if g["T"] == T] for T in (1, 2, 3, 4)}
    out.update({f"KJ = {k}": [r for r, g in geo if g["KJ"] == k] for k in (1, 2)})
    out["a lane group that holds only padding"] = [r for r, g in geo if g["padding_only_groups"]]
    out["a tile with one real row"] = [r for r, g in geo if g["last_tile_rows"] == 1]
    out["an identity-remap grid"] = [r for r, g in geo if not g["remapped"] and g["grid"] > 1]
    out["a remapped grid with a tail"] = [r for r, g in geo if g["remapped"] and g["last_columns"] < 16]
    out["a remapped grid of full blocks"] = [r for r, g in geo if g["remapped"] and g["last_columns"] == 16]
    out["one live column in the last block"] = [r for r, g in geo if g["last_columns"] == 1 and g["grid"] > 1]
    out["B < 16"] = [r for r in rows if r.B < 16]
    out["B = 16"] = [r for r in rows if r.B == 16]
    out["a done row"] = [r for r in rows if r.entry == "step_env" and (S.script(r).done != 0).any()]
    out["a null first_input"] = [r for r in rows if r.entry == "step_env"]
    out["alpha = 1 because admm_relaxation is unset"] = [r for r in rows if r.relaxation == 0.0]
    out["one iteration"] = [r for r in rows if S.config(r).admm_iterations == 1]
    out["more iterations than the default"] = [r for r in rows if r.iterations is not None and r.iterations > abi.default_mpc_config(1, r.N).admm_iterations]
    return out


def test_table_covers_the_classes():
    classes = _classes(S.MATRIX)
    assert all(classes.values()), [k for k, v in classes.items() if not v]
    horizons = {r.N for r in S.MATRIX if r.entry == "step" and r.B == 500 and S.default_settings(r)}
    assert horizons >= {1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49, 50, 51, 63, 64}
    for N in (1, 15, 50):
        assert {r.B for r in S.MATRIX if r.N == N and r.entry == "step" and S.default_settings(r)} >= {1, 15, 16, 17, 100, 128, 129, 500}
    assert {(r.N, r.B) for r in S.ENV_ROWS} == {(N, B) for N in (1, 7, 16, 33, 50) for B in (17, 100, 500)}
    assert {r.N for r in S.MATRIX if r.relaxation == 0.0} == {2, 16, 50}
    assert {(r.iterations, r.N) for r in S.MATRIX if r.iterations is not None} == {(i, N) for i in (1, 2, 31) for N in (15, 50)}
    # step_env reaches the geometry too (T = 2 shares its KJ with T = 1 and its tile count with nothing else: step's alone)
    env = _classes(S.ENV_ROWS)
    assert all(env[k] for k in ("T = 1", "T = 3", "T = 4", "KJ = 1", "KJ = 2", "a lane group that holds only padding", "a tile with one real row",
                                "an identity-remap grid", "a remapped grid with a tail", "one live column in the last block"))


def test_a_class_is_lost_with_the_rows_that_cover_it():
    """Class by class: without the rows that cover it the class is empty, whatever else stays, and
    `test_table_covers_the_classes` reports it; a class that one row alone covers is lost with that row."""
    classes = _classes(S.MATRIX)
    for name, rows in classes.items():
        assert not _classes([r for r in S.MATRIX if r not in rows])[name], name
        if len(rows) == 1:
            assert not _classes([r for r in S.MATRIX if r != rows[0]])[name], name
    # horizons 2 .. 4 at step and 1 at every entry are all that leaves a lane group without a real element
    assert {r.N for r in classes["a lane group that holds only padding"]} == {1, 2, 3}
    assert {r.N for r in classes["one iteration"]} == {15, 50}


# ---------------------------------------------------------------- the inputs decide what they should
@pytest.mark.parametrize("N", sorted({r.N for r in S.MATRIX}))
def test_scripted_inputs_reach_every_branch(N):
    pool = S._pool(N)
    assert all(a.dtype == S.F32 for a in (pool.x0, pool.target, pool.act, pool.done, pool.v0)) and pool.contact.dtype == np.uint8
    pitch = np.abs(pool.x0[:, :, 1])
    over = pitch > S.FALL_PITCH
    assert (np.abs(pitch - S.FALL_PITCH) > 1e-3).all(), "no pitch at the threshold"
    assert ((pitch[over] >= 1.05 * S.FALL_PITCH - 1e-6) & (pitch[over] <= 1.3 * S.FALL_PITCH + 1e-6)).all() and (pitch[~over] <= 0.75 + 1e-6).all()
    assert pool.contact[over].all(), "fallen, but touching"
    for t in range(S.STEPS):
        assert 0.05 < over[t].mean() < 0.16 and 0.05 < (pool.contact[t] == 0).mean() < 0.16
        share = (pool.done[t] != 0).mean()
        assert (0.10 < share < 0.20) if t in (1, 3) else share == 0.0
    assert {float(v) for v in np.unique(pool.done)} == {0.0, 1.0, 2.5} and np.signbit(pool.done[pool.done == 0]).any(), "a -0.0 that is not done"
    assert np.isnan(pool.act[:, :, 1]).all() and np.array_equal(pool.act[:, :, 0], pool.target)
    assert np.abs(pool.v0).max() <= 1.02 * S.V_MAX + 1e-6 and (pool.v0 > S.V_MAX).any() and (pool.v0 < -S.V_MAX).any()
    for sign in (1.0, -1.0):
        inside = S.V_MAX - sign * pool.v0
        assert ((inside > 0) & (inside < 0.02)).any(), "a start inside the last 0.02 below the bound"
    # the scripted head (mpc_shapes._pool): what a batch of one still sees
    assert not over[0, :4].any() and pool.contact[0, :4].all() and pool.v0[0] > S.V_MAX and pool.v0[1] < -S.V_MAX
    assert over[1, 0] and pool.done[1, 0] == 0 and np.signbit(pool.done[1, 0]) and pool.done[3, 0] == 2.5 and pool.done[1, 1] == 1.0


@pytest.mark.parametrize("row", DEFAULT_ROWS, ids=[S.row_id(r) for r in DEFAULT_ROWS])
def test_checker_alone_meets_the_exact_qp_and_saturates(row):
    """Conditions on the inputs, from the fp64 checker alone: what the fixed number of iterations leaves open stays inside
    2e-3 a_max on every tenth env at every step; steps 2 and 3 put between 5 % and 90 % of the plan at the bound. The
    share is taken over the horizon's whole script (POOL envs), of which a smaller batch reads the first rows: a plan of
    one element in a batch of one has no share between the two."""
    share = S.exact_share(row, S.twin_trace(row))
    print(f"{S.row_id(row)}: checker against the exact QP {share:.3g} of the bound")
    assert share <= 1.0
    at_bound = _saturation(row.N)
    print(f"N = {row.N}: share of the plan at the bound, step by step {at_bound}")
    assert all(0.05 <= a <= 0.90 for a in at_bound[2:]), at_bound


@functools.lru_cache(maxsize=None)
def _saturation(N):
    """Per step: the share of the checker's plan that lies at +-a_max, over the horizon's whole script."""
    whole = S.Row(N, S.POOL, "step", None, None, None, None, "the whole script")
    twin, s = R.Twin(S.config(whole)), S.script(whole)
    twin.commanded_velocity[:] = s.v0
    out = []
    for t in range(S.STEPS):
        twin.step(s.x0[t], s.target[t], s.contact[t], S.DT)
        out.append(round(float((np.abs(twin.workspace[:N]) >= S.A_MAX).mean()), 3))
    return out


@ROWS
def test_every_branch_decides_something_in_every_row(row):
    """From the checker alone, on the row's own envs: the clamp, the fallen-but-touching branch, the decay of an env in
    the air and (step_env rows) a done row each set a commanded velocity."""
    s, trace = S.script(row), S.twin_trace(row)
    assert S.fallen_but_touching(s, 1)[0]
    assert (np.abs(trace.velocity) <= S.V_MAX).all() and np.abs(trace.velocity[0, 0]) == S.V_MAX, "env 0 is clamped in step 0"
    if row.B >= 2:
        assert trace.velocity[0, 0] == S.V_MAX and trace.velocity[0, 1] == -S.V_MAX, "the clamp acts on both signs"
    if row.entry == "step_env":
        assert trace.done[3, 0] and not trace.done[1, 0] and trace.done[1, 1]
        assert (trace.velocity[trace.done] == 0).all() and (trace.workspace[:, trace.done[-1]] == 0).all()
        assert (trace.workspace[:, ~trace.done[-1]] != 0).any(axis=0).all()
    else:
        assert not trace.done.any()


# ---------------------------------------------------------------- the twin of step_env
@pytest.mark.parametrize("row", S.ENV_ROWS[:6], ids=S.ENV_IDS[:6])
def test_twin_of_step_env_is_the_checkers_step_on_the_envs_that_are_not_done(row):
    s, cfg = S.script(row), S.config(row)
    env, plain = R.Twin(cfg), R.Twin(cfg)
    env.commanded_velocity[:] = plain.commanded_velocity[:] = s.v0
    for t in range(S.STEPS):
        before_ws, before_v = env.workspace.copy(), env.commanded_velocity.copy()
        plain.workspace[:], plain.commanded_velocity[:] = before_ws, before_v
        env.step_env(s.x0[t], s.act[t], s.contact[t], s.done[t], S.DT)
        plain.step(s.x0[t], s.target[t], s.contact[t], S.DT)
        done = s.done[t] != 0
        assert np.array_equal(env.workspace[:, ~done], plain.workspace[:, ~done]) and np.array_equal(env.commanded_velocity[~done], plain.commanded_velocity[~done])
        assert (env.workspace[:, done] == 0).all() and (env.commanded_velocity[done] == 0).all()
        assert not done[np.signbit(s.done[t]) & (s.done[t] == 0)].any()


# ---------------------------------------------------------------- sharpness
@ROWS
@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_the_gpu_test_would_notice(row, mutation):
    """The mutated twin fails the comparison against the right one, which stands in for a right device here."""
    right = S.twin_trace(row)
    assert S.compare(row, right, right) == {"first_input": 0.0, "velocity": 0.0, "plan": 0.0, "dual": 0.0}
    wrong = S.run_twin(row, mutation)
    if S.applies(mutation, row):
        with pytest.raises(AssertionError):
            S.compare(row, wrong, right)
    elif row.N > 1:  # (a step row has neither a done row nor an action to read)
        assert all(np.array_equal(a, b) for a, b in zip(wrong, right))
