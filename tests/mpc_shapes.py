"""The shapes the MPC balancer (upkie_amd/csrc/mpc.hpp: `mpc_tile_h<T, COLUMNS>` behind `upkie_mpc_step` and
`upkie_mpc_step_env`) is tested at, and the builders the tests share: the geometry of a row as the header computes it, its
settings, its scripted inputs and the fp64 twin's run of them, all plain numpy under seeds of the row.

A row is (horizon N, batch B, entry point, overrides of `abi.default_mpc_config`). `MATRIX` is no cross product: every row
says what it is there for. tests/test_mpc_matrix.py asserts that the table covers what it claims and that the inputs decide
what they should, tests/test_mpc_matrix_gpu.py runs every row on the device."""

import ctypes as C
import functools
from collections import namedtuple

import numpy as np

from tests import mpc_reference as R
from upkie_amd import abi

DEV = "cuda:0"
F32 = np.float32
DT = 0.005
STEPS = 4  # tests/test_parity_gpu.py::test_mpc_step_matches_oracle's: two interior steps, two at scale 5
POOL = 500  # envs of a horizon's script; a smaller batch reads the first rows
# Chosen for the two conditions tests/test_mpc_matrix.py sets on the inputs (the checker within 2e-3 a_max of the exact QP on every
# tenth env, 5 .. 90 % of the plan at the bound in the saturating steps): on random saturating states about one solve in a
# thousand is further from the exact QP than that after the fixed number of iterations, and the projected Newton method
# itself gives up on a few QPs at N = 63 / 64. Of the seeds 1 .. 24, 14 and 20 meet both conditions on every row (worst
# share of the bound 0.13 and 0.25).
SEED = 14
FALL_PITCH, V_MAX, A_MAX = 1.0, 3.0, 10.0  # abi.default_mpc_config's (tests/test_mpc_matrix.py holds them to it)

# the bounds of tests/test_parity_gpu.py::test_mpc_step_matches_oracle
FIRST_INPUT_BOUND = 1e-4 * A_MAX
VELOCITY_BOUND = 5e-6
PLAN_BOUND = 2e-3
DUAL_BOUND = 4e-3
EXACT_BOUND = 2e-3 * A_MAX

Row = namedtuple("Row", "N B entry relaxation iterations rho leg_length why")


def _step(N, B, why, **kw):
    return Row(N, B, "step", kw.get("relaxation"), kw.get("iterations"), kw.get("rho"), kw.get("leg_length"), why)


def _env(N, B, why):
    return Row(N, B, "step_env", None, None, None, None, why)


_HORIZONS = [
    (1, "only element (t0, g0, r0) is real: 63 of a lane's 64 rows are padding"),
    (2, "lane groups 0 and 1 hold one real element each, in register 0; groups 2 and 3 hold padding alone"),
    (3, "lane group 3 holds padding alone"),
    (4, "every lane group holds exactly one real element, register 0"),
    (5, "the first real element in register 1"),
    (15, "one padding element per column"),
    (16, "tests/test_parity_gpu.py's; T = 1 without padding"),
    (17, "tests/test_parity_gpu.py's; T = 2, KJ = 1, a second tile with one real row"),
    (31, "T = 2 with one padding element"),
    (32, "tests/test_parity_gpu.py's; T = 2 without padding"),
    (33, "tests/test_parity_gpu.py's; T = 3, KJ = 2: the second 32-wide K-step is half padding, its tile has one real row"),
    (47, "T = 3 with one padding element"),
    (48, "tests/test_parity_gpu.py's; T = 3 without padding"),
    (49, "tests/test_parity_gpu.py's; T = 4, a fourth tile with one real row"),
    (50, "tests/test_parity_gpu.py's; the reference's default horizon"),
    (51, "T = 4, three real rows in the last tile"),
    (63, "T = 4 with one padding element"),
    (64, "tests/test_parity_gpu.py's; the longest horizon, no padding anywhere"),
]
_BATCHES = [
    (1, "one env: one block with one live column"),
    (15, "one block, one dead column"),
    (16, "one full wave, one block"),
    (17, "two blocks, the second with one live column"),
    (100, "7 blocks: the XCD remap is the identity, the tail has 4 columns"),
    (128, "8 full blocks, remapped"),
    (129, "9 blocks: identity, one live column in the last"),
]

MATRIX = (
    [_step(N, 500, why) for N, why in _HORIZONS]
    + [_step(N, B, why) for B, why in _BATCHES for N in (1, 15, 50)]
    + [_env(N, B, f"step_env (stride 2, done rows, null first_input) at T = {(N + 15) // 16}, {(B + 15) // 16} blocks")
       for N in (1, 7, 16, 33, 50) for B in (17, 100, 500)]
    + [_step(N, 500, "admm_relaxation = 0 means unset: alpha = 1, beta2 = 0, every carry term drops out", relaxation=0.0) for N in (2, 16, 50)]
    + [_step(N, 500, f"{it} iteration{'s' if it > 1 else ''} instead of the default", iterations=it) for it in (1, 2, 31) for N in (15, 50)]
    + [_step(N, 256, "tests/test_parity_gpu.py::test_mpc_other_solver_settings_and_models's", rho=rho, relaxation=alpha, leg_length=leg)
       for N, rho, alpha, leg in [(50, 1e-4, 1.5, 0.58), (50, 1e-2, 1.0, 0.58), (16, 1e-5, 1.6, 0.4), (32, 1e-1, 1.2, 0.7)]]
)
# what the device suite ran before this table: (N, B) of test_mpc_step_matches_oracle, then (N, rho, relaxation, leg_length) of
# test_mpc_other_solver_settings_and_models at B = 256
EXISTING = [(N, 500) for N in (16, 17, 32, 33, 48, 49, 50, 64)]
EXISTING_SETTINGS = [(50, 1e-4, 1.5, 0.58), (50, 1e-2, 1.0, 0.58), (16, 1e-5, 1.6, 0.4), (32, 1e-1, 1.2, 0.7)]


def default_settings(row):
    return row.relaxation is None and row.iterations is None and row.rho is None and row.leg_length is None


def row_id(row):
    parts = [f"N{row.N}", f"B{row.B}", row.entry]
    for tag, value in (("alpha", row.relaxation), ("it", row.iterations), ("rho", row.rho), ("leg", row.leg_length)):
        if value is not None:
            parts.append(f"{tag}{value:g}")
    return "-".join(parts)


IDS = [row_id(r) for r in MATRIX]
ENV_ROWS = [r for r in MATRIX if r.entry == "step_env"]
ENV_IDS = [row_id(r) for r in ENV_ROWS]


def config(row, num_envs=None):
    cfg = abi.default_mpc_config(row.B if num_envs is None else num_envs, row.N)
    if row.relaxation is not None:
        cfg.admm_relaxation = row.relaxation
    if row.iterations is not None:
        cfg.admm_iterations = row.iterations
    if row.rho is not None:
        cfg.admm_rho = row.rho
    if row.leg_length is not None:
        cfg.leg_length = row.leg_length
    return cfg


# ---------------------------------------------------------------- the geometry, as csrc/mpc.hpp and the C-ABI compute it
def mpc_index(t, g, r):
    """Horizon index of element (row tile t, lane group g, register r)."""
    return 16 * t + 4 * r + g


def tiles(N):
    return (N + 15) // 16


def k_steps(T):
    """KJ: the 32-wide K-steps of a product over T row tiles."""
    return (T + 1) // 2


def grid(B):
    return (B + 15) // 16


def remapped(B):
    """Whether the kernel permutes its blocks over the XCDs: a grid that is a multiple of 8."""
    return grid(B) % 8 == 0


def last_block_columns(B):
    return B - 16 * (grid(B) - 1)


def real_elements(N, g):
    """The (t, r) of lane group g that lie inside the horizon."""
    return [(t, r) for t in range(tiles(N)) for r in range(4) if mpc_index(t, g, r) < N]


def geometry(row):
    T = tiles(row.N)
    return {"T": T, "KJ": k_steps(T), "grid": grid(row.B), "remapped": remapped(row.B), "last_columns": last_block_columns(row.B),
            "padding_only_groups": [g for g in range(4) if not real_elements(row.N, g)], "last_tile_rows": row.N - 16 * (T - 1)}


# ---------------------------------------------------------------- scripted inputs
Script = namedtuple("Script", "x0 target contact act done v0")


@functools.lru_cache(maxsize=None)
def _pool(N):
    """The inputs of horizon N for POOL envs, generated in float32 (both sides read the same values, so no decision rests
    on input rounding). The parity test's four steps; about a tenth of the envs lie beyond `fall_pitch` with their wheels
    on the ground (|pitch| in 1.05 .. 1.3 fall_pitch, the same envs on the same side at every step: an unrelated warm start
    with the duals of such a state is not what the iteration count is for; every other pitch stays below 0.75) and about
    a tenth are in the air. The commanded velocity is preloaded, uniform in +-1.02 max_ground_velocity. `done` (step_env rows):
    about 15 % of the envs at steps 1 and 3, as 1 or 2.5; -0.0 on some others, which does not mean done.
    The head of the pool is scripted, so that every batch size sees every branch decide something:
      env 0  starts above +max_ground_velocity, upright and touching: step 0 clamps it; step 1 finds it fallen but touching;
             its `done` word is -0.0 at step 1 and 2.5 at step 3
      env 1  the same at -max_ground_velocity; done (1.0) at step 1
      env 2 / env 3  start 0.01 inside the upper / the lower bound, upright and touching at step 0"""
    rng = np.random.default_rng([SEED, N])
    B = POOL
    # a robot that lies on the ground stays there, on the same side; so does one in the air
    kind, side = rng.uniform(size=B), rng.choice([-1.0, 1.0], B)
    kind[:4] = 1.0
    x0, target, contact, done = [], [], [], []
    for step in range(STEPS):
        scale = 1.0 if step < 2 else 5.0
        x = np.stack([rng.uniform(-0.5, 0.5, B), rng.uniform(-0.15, 0.15, B) * scale, rng.uniform(-0.5, 0.5, B) * scale,
                      rng.uniform(-0.5, 0.5, B) * scale], axis=1)
        over = side * rng.uniform(1.05, 1.3, B) * FALL_PITCH
        if step == 1:
            kind[0] = 0.0
        fallen, airborne = kind < 0.1, (kind >= 0.1) & (kind < 0.2)
        x[fallen, 1] = over[fallen]
        x[fallen, 2:] /= scale  # (it lies there: nothing drives its velocities up)
        x0.append(x.astype(F32))
        target.append(rng.uniform(-0.5, 0.5, B).astype(F32))
        contact.append((~airborne).astype(np.uint8))
        d = rng.uniform(size=B)
        flags = np.where(d < 0.075, 1.0, np.where(d < 0.15, 2.5, np.where(d < 0.3, -0.0, 0.0))).astype(F32)
        if step not in (1, 3):
            flags[:] = 0.0
        if step == 1:
            flags[0], flags[1] = -0.0, 1.0
        if step == 3:
            flags[0] = 2.5
        done.append(flags)
    v0 = rng.uniform(-1.02 * V_MAX, 1.02 * V_MAX, B).astype(F32)
    v0[:4] = [1.017 * V_MAX, -1.017 * V_MAX, V_MAX - 0.01, -(V_MAX - 0.01)]
    x0, target, contact, done = np.stack(x0), np.stack(target), np.stack(contact), np.stack(done)
    act = np.stack([target, np.full_like(target, np.nan)], axis=2)  # column 1 is never the balancer's to read
    out = Script(x0, target, contact, act, done, v0)
    for a in out:
        a.setflags(write=False)
    return out


def script(row, envs=None):
    """The scripted run of a row: `x0` [STEPS, B, 4], `target` [STEPS, B], `contact` [STEPS, B] uint8, `act` [STEPS, B, 2]
    (column 0 the target, column 1 NaN), `done` [STEPS, B] float32, `v0` [B]: the commanded velocity before the first step.
    `envs`: these envs of the pool instead of the first B. Read-only."""
    s = _pool(row.N)
    pick = slice(0, row.B) if envs is None else np.asarray(envs)
    return Script(s.x0[:, pick], s.target[:, pick], s.contact[:, pick], s.act[:, pick], s.done[:, pick], s.v0[pick])


def fallen_but_touching(s, step):
    return (np.abs(s.x0[step][:, 1]) > FALL_PITCH) & (s.contact[step] != 0)


# ---------------------------------------------------------------- the twin's run of a script
Trace = namedtuple("Trace", "first velocity plan0 workspace done")


def run_twin(row, mutation=None):
    """What every step leaves: `first` [STEPS, B] (step rows: the first input; step_env rows: word 0 of the plan, which is
    the same number), `velocity` [STEPS, B], `plan0` [STEPS, B], the last `workspace` [2 N, B], and `done` [STEPS, B]: the
    envs that a step reset instead of solving."""
    s, tw = script(row), R.Twin(config(row), mutation)
    tw.commanded_velocity[:] = s.v0
    first, velocity, plan0, done = [], [], [], []
    for t in range(STEPS):
        if row.entry == "step":
            tw.step(s.x0[t], s.target[t], s.contact[t], DT)
            done.append(np.zeros(row.B, dtype=bool))
            first.append(tw.first_input.copy())
        else:
            tw.step_env(s.x0[t], s.act[t], s.contact[t], s.done[t], DT)
            done.append(s.done[t] != 0)
            first.append(tw.workspace[0].copy())
        velocity.append(tw.commanded_velocity.copy())
        plan0.append(tw.workspace[0].copy())
    out = Trace(np.stack(first), np.stack(velocity), np.stack(plan0), tw.workspace.copy(), np.stack(done))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def twin_trace(row):
    """The unmutated twin's, computed once and shared (about half a MiB per row)."""
    return run_twin(row)


def checked_envs(row):
    """Every tenth env: the ones held to the exact QP."""
    return np.arange(0, row.B, 10)


@functools.lru_cache(maxsize=None)
def exact_first_inputs(row):
    """[STEPS, len(checked_envs)]: the first input of the exact solution of each step's QP (`oracle_mpc_solve_exact`, a
    projected Newton method on the fp64 problem)."""
    from oracle import oracle as O

    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    N, cfg, s, envs = row.N, config(row), script(row), checked_envs(row)
    P, Kx, kv = np.zeros((N, N)), np.zeros((N, 4)), np.zeros(N)
    O.lib().oracle_mpc_build(C.byref(cfg), p(P), p(Kx), p(kv))
    out = np.zeros((STEPS, len(envs)))
    for t in range(STEPS):
        q = s.x0[t].astype(np.float64) @ Kx.T + np.outer(s.target[t].astype(np.float64), kv)
        for i, e in enumerate(envs):
            u = np.zeros(N)
            assert O.lib().oracle_mpc_solve_exact(N, p(P), p(np.ascontiguousarray(q[e])), C.c_double(cfg.max_ground_accel), p(u)) >= 0
            out[t, i] = u[0]
    out.setflags(write=False)
    return out


# ---------------------------------------------------------------- the comparison (tests/test_mpc_matrix_gpu.py)
def applies(mutation, row):
    """Whether a row has the feature that a mutation of the twin (tests/mpc_reference.py) breaks."""
    if mutation == "drop_last_index":
        return row.N > 1
    if mutation in ("ignore_done", "target_stride_1"):
        return row.entry == "step_env"
    return True


def shares(row, got, want):
    """The worst error of a run `got` (a Trace: the device's) against the twin's `want`, each as a share of its bound from
    the parity test: over the steps the first input (envs that the step solved) and the commanded velocity, after the
    last step the plan and the duals."""
    out = {"first_input": 0.0, "velocity": 0.0}
    for t in range(STEPS):
        solved = ~want.done[t]
        if solved.any():
            out["first_input"] = max(out["first_input"], float(np.abs(got.first[t] - want.first[t])[solved].max()) / FIRST_INPUT_BOUND)
        out["velocity"] = max(out["velocity"], float(np.abs(got.velocity[t] - want.velocity[t]).max()) / VELOCITY_BOUND)
    N = row.N
    out["plan"] = float(np.abs(got.workspace[:N] - want.workspace[:N]).max()) / PLAN_BOUND
    out["dual"] = float(np.abs(got.workspace[N:] - want.workspace[N:]).max()) / DUAL_BOUND
    return out


def compare(row, got, want):
    """`shares`, asserted: every word finite and no share above 1. Returns the shares."""
    assert np.isfinite(got.workspace).all() and np.isfinite(got.velocity).all() and np.isfinite(got.first).all()
    out = shares(row, got, want)
    for kind, share in out.items():
        assert share <= 1.0, (row_id(row), kind, out)
    return out


def exact_share(row, trace):
    """The worst distance of a run's first inputs from the exact QP's, every tenth env, as a share of 2e-3 a_max."""
    envs, exact = checked_envs(row), exact_first_inputs(row)
    solved = ~trace.done[:, envs]
    return float((np.abs(trace.first[:, envs] - exact) * solved).max()) / EXACT_BOUND


# ---------------------------------------------------------------- device helpers (torch is imported by the GPU tests only)
def _dev(a, dtype=None):
    import torch

    return torch.as_tensor(np.array(a, order="C"), dtype=dtype).to(DEV)  # (a copy: the scripts are read-only)


def _np(t):
    return t.detach().cpu().numpy()


def balancer(row, num_envs=None):
    from upkie_amd.mpc import BatchedMpc

    return BatchedMpc(config(row, num_envs), device=DEV)


def run_device(row, s=None, entry=None, done=True, mpc=None, close=True):
    """The script `s` (the row's own by default) on the device through `entry` (the row's by default): a Trace in fp64, its
    `workspace` and `velocity` the device's float32 words widened. `done` False: step_env is given a row of zeros."""
    s = script(row) if s is None else s
    entry = entry or row.entry
    B = s.v0.shape[0]
    mpc = mpc or balancer(row, B)
    mpc.commanded_velocity.copy_(_dev(s.v0))
    first, velocity, plan0, flags = [], [], [], []
    for t in range(STEPS):
        x0, contact = _dev(s.x0[t]), _dev(s.contact[t])
        if entry == "step":
            _, u0 = mpc.step(x0, _dev(s.target[t]), contact, DT)
            flags.append(np.zeros(B, dtype=bool))
            first.append(_np(u0).astype(np.float64))
        else:
            d = s.done[t] if done else np.zeros_like(s.done[t])
            mpc.step_env(x0, _dev(s.act[t]), contact, _dev(d), DT)
            flags.append(d != 0)
            first.append(_np(mpc.workspace[0]).astype(np.float64))
        velocity.append(_np(mpc.commanded_velocity).astype(np.float64))
        plan0.append(_np(mpc.workspace[0]).astype(np.float64))
    out = Trace(np.stack(first), np.stack(velocity), np.stack(plan0), _np(mpc.workspace).astype(np.float64), np.stack(flags))
    if close:
        mpc.close()
    return out


@functools.lru_cache(maxsize=None)
def device_trace(row):
    """The device's run of a row, once: the row's own test and the mutation tests read the same run."""
    return run_device(row)
