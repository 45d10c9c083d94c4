"""The MPC balancer on the device at every row of tests/mpc_shapes.py: each (horizon, batch, entry point, settings) against
the fp64 twin (tests/mpc_reference.py) under the bounds of tests/test_parity_gpu.py::test_mpc_step_matches_oracle, and
against the exact QP on the default-settings rows; `step_env` with no env done against `step`, bit for bit; an env's solve
against the same env's solve in another batch, at another column, and beside a solve that leaves fp16's range; the masked
reset; the balancer inside the step's launch against the two launches; and every mutation of the twin against the device,
which the comparison must refuse.

`python -m tests.test_mpc_matrix_gpu` prints the table of profiles/mpc_matrix.txt."""

import time

import numpy as np
import pytest
import torch

from tests import mpc_reference as R
from tests import mpc_shapes as S

pytestmark = pytest.mark.gpu

ROWS = pytest.mark.parametrize("row", S.MATRIX, ids=S.IDS)
TILE_HORIZONS = [5, 16, 32, 48, 50]  # T = 1 (with and without padding), 2, 3, 4


def step_row(N, B=500):
    return next(r for r in S.MATRIX if (r.N, r.B, r.entry) == (N, B, "step") and S.default_settings(r))


# ---------------------------------------------------------------- every row against the twin
@ROWS
def test_row_matches_the_twin(row):
    """After every step the first input within 1e-4 a_max and the commanded velocity within 5e-6; after the last the plan
    within 2e-3 and the duals within 4e-3; every workspace word finite; default-settings rows within 2e-3 a_max of the exact
    QP on every tenth env. No row has a bound of its own.

    Measured on one MI355X (profiles/mpc_matrix.txt): over all rows the first input reaches 0.050 of its bound, the commanded
    velocity 0.086, the plan 0.15, the duals 0.88, the distance from the exact QP 0.13; below N = 16 no distance from the
    twin reaches a hundredth of its bound but the velocity's (0.08: fp32 roundings of a value of 3). The duals come closest
    at N = 48 .. 51 (0.88 / 0.87 / 0.51 / 0.85), on the envs that lie beyond `fall_pitch`: their duals are 1.3e3 .. 2.2e3 and
    the error 2e-6 of the value. With the dual as the C operand of the product's first MFMA these rows missed the bound
    (1.35 / 0.98 / 0.95 / 1.13): the accumulators of `mpc_tile_h` start from 0 since."""
    got, want = S.device_trace(row), S.twin_trace(row)
    exact = S.exact_share(row, got) if S.default_settings(row) else 0.0
    print(f"mpc {S.row_id(row)}: shares of the bounds {S.shares(row, got, want)} exact QP {exact:.4f}")
    S.compare(row, got, want)
    assert exact <= 1.0, (S.row_id(row), exact)


@pytest.mark.parametrize("row", S.ENV_ROWS, ids=S.ENV_IDS)
def test_step_env_with_nobody_done_is_step(row):
    """Stride 2 instead of 1, a `done` row of zeros, no first_input: the same workspace and commanded velocity, bit for bit,
    as `step` on the same inputs."""
    a = S.run_device(row, entry="step")
    b = S.run_device(row, entry="step_env", done=False)
    assert np.array_equal(a.workspace, b.workspace) and np.array_equal(a.velocity, b.velocity) and np.array_equal(a.plan0, b.plan0)
    assert np.abs(a.workspace).max() > 0 and not np.array_equal(a.velocity[-1], S.script(row).v0)


# ---------------------------------------------------------------- one env's solve is its own
def _scattered(N, count=37):
    """`count` envs of the 500, in no order: the ends of the batch, both sides of a block's edge, the rest at random."""
    rng = np.random.default_rng([S.SEED, N, count])
    fixed = [499, 0, 16, 15, 484, 483]
    rest = rng.permutation([e for e in range(500) if e not in fixed])[:count - len(fixed)]
    return rng.permutation(np.concatenate([fixed, rest]).astype(np.int64))


@pytest.mark.parametrize("N", TILE_HORIZONS)
def test_an_envs_solve_does_not_depend_on_its_batch(N):
    """37 envs of the batch of 500 again as a batch of 37 in a permuted order (another column, another block, another grid
    and remap): the same bits. The MFMA's columns are independent and the A operand is shared."""
    row, envs = step_row(N), _scattered(N)
    assert len(set(envs.tolist())) == 37
    big = S.device_trace(row)
    small = S.run_device(row, s=S.script(row, envs))
    assert np.array_equal(small.first, big.first[:, envs]) and np.array_equal(small.velocity, big.velocity[:, envs])
    assert np.array_equal(small.workspace, big.workspace[:, envs])


@pytest.mark.parametrize("N", TILE_HORIZONS)
def test_a_solve_that_leaves_fp16s_range_is_discarded_alone(N):
    """A target of 1e30 (tests/test_nonfinite_guard_gpu.py's) in one env at the last step: every other env's bits are those
    of the run without it; its own columns come back zero, its first input 0, and its commanded velocity decays as for a
    fallen robot."""
    row = step_row(N)
    s, clean = S.script(row), S.device_trace(row)
    upright = (np.abs(s.x0[-1][:, 1]) < S.FALL_PITCH) & (s.contact[-1] != 0) & (np.abs(clean.velocity[-2]) > 1.0)
    bad = int(np.nonzero(upright)[0][np.nonzero(upright)[0] >= 100][0])  # (inside the batch, away from the scripted head)
    target = s.target.copy()
    target[-1, bad] = 1e30
    act = np.stack([target, np.full_like(target, np.nan)], axis=2)
    got = S.run_device(row, s=s._replace(target=target, act=act))
    others = np.arange(row.B) != bad
    assert np.isfinite(got.workspace).all() and np.isfinite(got.velocity).all() and np.isfinite(got.first).all()
    assert np.array_equal(got.workspace[:, others], clean.workspace[:, others])
    assert np.array_equal(got.velocity[:, others], clean.velocity[:, others]) and np.array_equal(got.first[:, others], clean.first[:, others])
    assert np.array_equal(got.velocity[:-1], clean.velocity[:-1]) and np.array_equal(got.first[:-1], clean.first[:-1])
    print(f"mpc N={N} poisoned env {bad}: |plan| {np.abs(got.workspace[:N, bad]).max():.3g} |duals| {np.abs(got.workspace[N:, bad]).max():.3g} "
          f"first input {got.first[-1, bad]:.3g} velocity {got.velocity[-2, bad]:.6f} -> {got.velocity[-1, bad]:.6f}")
    assert (got.workspace[:, bad] == 0).all() and got.first[-1, bad] == 0
    before = got.velocity[-2, bad]
    assert abs(got.velocity[-1, bad] - (before + (S.DT / 0.1) * (0.0 - before))) <= S.VELOCITY_BOUND


# ---------------------------------------------------------------- the masked reset
@pytest.mark.parametrize("B", [1, 17, 129])
@pytest.mark.parametrize("N", [1, 50])
def test_masked_reset(N, B):
    row = step_row(N, B)
    mpc = S.balancer(row)
    S.run_device(row, mpc=mpc, close=False)
    ws, v = mpc.workspace.clone(), mpc.commanded_velocity.clone()
    assert bool((ws != 0).any(dim=0).all()) and bool((v != 0).all())
    mask = np.random.default_rng([S.SEED, N, B]).uniform(size=B) < 0.5
    mask[0] = B == 1  # (a batch of one: first the reset that masks nobody, then the one that takes it)
    mask[-1] = True
    for m in (mask if B > 1 else ~mask, ~mask if B > 1 else mask):
        hit = torch.from_numpy(m).to(S.DEV)
        mpc.reset(hit.to(torch.uint8))
        assert float(mpc.workspace[:, hit].abs().sum()) == 0.0 and float(mpc.commanded_velocity[hit].abs().sum()) == 0.0
        assert torch.equal(mpc.workspace[:, ~hit], ws[:, ~hit]) and torch.equal(mpc.commanded_velocity[~hit], v[~hit])
        ws, v = mpc.workspace.clone(), mpc.commanded_velocity.clone()
    assert float(ws.abs().sum()) == 0.0 and float(v.abs().sum()) == 0.0
    mpc.close()


# ---------------------------------------------------------------- balancer and step in one launch
@pytest.mark.parametrize("B", [43, 50])
@pytest.mark.parametrize("lanes", ["2", "8"])
@pytest.mark.parametrize("nb_timesteps", [1, 5, 15, 17])
def test_balancer_and_step_in_one_launch_equal_two_launches(nb_timesteps, lanes, B, monkeypatch):
    """tests/test_baseline_configs_gpu.py::test_c3_balancer_and_step_in_one_launch_equal_two_launches at the horizons
    below 16 (`mpc_tile_h<1>` / `<1, 8>` inside the step's launch, every lane group padded) and at batch sizes whose last
    block is part empty: two lanes per env, second 16-env tile of the last block with none (43) and two (50) live envs; eight
    lanes per env, last octet with three and two. A horizon of 17 does not fit one tile: `fuse_mpc` then takes the two
    launches itself and gives the same bits. The two-launch side is `step_env`, which the rows above hold to the twin."""
    from upkie_amd import envs
    from upkie_amd.utils.robot_state import RobotState
    from upkie_amd.utils.robot_state_randomization import RobotStateRandomization

    monkeypatch.setenv("UPKIE_LANES_PER_ENV", lanes)
    kw = dict(num_envs=B, frequency=200.0, nb_timesteps=nb_timesteps, seed=0, fall_pitch=0.3,
              init_state=RobotState(randomization=RobotStateRandomization(pitch=0.29, x=0.05, omega_y=0.3, linear_velocity=np.array([0.2, 0.0, 0.0]))))
    one = envs.make("Upkie-HIP-BaseVelocity-Vec", **kw)
    two = envs.make("Upkie-HIP-BaseVelocity-Vec", **kw)
    one.fuse_mpc, two.fuse_mpc = True, False
    one.reset(seed=0)
    two.reset(seed=0)
    rng = np.random.default_rng(1)
    act = torch.zeros(B, 2)
    ended_before_the_last_step = 0
    for step in range(20):
        act[:, 0] = torch.from_numpy(rng.uniform(-0.8, 0.8, B)).float()
        act[:, 1] = torch.from_numpy(rng.uniform(-0.5, 0.5, B)).float()
        o1, _, t1, u1, _ = one.step(act)
        o2, _, t2, u2, _ = two.step(act)
        assert torch.equal(o1, o2) and torch.equal(t1, t2) and torch.equal(u1, u2), step
        if step < 19:
            ended_before_the_last_step += int(t1.sum()) + int(u1.sum())
    assert torch.equal(one.sim.state, two.sim.state)
    assert torch.equal(one.mpc_balancer.commanded_velocity, two.mpc_balancer.commanded_velocity)
    assert torch.equal(one.mpc_balancer.workspace, two.mpc_balancer.workspace)
    assert float(one.mpc_balancer.commanded_velocity.abs().max()) > 0.05  # the balancer did act
    assert ended_before_the_last_step >= 1, "no env was reset by `done`"
    print(f"mpc fused N={nb_timesteps} lanes={lanes} B={B}: {ended_before_the_last_step} episodes ended, max |v| {float(one.mpc_balancer.commanded_velocity.abs().max()):.3f}")
    one.close()
    two.close()


# ---------------------------------------------------------------- the comparison is sharp
@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_mutated_twin_fails_on_every_row_that_has_the_feature(mutation):
    """The device against a twin that is wrong in one way a kernel could be wrong: the comparison refuses it on every row
    the mutation applies to (the inputs are built so that each feature decides something in every row)."""
    rows = [r for r in S.MATRIX if S.applies(mutation, r)]
    assert len(rows) >= len(S.ENV_ROWS)
    missed = []
    for row in rows:
        got = S.device_trace(row)
        right, wrong = S.shares(row, got, S.twin_trace(row)), S.shares(row, got, S.run_twin(row, mutation))
        if not any(wrong[kind] > 1.0 >= right[kind] for kind in wrong):  # (refused for a reason the right twin does not share)
            missed.append((S.row_id(row), wrong))
    assert not missed, (mutation, missed)


# ---------------------------------------------------------------- the record
def main():
    print("# tests/test_mpc_matrix_gpu.py, every row of tests/mpc_shapes.py on one MI355X: the worst error against the fp64 twin as a share")
    print("# of its bound (first input 1e-4 a_max, commanded velocity 5e-6, plan 2e-3, duals 4e-3), the first input's worst distance from")
    print("# the exact QP as a share of 2e-3 a_max (default-settings rows), and the time of the row's device run, its balancer's creation included")
    print(f"{'row':<34} {'first':>8} {'velocity':>8} {'plan':>8} {'dual':>8} {'exact':>8} {'seconds':>8}")
    worst, slowest, beyond = {}, ("", 0.0), []
    for row in S.MATRIX:
        t0 = time.perf_counter()
        got = S.run_device(row)
        seconds = time.perf_counter() - t0
        shares = S.shares(row, got, S.twin_trace(row))
        exact = S.exact_share(row, got) if S.default_settings(row) else float("nan")
        print(f"{S.row_id(row):<34} {shares['first_input']:8.4f} {shares['velocity']:8.4f} {shares['plan']:8.4f} {shares['dual']:8.4f} {exact:8.4f} {seconds:8.3f}")
        beyond += [f"{S.row_id(row)} {k} {v:.4f}" for k, v in shares.items() if v > 1.0]
        for k, v in shares.items():
            worst[k] = max(worst.get(k, (0.0, "")), (v, S.row_id(row)))
        slowest = max(slowest, (S.row_id(row), seconds), key=lambda x: x[1])
    for k, (v, name) in worst.items():
        print(f"# worst {k} share {v:.4f} ({name})")
    print(f"# beyond a bound: {'; '.join(beyond) if beyond else 'no row'}")
    print(f"# slowest device run {slowest[1]:.3f} s ({slowest[0]})")


if __name__ == "__main__":
    main()
