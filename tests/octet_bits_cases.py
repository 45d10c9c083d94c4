"""The cases of tests/test_octet_bits_gpu.py, shared with the recorder of its fixture (tools/make_golden_octet_bits.py).

Each case seeds a small batch so that ONE named path of the eight-lane step kernels (csrc/octet.hpp) is taken inside
40 env.step() calls, runs them and returns every word the launches wrote as raw bit patterns: the whole state, the
per-step records and flags, and the rare-path census (`upkie_sim_set_census`) that proves which path ran. `path_taken`
says what the census (and the episode counters) must show for the case to be the case its name says."""

import numpy as np
import torch

import bench
from upkie_amd import abi
from upkie_amd.sim import BatchedSim

STEPS = 40
ROLLOUT_STEPS_PER_LAUNCH = 4
# 8 envs: one full wavefront; 9: a second wavefront with one env and 56 idle lanes; 17: an odd count across the swizzle
SHAPES = (8, 9, 17)
HIP_UPPER, KNEE_UPPER = 1.26, 2.51  # the default model's stops (upkie_amd/model/default_model.py)


def _spread(sim, scale):
    """A small per-env factor 1 + scale * i / B: the envs of a case are near each other, never equal."""
    B = sim.num_envs
    return 1.0 + scale * torch.arange(B, dtype=torch.float32, device=sim.device) / B


def _pitch(sim, pitch):
    sim.state[abi.S_QUAT + 0] = torch.cos(0.5 * pitch)
    sim.state[abi.S_QUAT + 1] = 0.0
    sim.state[abi.S_QUAT + 2] = torch.sin(0.5 * pitch)
    sim.state[abi.S_QUAT + 3] = 0.0


def seed_calm(sim):
    """Balancing from the bench workload's own reset (the robots land first: a few substeps of the first steps are answered
    by lam = 0 or an active set; no sweep, no joint stop, no fall)."""


def seed_restart(sim):
    """A pitch just inside `fall_pitch` (1 rad) and a pitch rate that carries it across: the env is flagged done and the
    NEXT_STEP autoreset restarts it in the following launch."""
    _pitch(sim, 0.985 * _spread(sim, 0.01))
    sim.state[abi.S_ANGVEL + 1] = 2.0


def seed_unloading(sim):
    """The base moving up right after a reset: both tires are still inside the contact threshold, neither normal row asks
    for an impulse, the direct solution pulls -- not admissible, answered by lam = 0 without a solve."""
    sim.state[abi.S_LINVEL + 2] = 0.4 * _spread(sim, 0.2)


def seed_spinning_wheels(sim):
    """Wheels spinning fast against the commanded velocity: the velocity servo saturates at the torque limit (1.7 N m
    against mu N r = 1.35 N m a tire can transmit), the tires skid: friction rows on their bounds, an active set."""
    s = _spread(sim, 0.3)
    sim.state[abi.S_QD + 2] = 60.0 * s
    sim.state[abi.S_QD + 5] = -60.0 * s


def seed_tumbling(sim):
    """The same wheels under a trunk that rolls, yaws and slides sideways: the tires skid across their rolling direction
    while one of them unloads, the sets change from attempt to attempt and some substeps end in the Gauss-Seidel sweeps."""
    s = _spread(sim, 0.3)
    roll = 0.1 * s
    sim.state[abi.S_QUAT + 0] = torch.cos(0.5 * roll)
    sim.state[abi.S_QUAT + 1] = torch.sin(0.5 * roll)
    sim.state[abi.S_QUAT + 2] = 0.0
    sim.state[abi.S_QUAT + 3] = 0.0
    sim.state[abi.S_ANGVEL + 0] = 2.0
    sim.state[abi.S_ANGVEL + 2] = 6.0 * s
    sim.state[abi.S_LINVEL + 1] = 1.0
    sim.state[abi.S_QD + 2] = 60.0 * s
    sim.state[abi.S_QD + 5] = -60.0 * s


def seed_joint_stop(sim):
    """A hip (even envs) or a knee (odd envs) within reach of its upper stop and moving towards it."""
    B = sim.num_envs
    even = (torch.arange(B, device=sim.device) % 2) == 0
    zero = torch.zeros(B, device=sim.device)
    hip = torch.where(even, zero + (HIP_UPPER - 0.004), zero)
    knee = torch.where(even, zero, zero + (KNEE_UPPER - 0.004))
    for leg in range(2):
        sim.state[abi.S_Q + 3 * leg + 0] = hip
        sim.state[abi.S_Q + 3 * leg + 1] = knee
        sim.state[abi.S_QD + 3 * leg + 0] = torch.where(even, zero + 1.0, zero)
        sim.state[abi.S_QD + 3 * leg + 1] = torch.where(even, zero, zero + 1.0)
        sim.state[abi.S_LEGREF + 2 * leg + 0] = hip
        sim.state[abi.S_LEGREF + 2 * leg + 1] = knee


SEEDS = {
    "calm": seed_calm,
    "restart": seed_restart,
    "unloading": seed_unloading,
    "active_set": seed_spinning_wheels,
    "sweeps": seed_tumbling,
    "joint_stop": seed_joint_stop,
}

# (path, mode, envs): every path at every shape in the headline mode; the fused rollout and the Servos instantiation at 8 envs
CASES = [(path, "agent", envs) for path in SEEDS for envs in SHAPES]
CASES += [("restart", "rollout", 8), ("active_set", "rollout", 8), ("joint_stop", "servos", 8), ("active_set", "servos", 8)]


def case_id(case):
    return "-".join(str(x) for x in case)


def run_case(case):
    """Run one case; returns {name: array} of bit patterns (uint32 / uint8) and the census counters (int64)."""
    path, mode, envs = case
    sim = BatchedSim(bench.make_config(envs, seed=3))
    assert sim.lanes_per_env == 8
    sim.reset()
    sim.obs4.copy_(sim.obs6[:, [1, 0, 4, 3]])
    SEEDS[path](sim)
    episodes_before = int(sim.state[abi.S_EPISODE].sum())
    census = sim.enable_census()
    records, term, trunc = [], [], []
    if mode == "agent":
        for _ in range(STEPS):
            obs, _, terminated, truncated = sim.step_pendulum_agent()
            records.append(obs.clone())
            term.append(terminated.clone())
            trunc.append(truncated.clone())
    elif mode == "rollout":
        prev = torch.zeros(envs, 8, device=sim.device)
        prev[:, :4] = sim.obs4
        ring = torch.zeros(ROLLOUT_STEPS_PER_LAUNCH, envs, 8, device=sim.device)
        for _ in range(STEPS // ROLLOUT_STEPS_PER_LAUNCH):
            sim.rollout_pendulum_records(prev, ring)
            prev.copy_(ring[-1])
            records.append(ring.clone())
    elif mode == "servos":
        # hips and knees commanded beyond their stops, wheels a velocity they cannot reach: every joint at a limit of its own
        act = torch.zeros(envs, 6, 6, device=sim.device)
        act[:, :, 3] = 1.0
        act[:, :, 4] = 1.0
        for j, (position, velocity, torque) in enumerate([(2.0, 0.0, 16.0), (3.0, 0.0, 16.0), (float("nan"), 100.0, 1.7)] * 2):
            act[:, j, 0], act[:, j, 1], act[:, j, 5] = position, velocity, torque
        act[:, 5, 1] = -100.0
        for _ in range(STEPS):
            obs, _, terminated, truncated = sim.step_servos(act)
            records.append(obs.clone())
            term.append(terminated.clone())
            trunc.append(truncated.clone())
    else:
        raise ValueError(mode)
    torch.cuda.synchronize()
    out = {
        "state": sim.state.cpu().numpy().view(np.uint32),
        "records": torch.stack(records).cpu().numpy().view(np.uint32),
        "census": census.cpu().numpy().astype(np.int64),
        "episodes": np.array([int(sim.state[abi.S_EPISODE].sum()) - episodes_before], dtype=np.int64),
    }
    if term:
        out["terminated"] = torch.stack(term).cpu().numpy()
        out["truncated"] = torch.stack(trunc).cpu().numpy()
    sim.close()
    return out


def path_taken(case, out):
    """None when the census and the episode counters show the path the case is named for, else what is missing."""
    path, mode, _ = case
    c = dict(zip(BatchedSim.CENSUS_FIELDS, out["census"][:8].tolist()))
    episodes = int(out["episodes"][0])
    if path == "calm":
        ok = c["joint_limit"] == 0 and c["sweeps_total"] == 0 and episodes == 0
    elif path == "restart":
        ok = episodes > 0
    elif path == "unloading":
        # not-admissible env-substeps that neither an active set nor the sweeps answered: the lam = 0 exit, and far more often
        # than the landing of the calm case takes it
        ok = c["sweeps_total"] == 0 and c["friction_cone"] - c["active_set_solves"] > 50 * out["state"].shape[1]
    elif path == "active_set":
        ok = c["active_set_solves"] > 0
    elif path == "sweeps":
        ok = c["sweeps_total"] > 0 and c["wavefront_substeps_sweeps"] > 0
    elif path == "joint_stop":
        ok = c["joint_limit"] > 0 and c["wavefront_substeps_limit"] > 0
    else:
        raise ValueError(path)
    return None if ok else f"{case_id(case)}: path not taken: {c}, episodes ended {episodes}"
