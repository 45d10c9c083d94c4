"""The reference's OWN classes on this repository's side of the boundary
(VERDICT r1, item 8), replayed from tests/golden/reference_wrappers.json.gz,
which tools/make_golden_wrappers.py recorded while those classes ran unmodified
(gymnasium / loop_rate_limiters / upkie_description stubbed as in
tools/make_golden_envs.py):

* `UpkiePendulum(UpkieServos(backend=...))` (its own UpkieGyropod inside),
  `UpkieGyropod` and `UpkieServos` on top of
  `upkie_amd.envs.backends.HipBackend` -- the drop-in for `PyBulletBackend`
  (upkie/envs/backends/backend.py:11-50) -- over the fp64 CPU double of the
  simulation handle: the actions their scripted agents chose and what the
  wrappers returned. This repository's fused `UpkiePendulum` / `UpkieGyropod` /
  `UpkieServos` are given the same seeds and actions, on the same double, so
  the comparison isolates the wrapper arithmetic: the reference's Python
  (command maps, leg low-pass, clamps, observation maps, fall detection,
  init-state sampling) versus the step functions that restate it.
* the reference's `SpineInterface` (upkie/envs/backends/spine/spine_interface.py)
  as the agent of a `HipSpine`: the requests and msgpack payloads it wrote into
  the shared memory, written again verbatim, and the observations it read back.
"""

import base64
import gzip
import json
import os
import sys
import uuid

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with gzip.open(os.path.join(ROOT, "tests", "golden", "reference_wrappers.json.gz"), "rt") as f:
    GOLDEN = json.load(f)
SERVO_KEYS = ("position", "velocity", "torque")


def fused_env(kind):
    import upkie_amd.envs as envs
    from upkie_amd.utils.robot_state import RobotState
    from upkie_amd.utils.robot_state_randomization import RobotStateRandomization

    from .fake_sim import oracle_sim_factory

    rand = dict(pitch=0.1, x=0.05, omega_y=0.1, linear_velocity=np.array([0.05, 0.0, 0.0]))
    init = RobotState(position_base_in_world=np.array([0.0, 0.0, 0.6]), randomization=RobotStateRandomization(**rand))
    name = {"servos": "Upkie-HIP-Servos", "gyropod": "Upkie-HIP-Gyropod", "pendulum": "Upkie-HIP-Pendulum"}[kind]
    return envs.make(name, frequency=200.0, init_state=init, sim_factory=oracle_sim_factory)


@pytest.mark.parametrize("kind", ["pendulum", "gyropod"])
def test_reference_wrappers_on_hip_backend_equal_the_fused_envs(kind):
    mine = fused_env(kind)
    episodes = GOLDEN["wrappers"][kind]
    assert [e["seed"] for e in episodes] == [3, 11]
    for episode in episodes:
        obs_m, info_m = mine.reset(seed=episode["seed"])
        np.testing.assert_allclose(obs_m, episode["reset_observation"], atol=2e-6)
        assert set(info_m["spine_observation"]) >= {"base_orientation", "floor_contact", "imu", "servo", "wheel_odometry"}
        assert set(episode["spine_observation_keys"]) == set(info_m["spine_observation"])
        assert len(episode["steps"]) == 120
        for step, rec in enumerate(episode["steps"]):
            obs_m, rew_m, term_m, trunc_m, info_m = mine.step(np.array(rec["action"], dtype=np.float32))
            # (the reference hands float32 observations to the agent: compare there)
            np.testing.assert_allclose(obs_m, rec["observation"], atol=5e-6, err_msg=f"step {step}")
            assert rew_m == rec["reward"] == 0.0 and term_m == rec["terminated"] and trunc_m == rec["truncated"]
            sm = info_m["spine_observation"]["servo"]
            assert len(rec["servo"]) == 6
            for joint, values in rec["servo"].items():
                for key, want in zip(SERVO_KEYS, values):
                    assert sm[joint][key] == pytest.approx(want, abs=2e-5), (step, joint, key)
    mine.close()


def test_reference_servos_on_hip_backend_equal_the_fused_env():
    """Dictionary actions through the reference's UpkieServos (clamps, neutral
    action, missing keys) onto HipBackend.step, against this repository's
    UpkieServos, and the observation dictionaries they return."""
    mine = fused_env("servos")
    recorded = GOLDEN["servos"]
    mine.reset(seed=recorded["seed"])
    assert len(recorded["steps"]) == 60
    for step, rec in enumerate(recorded["steps"]):
        obs_m, _, term_m, _, _ = mine.step(rec["action"])
        assert term_m == rec["terminated"]
        assert len(rec["observation"]) == 6
        for joint, values in rec["observation"].items():
            for key, want in values.items():
                assert float(np.asarray(obs_m[joint][key]).reshape(-1)[0]) == pytest.approx(want, abs=2e-5), (step, joint, key)
    mine.close()


def assert_close(got, want, path=""):
    """Observation dictionaries equal up to float32 rounding."""
    if isinstance(want, dict):
        assert isinstance(got, dict) and set(got) == set(want), path
        for key in want:
            assert_close(got[key], want[key], f"{path}/{key}")
    elif isinstance(want, list):
        assert isinstance(got, list) and len(got) == len(want), path
        for i, (g, w) in enumerate(zip(got, want)):
            assert_close(g, w, f"{path}[{i}]")
    elif isinstance(want, float) and not isinstance(got, bool):
        assert got == pytest.approx(want, rel=1e-6, abs=2e-5), path
    else:
        assert got == want, path


def test_reference_spine_backend_drives_hip_spine():
    """The reference's SpineBackend / SpineInterface (shared memory, msgpack
    dictionaries, the request word protocol of spine_interface.py:66-169) as the
    agent side of a `HipSpine` running in its own process and serving env #1 of
    a batch: start with the reference's own spine configuration and reset state,
    act, stop; the reference's UpkieServos on that backend balances the robot."""
    import subprocess

    from upkie_amd.spine import Request, SpineInterface

    traffic = GOLDEN["spine"]["traffic"]
    assert [x["request"] for x in traffic] == [Request.kStop, Request.kStart] + [Request.kAction] * 60 + [Request.kStop] * 2
    name = f"/upkie_ref_{os.getpid()}_{uuid.uuid4().hex[:8]}"
    server = subprocess.Popen([sys.executable, "-m", "tests.spine_server", name], cwd=ROOT, stdout=subprocess.PIPE, text=True)
    responses = []
    try:
        assert server.stdout.readline().strip() == "ready"
        # the spine is another process of a possibly busy host: more patience than the reference's 100 ms per request
        agent = SpineInterface(name, timeout_ns=10_000_000_000)
        for exchange in traffic:
            agent._wait_for_spine()
            if "payload" in exchange:  # the reference's bytes, verbatim
                data = base64.b64decode(exchange["payload"])
                agent._buf[4:8] = len(data).to_bytes(4, sys.byteorder)
                agent._buf[8 : 8 + len(data)] = data
            agent._write_request(exchange["request"])
            if "response" in exchange:
                agent._wait_for_spine()
                responses.append(agent._read_dict())
                assert_close(responses[-1], exchange["response"], f"request {len(responses)}")
        agent.close()
    finally:
        server.terminate()
        tail = server.communicate(timeout=30)[0]
    start, last = responses[0], responses[-1]
    assert set(start) >= {"servo", "imu", "base_orientation", "floor_contact", "wheel_odometry", "time"}
    assert start["time"] == 0.0
    assert start["servo"]["left_hip"]["position"] == pytest.approx(0.1, abs=2e-3) and start["servo"]["right_knee"]["position"] == pytest.approx(-0.2, abs=2e-3)
    assert last["time"] == pytest.approx(60 * 0.005)
    assert abs(last["base_orientation"]["pitch"]) < 0.2 and last["floor_contact"]["contact"] is True
    assert last["servo"]["left_hip"]["position"] == pytest.approx(0.1, abs=0.05)
    over = tail.strip().splitlines()[-1].split()
    assert over[0] == "over"  # the spine left its loop in order (State.kOver) ...
    # ... env #0 was stepped alongside from its own reset state (a passive robot tipping over near x = 0), env #1 from x = 0.1
    assert abs(float(over[1])) < 0.05 and float(over[2]) == pytest.approx(0.1, abs=0.3) and abs(float(over[2]) - float(over[1])) > 0.02
    assert [float(over[1]), float(over[2])] == pytest.approx(GOLDEN["spine"]["server_over"], abs=1e-5)
    assert not os.path.exists(f"/dev/shm{name}")  # unlinked by the spine (AgentInterface.cpp:81-83)
