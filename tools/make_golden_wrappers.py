"""What the reference's OWN env wrappers and spine agent did in the scenarios of tests/test_reference_interop.py.

* `UpkiePendulum` / `UpkieGyropod` / `UpkieServos` imported unmodified from the reference (gymnasium /
  loop_rate_limiters / upkie_description stubbed as in tools/make_golden_envs.py) running on `HipBackend` over the
  fp64 CPU double of the simulation handle: per reset and step, the action the scripted agent chose, the observation,
  reward, termination and the spine observation's servo dictionary the reference returned.
* the reference's `SpineBackend` / `SpineInterface` as the agent of a `HipSpine` (tests/spine_server.py) over shared
  memory: every request it wrote, with the msgpack payload bytes it packed, and every observation dictionary it read
  back.

The test replays the recorded actions into this repository's envs and the recorded wire traffic into a `HipSpine`,
and compares what comes back with what the reference saw, wherever the suite runs.

Output: tests/golden/reference_wrappers.json.gz (committed). Build container only (needs the reference's sources):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_wrappers.py
"""

import base64
import gzip
import importlib.util
import json
import os
import subprocess
import sys
import uuid

import numpy as np

sys.dont_write_bytecode = True  # never write into the reference tree
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "reference_wrappers.json.gz")
RAND = dict(pitch=0.1, x=0.05, omega_y=0.1, linear_velocity=np.array([0.05, 0.0, 0.0]))
SERVO_KEYS = ("position", "velocity", "torque")


def install_reference():
    spec = importlib.util.spec_from_file_location("make_golden_envs", os.path.join(ROOT, "tools", "make_golden_envs.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    tool.install_stubs()


def floats(x):
    return [float(v) for v in np.asarray(x, dtype=np.float64).reshape(-1)]


def reference_env(kind):
    import upkie.envs.upkie_gyropod as ref_gyropod
    import upkie.envs.upkie_pendulum as ref_pendulum
    import upkie.envs.upkie_servos as ref_servos
    import upkie.utils.robot_state as ref_state
    import upkie.utils.robot_state_randomization as ref_rand

    from tests.fake_sim import oracle_sim_factory
    from upkie_amd.envs.backends import HipBackend

    init = ref_state.RobotState(position_base_in_world=np.array([0.0, 0.0, 0.6]), randomization=ref_rand.RobotStateRandomization(**RAND))
    backend = HipBackend(dt=1.0 / 200.0, sim_factory=oracle_sim_factory, device="cpu")
    servos = ref_servos.UpkieServos(backend=backend, frequency=200.0, frequency_checks=False, init_state=init, regulate_frequency=False)
    if kind == "servos":
        return servos
    return ref_gyropod.UpkieGyropod(servos) if kind == "gyropod" else ref_pendulum.UpkiePendulum(servos)  # (UpkiePendulum wraps its own UpkieGyropod)


def record_wrapper(kind):
    """The scripted agents of test_reference_wrappers_on_hip_backend_equal_the_fused_envs: 120 steps after each of two seeded resets."""
    env = reference_env(kind)
    episodes = []
    for seed in (3, 11):
        obs, info = env.reset(seed=seed)
        episode = {"seed": seed, "reset_observation": floats(obs), "spine_observation_keys": sorted(info["spine_observation"]), "steps": []}
        rng = np.random.default_rng(seed)
        for _ in range(120):
            if kind == "pendulum":
                pitch, pos, _, vel = obs
                action = np.array([np.clip(10.0 * pitch + pos + 0.1 * vel, -0.9, 0.9)], dtype=np.float32)
            else:
                action = np.array([np.clip(10.0 * obs[1] + obs[0], -0.9, 0.9), rng.uniform(-0.5, 0.5)], dtype=np.float32)
            obs, reward, terminated, truncated, info = env.step(action)
            servo = info["spine_observation"]["servo"]
            episode["steps"].append({"action": floats(action), "observation": floats(obs), "reward": float(reward), "terminated": bool(terminated),
                                     "truncated": bool(truncated), "servo": {j: [float(servo[j][k]) for k in SERVO_KEYS] for j in sorted(servo)}})
        episodes.append(episode)
    env.close()
    return episodes


def record_servos():
    """The dictionary actions of test_reference_servos_on_hip_backend_equal_the_fused_env (clamps, neutral action, missing keys)."""
    env = reference_env("servos")
    env.reset(seed=5)
    rng = np.random.default_rng(5)
    steps = []
    for _ in range(60):
        action = env.get_neutral_action()
        for joint in action:
            if "wheel" in joint:
                action[joint]["velocity"] = float(rng.uniform(-3, 3))
                action[joint]["kd_scale"] = float(rng.uniform(0.0, 7.0))  # beyond max_gain_scale: clamped
            else:
                action[joint]["position"] = float(rng.uniform(-0.3, 0.3))
                action[joint]["kp_scale"] = float(rng.uniform(0.0, 2.0))
                action[joint]["maximum_torque"] = float(rng.uniform(0.0, 20.0))  # beyond the effort limit: clamped
        obs, _, terminated, _, _ = env.step(action)
        steps.append({"action": {j: {k: float(v) for k, v in a.items()} for j, a in action.items()}, "terminated": bool(terminated),
                      "observation": {j: {k: float(np.asarray(v).reshape(-1)[0]) for k, v in o.items()} for j, o in obs.items()}})
    env.close()
    return {"seed": 5, "steps": steps}


def record_spine():
    """The reference's UpkieServos on its SpineBackend balancing env #1 of a HipSpine's batch for 60 steps, then stopping."""
    import upkie.envs.backends.spine.spine_interface as ref_interface
    import upkie.envs.backends.spine_backend as ref_spine_backend
    import upkie.envs.upkie_servos as ref_servos
    import upkie.utils.robot_state as ref_state

    traffic = []
    write_dict, write_request, read_dict = (ref_interface.SpineInterface._write_dict, ref_interface.SpineInterface._write_request,
                                            ref_interface.SpineInterface._read_dict)

    def recording_write_dict(self, dictionary):
        traffic.append({"payload": base64.b64encode(self._packer.pack(dictionary)).decode()})
        return write_dict(self, dictionary)

    def recording_write_request(self, request):
        if int(request) != 0:  # (kNone is written back after a kError only)
            if not traffic or "request" in traffic[-1]:
                traffic.append({})
            traffic[-1]["request"] = int(request)
        return write_request(self, request)

    def recording_read_dict(self):
        out = read_dict(self)
        traffic[-1]["response"] = out
        return out

    ref_interface.SpineInterface._write_dict, ref_interface.SpineInterface._write_request = recording_write_dict, recording_write_request
    ref_interface.SpineInterface._read_dict = recording_read_dict
    name = f"/upkie_golden_{os.getpid()}_{uuid.uuid4().hex[:8]}"
    server = subprocess.Popen([sys.executable, "-m", "tests.spine_server", name], cwd=ROOT, stdout=subprocess.PIPE, text=True)
    try:
        assert server.stdout.readline().strip() == "ready"
        backend = ref_spine_backend.SpineBackend(shm_name=name)
        init = ref_state.RobotState(position_base_in_world=np.array([0.1, 0.0, 0.58]), joint_configuration=np.array([0.1, -0.2, 0.0, 0.1, -0.2, 0.0]))
        servos = ref_servos.UpkieServos(backend=backend, frequency=200.0, frequency_checks=False, init_state=init, regulate_frequency=False)
        _, info = servos.reset(seed=1)
        for _ in range(60):
            so = info["spine_observation"]
            ground_velocity = 10.0 * so["base_orientation"]["pitch"] + so["wheel_odometry"]["position"] + 0.1 * so["wheel_odometry"]["velocity"]
            action = servos.get_neutral_action()
            for joint, target in (("left_hip", 0.1), ("left_knee", -0.2), ("right_hip", 0.1), ("right_knee", -0.2)):
                action[joint]["position"] = target
            action["left_wheel"]["velocity"] = ground_velocity / 0.05
            action["right_wheel"]["velocity"] = -ground_velocity / 0.05
            _, _, terminated, truncated, info = servos.step(action)
            assert not terminated and not truncated
        servos.close()
    finally:
        server.terminate()
        tail = server.communicate(timeout=30)[0]
    over = tail.strip().splitlines()[-1].split()
    assert over[0] == "over"
    return {"traffic": traffic, "server_over": [float(over[1]), float(over[2])]}


def compact(obj):
    """What the wrappers returned to 9 significant digits (every float32 value exactly; the tests compare at 2e-6 and
    beyond); the actions the agents chose stay exact."""
    if isinstance(obj, float):
        return float(f"{obj:.9g}")
    if isinstance(obj, dict):
        return {k: v if k == "action" else compact(v) for k, v in obj.items()}
    if isinstance(obj, list):
        return [compact(v) for v in obj]
    return obj


def main() -> None:
    install_reference()
    golden = {
        "source": "tools/make_golden_wrappers.py: the reference's UpkiePendulum / UpkieGyropod / UpkieServos on HipBackend over the fp64 CPU double, "
                  "and its SpineBackend driving tests/spine_server.py, unmodified",
        "wrappers": {kind: record_wrapper(kind) for kind in ("pendulum", "gyropod")},
        "servos": record_servos(),
        "spine": record_spine(),
    }
    with open(OUT, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0) as f:  # (mtime 0: the same bytes for the same content)
        f.write(json.dumps(compact(golden), separators=(",", ":")).encode())
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
