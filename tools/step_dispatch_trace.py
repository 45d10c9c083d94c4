"""Which kernels each step entry point launches, configuration by configuration: one line per configuration, the
configuration followed by the kernel names in dispatch order. Two builds of the library that choose the same step
kernels print the same lines (`UPKIE_HIP_LIBRARY` selects the build, as in tools/ab_step.py): the record of a change
to the host side of the dispatch (upkie_amd/csrc/step_dispatch.hpp), `profiles/step_dispatch_trace.txt`.

The calls run in a fresh child process under `rocprofv3 --kernel-trace` with a time limit of its own; every call sits
between two marker launches (a fill of an fp64 word: nothing else here launches one), the set-up of a configuration
(reset, randomisation) outside them. Grid: entry point x forced lanes per env x inertial records x in-step spine
observers | Bullet-like contact manifold x `set_final_observation` x default model | another wheel radius, at 64 envs;
Servos at 8193 envs and the one-lane Pendulum step at 131072 for the two batch thresholds.

usage: python tools/step_dispatch_trace.py [--timeout 600] [--keep DIR]"""
import argparse
import csv
import glob
import itertools
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ENTRY_POINTS = ("reset", "pendulum", "pendulum_packed", "pendulum_agent", "agent_rollout", "gyropod", "servos", "servos_policy",
                "base_velocity", "autoreset_done")
MARKER = "FillFunctor<double>"


def configurations():
    """(num_envs, default model, inertial records, spine observers, contact manifold, final observation, lanes, entry point):
    the handle's settings outermost, one handle serves the calls that share them."""
    for default_model, inertials, (spine, manifold), final_obs in itertools.product((True, False), (False, True),
                                                                                    ((False, False), (True, False), (False, True)), (False, True)):
        for lanes, entry in itertools.product((0, 1, 2, 8), ENTRY_POINTS):
            yield 64, default_model, inertials, spine, manifold, final_obs, lanes, entry
    for lanes, entry in itertools.product((0, 1, 2, 8), ("servos", "servos_policy")):
        yield 8193, True, False, False, False, False, lanes, entry
    yield 131072, True, False, False, False, False, 1, "pendulum"


def label(cfg):
    n, default_model, inertials, spine, manifold, final_obs, lanes, entry = cfg
    return (f"{entry} envs={n} lanes={lanes} inertials={int(inertials)} spine={int(spine)} manifold={int(manifold)} "
            f"final_obs={int(final_obs)} model={'default' if default_model else 'wheel_radius'}")


def child(out_dir):
    import torch

    import bench
    from upkie_amd import abi
    from upkie_amd.lib import UpkieHipError
    from upkie_amd.model.default_model import default_model
    from upkie_amd.mpc import BatchedMpc
    from upkie_amd.sim import BatchedSim

    dev = "cuda:0"
    mark = torch.empty(1, dtype=torch.float64, device=dev)  # (not zeros: that would be a marker launch)
    sim, mpc, key, results = None, None, None, []
    for cfg in configurations():
        n, default, inertials, spine, manifold, final_obs, lanes, entry = cfg
        if key != cfg[:6]:
            key = cfg[:6]
            model = default_model()
            if not default:
                model.wheel_radius *= 1.05
            sim = BatchedSim(bench.make_config(n), model)
            mpc = BatchedMpc(abi.default_mpc_config(n, 16))
            if inertials:
                sim.randomize_inertias(0.1)
            if spine:
                sim.attach_observers(abi.default_observer_config(n, 1e-3))
            if manifold:
                sim.use_bullet_like_contacts(True)
            final = torch.zeros(n * 30, device=dev)
            if final_obs:
                sim.set_final_observation(final)
            records, ring = torch.zeros(n, 8, device=dev), torch.zeros(4, n, 8, device=dev)
            act1, act2, act36 = torch.zeros(n, device=dev), torch.zeros(n, 2, device=dev), torch.zeros(n, 6, 6, device=dev)
            x0, contact = torch.zeros(n, 4, device=dev), torch.ones(n, dtype=torch.uint8, device=dev)
            policy = abi.velocity_balancing_policy(float(model.wheel_radius), 1.0, float(model.left_sign))
            sim.step_servos(act36)  # (allocates the Servos observation outside the windows)
        sim.set_lanes_per_env(lanes)
        sim.reset()
        mpc.reset()
        call = {
            "reset": sim.reset,
            "pendulum": lambda: sim.step_pendulum(act1),
            "pendulum_packed": lambda: sim.step_pendulum_packed(records, act1),
            "pendulum_agent": sim.step_pendulum_agent,
            "agent_rollout": lambda: sim.rollout_pendulum_records(records, ring),
            "gyropod": lambda: sim.step_gyropod(act2),
            "servos": lambda: sim.step_servos(act36),
            "servos_policy": lambda: sim.step_servos_policy(policy),
            "base_velocity": lambda: sim.step_base_velocity_mpc(mpc, act2, x0, contact),
            "autoreset_done": lambda: sim.autoreset_done(abi.OBSERVATION_PENDULUM, sim.obs4, final),
        }[entry]
        if entry == "base_velocity":
            sim.step_base_velocity_mpc(mpc, act2, x0, contact)  # (allocates its observation outside the window)
        mark.fill_(1.0)
        try:
            call()
            results.append("ok")
        except UpkieHipError as err:
            if err.status != -1:  # (UPKIE_ERR_INVALID_ARGUMENT: a refused call is part of the record; anything else ends the run)
                raise
            results.append("refused: " + str(err).splitlines()[0] + " ")
        mark.fill_(2.0)
        torch.cuda.synchronize()
    with open(os.path.join(out_dir, "results.txt"), "w") as f:
        f.write("\n".join(results) + "\n")


def windows(out_dir):
    """The kernel names between the marker pairs, in dispatch order."""
    paths = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not paths:
        sys.exit(f"step_dispatch_trace: no kernel trace under {out_dir}")
    rows = []
    for path in paths:
        with open(path) as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    found, current = [], None
    for r in rows:
        name = r["Kernel_Name"]
        if MARKER in name:
            if current is None:
                current = []
            else:
                found.append(current)
                current = None
        elif current is not None:
            current.append(name.split("(")[0].replace("void ", "").replace("upkie::", ""))
    return found


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--timeout", type=int, default=600, help="seconds the profiled child process may take")
    ap.add_argument("--keep", metavar="DIR", help="keep the trace under DIR")
    ap.add_argument("--child", metavar="DIR", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.child)
        sys.exit(0)
    out_dir = args.keep or tempfile.mkdtemp(prefix="step_dispatch_trace_")
    os.makedirs(out_dir, exist_ok=True)
    cmd = ["timeout", "-k", "10", str(args.timeout), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "-o", "trace",
           "--", sys.executable, os.path.abspath(__file__), "--child", out_dir]
    done = subprocess.run(cmd, capture_output=True, text=True)
    if done.returncode != 0:
        sys.exit(f"step_dispatch_trace: the profiled run ended with status {done.returncode}\n{done.stdout[-2000:]}\n{done.stderr[-2000:]}")
    with open(os.path.join(out_dir, "results.txt")) as f:
        results = f.read().splitlines()
    cfgs, found = list(configurations()), windows(out_dir)
    if not len(cfgs) == len(results) == len(found):
        sys.exit(f"step_dispatch_trace: {len(cfgs)} configurations, {len(results)} calls, {len(found)} marked windows in the trace")  # (the marker's name?)
    for cfg, result, names in zip(cfgs, results, found):
        print(f"{label(cfg)}: {result if result != 'ok' else ''}{' | '.join(names)}", flush=True)
