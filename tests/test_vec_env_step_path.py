"""One step path between `env.step()` and the handle: the CPU doubles of tests/fake_sim.py meet the handle contract
`upkie_amd.sim` states, so the wrappers run on them the code they run on a `BatchedSim`. The checks of the cached
five-tuple are functions of how an env is made: tests/test_vec_env_step_path_gpu.py repeats them on the real handle."""

import inspect

import numpy as np
import pytest
import torch

import upkie_amd.envs as envs
from upkie_amd import abi
from upkie_amd.distributed import ShardedVecEnv
from upkie_amd.envs.vec_env import _SameStepInfo
from upkie_amd.exceptions import UpkieException
from upkie_amd.model.default_model import default_model
from upkie_amd.mpc import BALANCER_METHODS, BatchedMpc
from upkie_amd.sim import HANDLE_BUFFERS, HANDLE_METHODS, BatchedSim

from .fake_sim import OracleMpc, OracleObservers, OracleSim, oracle_sim_factory

DOUBLES = dict(sim_factory=oracle_sim_factory, observers_factory=OracleObservers)
FUSED_KINDS = {"pendulum": ("Upkie-HIP-Pendulum-Vec", (1,)), "gyropod": ("Upkie-HIP-Gyropod-Vec", (2,)), "servos": ("Upkie-HIP-Servos-Vec", (6, 6))}


def _parameters(cls, name):
    member = inspect.getattr_static(cls, name)
    if isinstance(member, property):
        return "property"
    return list(inspect.signature(member).parameters)


@pytest.mark.parametrize("product, double, names", [(BatchedSim, OracleSim, HANDLE_METHODS), (BatchedMpc, OracleMpc, BALANCER_METHODS)])
def test_doubles_define_the_contract_with_the_products_parameter_names(product, double, names):
    for name in names:
        assert _parameters(product, name) == _parameters(double, name), name


def test_double_holds_the_contracts_buffers():
    sim = OracleSim(abi.default_sim_config(2), default_model())
    for name in HANDLE_BUFFERS:
        assert hasattr(sim, name), name
    assert sim.obs_servos is None and sim.obs3 is None  # (allocated by the first method that needs them, like the handle's)


def test_base_velocity_env_and_sharded_env_step_through_one_composition():
    """`UpkieBaseVelocityVecEnv` and `ShardedVecEnv("base_velocity")` on the doubles run the same balancer + step
    composition (the double's): the same arrays, step by step, across a NEXT_STEP autoreset."""
    B = 4
    env = envs.make("Upkie-HIP-BaseVelocity-Vec", num_envs=B, frequency=200.0, nb_timesteps=16, seed=3, mpc_factory=OracleMpc, **DOUBLES)
    assert env.autoreset_mode == "next_step" and not env.fuse_mpc
    copy = lambda struct: type(struct).from_buffer_copy(struct)  # noqa: E731
    sharded = ShardedVecEnv("base_velocity", copy(env.config), device="cpu", model=env.model.struct, horizon=32, chunk=4,
                            sim_factory=oracle_sim_factory, mpc_config=copy(env.mpc_balancer.config), mpc_factory=OracleMpc)
    obs, _ = env.reset()
    assert np.array_equal(obs.numpy(), sharded.reset().numpy())
    actions = torch.from_numpy(np.random.default_rng(0).uniform(-0.5, 0.5, size=(30, B, 2)).astype(np.float32))
    flagged = torch.tensor([0.0, 0.0, 1.0, 0.0])
    for k in range(30):
        if k == 10:
            env.sim.flag_done(flagged)
            sharded.sim.flag_done(flagged)
        obs, _, terminated, truncated, _ = env.step(actions[k])
        obs_s, _, terminated_s, truncated_s = sharded.step(actions[k].clone())
        assert obs is env.sim.obs3
        assert np.array_equal(obs.numpy(), obs_s.numpy()), k
        assert np.array_equal(terminated.numpy(), terminated_s.numpy().astype(bool)), k
        assert np.array_equal(truncated.numpy(), truncated_s.numpy().astype(bool)), k
        if k == 10:  # the flagged env restarted at the origin, the others kept their pose
            assert obs[2, 0] == 0.0 and obs[2, 1] == 0.0 and bool((obs[[0, 1, 3], 0] != 0.0).all())
    assert env.sim.state[abi.S_EPISODE].tolist() == [1.0, 1.0, 2.0, 1.0]
    env.close()
    sharded.shutdown()


def check_cached_step_output(kind, num_envs, **how):
    """The cached five-tuple of a fused env kind made with `how` (`sim_factory=` ...), through `step` and the
    in-launch policies: reused while nothing has to happen per step, built anew otherwise."""
    env_id, act_shape = FUSED_KINDS[kind]
    action = torch.zeros((num_envs,) + act_shape)
    if kind == "servos":
        action[:, :, 3:5], action[:, :, 5], action[:, [2, 5], 0] = 1.0, 16.0, float("nan")

    def steps(env):
        yield lambda: env.step(action.to(env.device))
        if kind == "pendulum":
            yield env.step_linear_policy
        if kind == "servos":
            law = abi.velocity_balancing_policy(0.06, 0.15, 1.0)
            yield lambda: env.step_servo_policy(law)

    env = envs.make(env_id, num_envs=num_envs, frequency=200.0, **how)
    env.reset(seed=0)
    outs = [step() for step in steps(env) for _ in range(2)]
    assert all(out is outs[0] for out in outs) and len(outs[0]) == 5
    assert outs[0][0] is env.observation and type(outs[0][4]) is dict
    env.close()

    for per_step in (dict(eager_spine_observation=True), dict(spine_observers=True)):
        env = envs.make(env_id, num_envs=num_envs, frequency=200.0, **per_step, **how)
        env.reset(seed=0)
        for step in steps(env):
            first, second = step(), step()
            assert first is not second and first[0] is second[0] is env.observation
        assert env._step_out is None
        env.close()

    env = envs.make(env_id, num_envs=num_envs, frequency=200.0, autoreset_mode="same_step", **how)
    env.reset(seed=0)
    assert env._final_obs is None
    step = next(steps(env))
    first = step()
    assert env._final_obs is not None and env.sim.final_obs is env._final_obs  # armed by the first step
    second, third = step(), step()
    assert second is third and second[0] is env.observation
    info = second[4]
    assert type(info) is _SameStepInfo and info["final_obs"] is env._final_obs and first[4]["final_obs"] is env._final_obs
    assert torch.equal(info["_final_obs"], second[2] | second[3])
    for policy_step in list(steps(env))[1:]:
        with pytest.raises(UpkieException):
            policy_step()
    env.close()
    assert env._final_obs is None and env._step_out is None and env.sim.final_obs is None


@pytest.mark.parametrize("kind", sorted(FUSED_KINDS))
def test_cached_step_output_on_the_doubles(kind):
    check_cached_step_output(kind, 3, **DOUBLES)
