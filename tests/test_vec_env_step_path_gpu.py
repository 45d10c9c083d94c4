"""The env wrappers' one step path on a real `BatchedSim` (one MI355X): the cached five-tuple of the fused kinds and
both bodies of `UpkieBaseVelocityVecEnv.step`. Eight envs: the eight-lane mapping, on which `fuse_mpc` is on."""

import pytest
import torch

import upkie_amd.envs as envs

from .test_vec_env_step_path import FUSED_KINDS, check_cached_step_output

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", sorted(FUSED_KINDS))
def test_cached_step_output_on_the_handle(kind):
    check_cached_step_output(kind, 8)


@pytest.mark.parametrize("fuse_mpc", [True, False])
def test_base_velocity_steps_with_one_call_and_with_two(fuse_mpc):
    env = envs.make("Upkie-HIP-BaseVelocity-Vec", num_envs=8, frequency=200.0, nb_timesteps=16)
    assert env.sim.lanes_per_env == 8 and env.fuse_mpc
    env.fuse_mpc = fuse_mpc
    env.reset(seed=1)
    action = torch.tensor([[0.2, 0.1]], device=env.device).repeat(8, 1)
    for _ in range(20):
        obs = env.step(action)[0]
        assert obs is env.sim.obs3 and obs is env.observation
    assert obs.shape == (8, 3) and bool(torch.isfinite(obs).all())
    env.close()
