"""Left/right symmetry in the PPO update: ppo_learn_targets.py's goal-conditioned Gyropod task -- every env is asked for a
ground velocity and a yaw velocity while it balances -- trained with `upkie_amd.symmetry.MirrorSymmetry.gyropod(targets)`,
as rsl_rl's ``symmetry_cfg`` does it. Upkie is mirror-symmetric: under the mirror yaw, yaw velocity, the yaw command and the
yaw-velocity target change sign and everything else stays, so how the policy turns left is how it turns right, mirrored.
The update uses that twice: every stored sample is joined by its mirrored partner (``augment``: the minibatch's loss runs
over twice the samples, through the same towers, in the same launches), and ``mirror_coef`` times the mirror loss pulls
the mean on the mirrored observation to the mirrored mean. The rollout does not change. Every record carries
``train/mirror_loss``; ``approx_kl`` (and with it ``target_kl``) is that of the stored samples alone. The observations are
normalised, so the mirror acts on normalised rows: a flipped word's running mean is slightly off zero, and so is its mirror.
EXAMPLE_ENVS shortens the batch, EXAMPLE_STEPS the rollout and EXAMPLE_ITERATIONS the run (smoke tests)."""
import os

import torch
import torch.nn as nn

from _common import steps

import upkie_amd.envs as envs
from upkie_amd.policies import MlpActorCritic
from upkie_amd.ppo import Ppo
from upkie_amd.rewards import RewardTerms
from upkie_amd.symmetry import MirrorSymmetry
from upkie_amd.targets import TaskTargets
from upkie_amd.utils.robot_state import RobotState
from upkie_amd.utils.robot_state_randomization import RobotStateRandomization

from ppo_learn_targets import DT, NAMES, D, G, terms, tower

if __name__ == "__main__":
    B, T, iterations = int(os.environ.get("EXAMPLE_ENVS", 4096)), steps(128), int(os.environ.get("EXAMPLE_ITERATIONS", 10))
    torch.manual_seed(0)
    init = RobotState(randomization=RobotStateRandomization(pitch=0.1))
    with envs.make("Upkie-HIP-Gyropod-Vec", num_envs=B, seed=0, frequency=200.0, init_state=init, autoreset_mode="same_step",
                   max_episode_steps=400) as env:
        dev = env.device
        targets = TaskTargets(env, names=NAMES, ranges=[(-1.0, 1.0), (-1.0, 1.0)], resample_steps=(200, 600), stand_prob=0.1, deadband=[0.05, 0.05])
        reward = RewardTerms(B, D + G, 2, dt=DT, terms=terms(), device=dev)
        symmetry = MirrorSymmetry.gyropod(targets, augment=True, mirror_coef=0.5)
        actor, critic = tower(D + G, 2).to(dev), tower(D + G, 1).to(dev)
        policy = MlpActorCritic.from_modules(actor, critic, nn.Parameter(torch.zeros(2, device=dev)), action_low=[-2.0, -1.0], action_high=[2.0, 1.0])
        model = Ppo(env, policy, n_steps=T, batch_size=B * T // 4, learning_rate=lambda p: 3e-4 * p, target_kl=0.03, reward=reward, targets=targets,
                    symmetry=symmetry)
        model.learn(iterations * T * B)
        for record in model.records:
            print(f"iteration {record['time/iterations']}: train/mirror_loss {record['train/mirror_loss']:.4g}, "
                  + ", ".join(f"{k} {v:.4g}" if isinstance(v, float) else f"{k} {v}" for k, v in record.items() if k != "train/mirror_loss"))
