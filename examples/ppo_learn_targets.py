"""A goal-conditioned policy: a Gyropod env whose policy is asked for a ground velocity and a yaw velocity while it
balances (`upkie_amd.targets.TaskTargets`: one more launch per env step, inside the captured rollout). Every env holds a
target of its own for 1 to 3 s, then draws another; one draw in ten asks it to stand still; an episode's end draws again.
The targets are the last two words of the observation, so the reward's tracking terms are plain taps --
``exp(-((v - v*) / s)^2)`` on ``obs(3)`` against ``obs(6)`` and on ``obs(5)`` against ``obs(7)`` -- next to an alive bonus
and a fall penalty. A `TargetCurriculum` starts at +-0.3 m/s (and rad/s) and widens both ranges by 0.1 whenever the
episodes that just finished tracked the ground velocity well, up to +-1.5 m/s; the ranges are device words, so the
captured rollout follows them without a re-capture, and every record carries them (``rollout/target_<name>_low`` /
``_high``). An `EvalCallback` evaluates at the FINAL ranges, in an env and with targets of its own.
EXAMPLE_ENVS shortens the batch, EXAMPLE_STEPS the rollout and EXAMPLE_ITERATIONS the run (smoke tests)."""
import os

import torch
import torch.nn as nn

from _common import steps

import upkie_amd.envs as envs
from upkie_amd.evaluation import EvalCallback
from upkie_amd.policies import MlpActorCritic
from upkie_amd.ppo import Ppo
from upkie_amd.rewards import RewardTerms, Term, obs, one, terminated
from upkie_amd.targets import TargetCurriculum, TaskTargets
from upkie_amd.utils.robot_state import RobotState
from upkie_amd.utils.robot_state_randomization import RobotStateRandomization

D, G, DT = 6, 2, 1.0 / 200.0  # the Gyropod observation [position, pitch, yaw, ground velocity, pitch rate, yaw velocity]; two targets
NAMES = ("ground_velocity", "yaw_velocity")
LIMIT = [(-1.5, 1.5), (-1.0, 1.0)]


def tower(d_in, d_out):  # SB3 MlpPolicy's default net_arch: [64, 64], tanh
    return nn.Sequential(nn.Linear(d_in, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, d_out))


def terms():  # on the row the targets stage writes: the env's six words, then the two targets
    return {
        "alive": Term(0.5, taps=[one()]),
        "track_ground_velocity": Term(1.0, "exp_square", 0.25, [obs(3), obs(D + 0, -1.0)]),
        "track_yaw_velocity": Term(0.5, "exp_square", 0.25, [obs(5), obs(D + 1, -1.0)]),
        "fall": Term(-10.0, taps=[terminated()]),
    }


if __name__ == "__main__":
    B, T, iterations = int(os.environ.get("EXAMPLE_ENVS", 4096)), steps(128), int(os.environ.get("EXAMPLE_ITERATIONS", 10))
    limit_steps = 400
    torch.manual_seed(0)
    init = RobotState(randomization=RobotStateRandomization(pitch=0.1))
    kw = dict(frequency=200.0, init_state=init, autoreset_mode="same_step", max_episode_steps=limit_steps)
    make = lambda n, seed: envs.make("Upkie-HIP-Gyropod-Vec", num_envs=n, seed=seed, **kw)  # noqa: E731
    with make(B, 0) as env, make(min(B, 256), 1) as eval_env:
        dev, E = env.device, int(eval_env.num_envs)
        # (an episode that tracked perfectly sums to `limit_steps`: widen when the finished episodes reach 60 % of that)
        curriculum = TargetCurriculum("track_ground_velocity", 0.6 * limit_steps, step=[0.1, 0.1], limit=LIMIT)
        targets = TaskTargets(env, names=NAMES, ranges=[(-0.3, 0.3), (-0.3, 0.3)], resample_steps=(200, 600), stand_prob=0.1,
                              deadband=[0.05, 0.05], curriculum=curriculum)
        reward = RewardTerms(B, D + G, 2, dt=DT, terms=terms(), device=dev)
        eval_targets = TaskTargets(eval_env, names=NAMES, ranges=LIMIT, resample_steps=(200, 600), stand_prob=0.1, deadband=[0.05, 0.05])
        eval_reward = RewardTerms(E, D + G, 2, dt=DT, terms=terms(), device=dev)
        callback = EvalCallback(eval_env, n_eval_episodes=E, eval_freq=2 * T, reward=eval_reward, targets=eval_targets, seed=1)
        actor, critic = tower(D + G, 2).to(dev), tower(D + G, 1).to(dev)
        policy = MlpActorCritic.from_modules(actor, critic, nn.Parameter(torch.zeros(2, device=dev)), action_low=[-2.0, -1.0], action_high=[2.0, 1.0])
        model = Ppo(env, policy, n_steps=T, batch_size=B * T // 4, learning_rate=lambda p: 3e-4 * p, target_kl=0.03, reward=reward, targets=targets)
        model.learn(iterations * T * B, callback=callback)
        for record in model.records:
            print(f"iteration {record['time/iterations']}: " + ", ".join(f"{k} {v:.4g}" if isinstance(v, float) else f"{k} {v}" for k, v in record.items()))
        print("training ranges: " + ", ".join(f"{name} [{lo:.2f}, {hi:.2f}]" for name, (lo, hi) in zip(NAMES, targets.limits.cpu().tolist())))
        if callback.last_mean_reward is not None:
            print(f"evaluated at the final ranges {LIMIT}: last mean reward {callback.last_mean_reward:.4g}")
