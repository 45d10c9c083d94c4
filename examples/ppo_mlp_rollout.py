"""A PPO iteration with an MLP actor-critic on the device: 128 steps of 4096 Pendulum envs collected with the policy
as ONE launch per step (`upkie_amd.policies.MlpActorCritic`: both towers, the Gaussian draw, its log-probability and
the clamp, written straight into the rollout buffer), advantages by the GAE kernel, then one PPO update of the same
torch modules with plain autograd and `update_from` to re-pack the new weights on the device."""
import torch
import torch.nn as nn

from _common import steps

import upkie_amd.envs as envs
from upkie_amd.policies import MlpActorCritic
from upkie_amd.rollout import RolloutBuffer
from upkie_amd.utils.robot_state import RobotState
from upkie_amd.utils.robot_state_randomization import RobotStateRandomization


def tower(d_in, d_out):  # SB3 MlpPolicy's default net_arch: [64, 64], tanh
    return nn.Sequential(nn.Linear(d_in, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, d_out))


if __name__ == "__main__":
    B, T = 4096, steps(128)
    torch.manual_seed(0)
    init = RobotState(randomization=RobotStateRandomization(pitch=0.1))
    with envs.make("Upkie-HIP-Pendulum-Vec", num_envs=B, frequency=200.0, init_state=init, autoreset_mode="same_step",
                   max_episode_steps=400) as env:
        dev = env.device
        actor, critic = tower(4, 1).to(dev), tower(4, 1).to(dev)
        log_std = nn.Parameter(torch.zeros(1, device=dev))
        policy = MlpActorCritic.from_modules(actor, critic, log_std, action_low=[-1.0], action_high=[1.0], seed=0)
        buffer = RolloutBuffer(T, B, obs_shape=(4,), action_shape=(1,), device=dev)
        obs, _ = env.reset(seed=0)
        starts = torch.ones(B, dtype=torch.uint8, device=dev)
        for t in range(T):
            # obs, action, value and log_prob land in the buffer's slot t; env_action is the clamped action
            out = policy.act(obs, out={"norm_obs": buffer.observations[t], "action": buffer.actions[t], "value": buffer.values[t],
                                       "log_prob": buffer.log_probs[t]})
            next_obs, reward, terminated, truncated, info = env.step(out[0])
            reward = 1.0 - next_obs[:, 0].abs()  # stand-in reward (the reference's is constant, upkie_env.py:230)
            buffer.add_policy_step(None, reward, starts, out)
            starts = (terminated | truncated).to(torch.uint8)
            obs = next_obs
        buffer.compute_returns_and_advantage(last_values=policy.value(obs), dones=starts)

        # one PPO epoch in torch (clipped surrogate + value loss), on the modules the policy was packed from
        opt = torch.optim.Adam(list(actor.parameters()) + list(critic.parameters()) + [log_std], lr=3e-4)
        for batch in buffer.get(batch_size=B * T // 4, generator=torch.Generator(device=dev).manual_seed(0)):
            adv = (batch["advantages"] - batch["advantages"].mean()) / (batch["advantages"].std() + 1e-8)
            dist = torch.distributions.Normal(actor(batch["observations"]), log_std.exp())
            ratio = torch.exp(dist.log_prob(batch["actions"]).sum(-1) - batch["old_log_prob"])
            policy_loss = -torch.min(adv * ratio, adv * ratio.clamp(0.8, 1.2)).mean()
            value_loss = (critic(batch["observations"])[:, 0] - batch["returns"]).pow(2).mean()
            opt.zero_grad()
            (policy_loss + 0.5 * value_loss).backward()
            opt.step()
        policy.update_from()  # re-pack the updated weights on the device
        value_after = policy.value(obs).mean()
        print(f"ppo_mlp_rollout: {T} x {B} steps, mean advantage {float(buffer.advantages.mean()):+.4f}, mean return "
              f"{float(buffer.returns.mean()):+.3f}, policy loss {float(policy_loss):+.4f}, value loss {float(value_loss):.4f}, "
              f"mean value of the last observations after the update {float(value_after):+.4f}")
