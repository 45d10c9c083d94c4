"""The PPO iteration of ppo_mlp_rollout.py with Stable-Baselines3's VecNormalize in training mode on the device
(`upkie_amd.normalize.RunningNormalizer`): after every env step the running observation and return statistics are
updated, the normalised reward and the episode starts are written into the rollout buffer, and the policy, attached to
the normalizer, normalises its next observations with the live statistics. The whole rollout step -- policy, env step,
normalizer -- is captured once with `GraphedLoop` and the 128 steps replay as one graph launch."""
import torch
import torch.nn as nn

from _common import steps

import upkie_amd.envs as envs
from upkie_amd.graphs import GraphedLoop
from upkie_amd.normalize import RunningNormalizer
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
        normalizer = RunningNormalizer.for_env(env, gamma=0.99)  # SB3's defaults: norm_obs, norm_reward, clip 10
        normalizer.attach(policy)  # (before the policy's first call)
        buffer = RolloutBuffer(T, B, obs_shape=(4,), action_shape=(1,), device=dev)
        env.reset(seed=0)
        obs = env.observation  # the env's persistent observation buffer, rewritten by every step
        normalizer.reset(obs)
        env_action = torch.empty(B, 1, device=dev)
        stand_in = torch.empty(B, device=dev)
        starts = torch.ones(B, dtype=torch.uint8, device=dev)
        slot = {"t": T - 1}  # (the warm-up step of the capture writes the last slot, replayed over; the capture records 0 .. T-1)

        def rollout_step():
            t = slot["t"]
            buffer.episode_starts[t].copy_(starts)
            # normalised obs, action, value and log_prob land in the buffer's slot t; env_action is the clamped action
            out = policy.act(obs, out={"norm_obs": buffer.observations[t], "action": buffer.actions[t], "value": buffer.values[t],
                                       "log_prob": buffer.log_probs[t], "env_action": env_action})
            next_obs, _, terminated, truncated, _ = env.step(out[0])
            torch.abs(next_obs[:, 0], out=stand_in).neg_().add_(1.0)  # stand-in reward (the reference's is constant, upkie_env.py:230)
            normalizer.step(next_obs, stand_in, terminated, truncated, out={"reward": buffer.rewards[t], "episode_starts": starts})
            slot["t"] = (t + 1) % T

        loop = GraphedLoop(rollout_step, unroll=T, warmup=1)
        loop.replay()  # T steps
        buffer.pos, buffer.full = T, True
        buffer.compute_returns_and_advantage(last_values=policy.value(obs), dones=starts)

        # one PPO epoch in torch (clipped surrogate + value loss) on the normalised observations the buffer holds
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
        policy.update_from()  # re-pack the updated weights; the live statistics stay (the normalizer's mirrors are its sources)
        print(f"ppo_mlp_normalized_rollout: {T} x {B} steps (one graph launch), obs mean {normalizer.obs_mean.cpu().numpy().round(4)}, "
              f"obs var {normalizer.obs_var.cpu().numpy().round(6)}, return var {float(normalizer.ret_var):.4f}, mean normalised reward "
              f"{float(buffer.rewards.mean()):+.4f}, mean advantage {float(buffer.advantages.mean()):+.4f}, policy loss "
              f"{float(policy_loss):+.4f}, value loss {float(value_loss):.4f}")
