"""Data-parallel PPO over the GPUs of a node: every rank steps its own shard of Upkie-Pendulum envs
(`upkie_amd.distributed.ShardedVecEnv`), runs a replica of the policy, keeps a `RunningNormalizer` and a `PpoTrainer`
that take the process group, and computes GAE on its own rollout. The normaliser's statistics and every minibatch's
gradient are exchanged between the ranks, so the replicas train as ONE learner on the union of the samples and hold
the same weights, bit for bit, after every minibatch.

    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 examples/ppo_mlp_train_sharded.py

EXAMPLE_BACKEND=gloo runs the exchanges through the host (several ranks may then share one GPU, as the tests do)."""
import os

import torch
import torch.distributed as dist
import torch.nn as nn

from _common import steps

from upkie_amd import abi
from upkie_amd.distributed import ShardedVecEnv, init_distributed
from upkie_amd.normalize import RunningNormalizer
from upkie_amd.policies import MlpActorCritic
from upkie_amd.ppo import STAT_NAMES, PpoTrainer
from upkie_amd.rollout import RolloutBuffer


def tower(d_in, d_out):  # SB3 MlpPolicy's default net_arch: [64, 64], tanh
    return nn.Sequential(nn.Linear(d_in, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, d_out))


if __name__ == "__main__":
    backend = os.environ.get("EXAMPLE_BACKEND")
    os.environ.setdefault("UPKIE_FORCE_PROCESS_GROUP", "1")  # (one rank still trains through the group: the same bits)
    rank, world, local_rank = init_distributed(backend=backend)
    group = dist.group.WORLD
    gloo = dist.get_backend(group) == "gloo"
    local_rank %= torch.cuda.device_count()
    torch.cuda.set_device(local_rank)
    dev = f"cuda:{local_rank}"
    B, T, iterations = 4096, steps(128), 3  # envs per rank
    cfg = abi.default_sim_config(B, frequency=200.0, seed=0)
    cfg.rand_pitch = 0.1
    cfg.autoreset_mode = abi.AUTORESET_NEXT_STEP
    cfg.env_id_offset = rank * B  # random streams are keyed by the global env id
    # The shard's per-step outputs travel to rank 0's rollout ring through RCCL; the learner here does not read them.
    # Over gloo (ranks sharing a GPU) each shard keeps its ring to itself.
    env = ShardedVecEnv("pendulum", cfg, dev, rank=0 if gloo else rank, world_size=1 if gloo else world, chunk=32, horizon=128)
    torch.manual_seed(0)  # (the same initial weights everywhere; broadcast_parameters makes sure of it)
    actor, critic = tower(4, 1).to(dev), tower(4, 1).to(dev)
    log_std = nn.Parameter(torch.zeros(1, device=dev))
    # the policy's noise is keyed by the LOCAL env index and the seed: a seed per rank, or every replica draws the same noise
    policy = MlpActorCritic.from_modules(actor, critic, log_std, action_low=[-1.0], action_high=[1.0], seed=rank)
    normalizer = RunningNormalizer.for_env(env, gamma=0.99, process_group=group)
    normalizer.attach(policy)
    trainer = PpoTrainer(policy, n_epochs=10, batch_size=B * T // 4, obs_normalized=True, seed=0, process_group=group)
    trainer.broadcast_parameters(0)
    normalizer.broadcast_statistics(0)
    buffer = RolloutBuffer(T, B, obs_shape=(4,), action_shape=(1,), device=dev)
    obs = env.reset()
    normalizer.reset(obs)
    env_action = torch.empty(B, 1, device=dev)
    starts = torch.ones(B, dtype=torch.uint8, device=dev)
    for it in range(iterations):
        for t in range(T):
            buffer.episode_starts[t].copy_(starts)
            policy.act(obs, out={"norm_obs": buffer.observations[t], "action": buffer.actions[t], "value": buffer.values[t],
                                 "log_prob": buffer.log_probs[t], "env_action": env_action})
            obs, reward, terminated, truncated = env.step(env_action)
            normalizer.step(obs, reward, terminated, truncated, out={"reward": buffer.rewards[t], "episode_starts": starts})
        buffer.pos, buffer.full = T, True
        buffer.compute_returns_and_advantage(last_values=policy.value(obs), dones=starts)
        stats = trainer.train(buffer)  # [10, 4, 7] on the device, the same on every rank
        last = stats[-1].mean(dim=0).cpu().numpy()
        if rank == 0:
            print(f"iteration {it}: mean normalised reward (rank 0) {float(buffer.rewards.mean()):+.4f}, "
                  + ", ".join(f"{name} {value:+.4g}" for name, value in zip(STAT_NAMES, last)), flush=True)
    packed = policy.packed.cpu() if gloo else policy.packed
    rows = [torch.empty_like(packed) for _ in range(world)]
    dist.all_gather(rows, packed, group=group)
    equal = all(torch.equal(r, rows[0]) for r in rows)
    if rank == 0:
        print(f"ppo_mlp_train_sharded: {world} rank(s) x {B} envs, {iterations} iterations of {T} steps + {trainer.n_epochs} x "
              f"{trainer.n_minibatches} minibatch updates; weights equal on all ranks: {equal}", flush=True)
    env.shutdown(destroy_group=False)
    dist.destroy_process_group()
    if not equal:
        raise SystemExit("the replicas' weights differ")
