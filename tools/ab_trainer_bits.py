"""Bit-for-bit A/B of the trainer-side kernels between builds of the library on ONE box: a fixed list of small launches
-- the sampled MLP policy, the agent pipeline, VecNormalize, the episode statistics, the PPO update and its data-parallel
halves on a one-rank slot -- and a SHA-256 of every output buffer, each build in its own fresh process
(UPKIE_HIP_LIBRARY, as tools/ab_step.py). The shapes are the smallest that reach what csrc/random.hpp and
csrc/block_reduce.hpp serve: both Box-Muller pairs of two Philox blocks, ragged last tiles and blocks, a ticket drawn by one
block and by several (two consecutive steps: the second shows the ticket went back to 0), fewer than 32, exactly 32 and 33
gradient partials under the fold's 32-deep load batch. Exit status 1 when a digest differs or a child fails (no child is
started after a failed one).
Usage: python tools/ab_trainer_bits.py libA.so libB.so ... [--timeout SECONDS per build]"""
import ctypes
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child():
    sys.path.insert(0, ROOT)
    import torch
    import torch.nn as nn

    from upkie_amd.distributed import SlotExchange
    from upkie_amd.episodes import EpisodeStatistics
    from upkie_amd.normalize import RunningNormalizer
    from upkie_amd.pipeline import AgentPipeline
    from upkie_amd.policies import MlpActorCritic
    from upkie_amd.ppo import PpoTrainer
    from upkie_amd.rollout import RolloutBuffer

    dev = "cuda:0"
    gen = torch.Generator().manual_seed(1234)  # (host draws, then copied: the same inputs in every process)

    def randn(*shape, scale=1.0):
        return (scale * torch.randn(*shape, generator=gen)).to(dev)

    def digest(label, tensors):
        for name, t in tensors.items():
            if t is not None:
                print(f"{label}/{name} {hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()}", flush=True)

    def towers(widths, act_dim, activation):
        torch.manual_seed(7)

        def tower(d_out):
            mods, n = [], 4
            for w in widths:
                mods += [nn.Linear(n, w), activation()]
                n = w
            return nn.Sequential(*mods, nn.Linear(n, d_out)).to(dev)

        return tower(act_dim), tower(1), (0.1 * torch.randn(act_dim)).to(dev)

    def policy(widths, act_dim, activation, seed):
        actor, critic, log_std = towers(widths, act_dim, activation)
        return MlpActorCritic.from_modules(actor, critic, log_std, [-0.5] * act_dim, [0.5] * act_dim, seed=seed)

    # the sampled policy: 17 envs = two 16-env tiles, the second ragged; act_dim 5 = two Philox blocks per env
    for name, activation in (("tanh", nn.Tanh), ("relu", nn.ReLU)):
        pol = policy([16], 5, activation, seed=11)
        obs = randn(17, 4)
        extra = {"norm_obs": torch.zeros(17, 4, device=dev), "mean": torch.zeros(17, 5, device=dev)}
        for call in range(2):
            env_action, action, value, log_prob = pol.act(obs, out=extra)
            digest(f"policy_{name}_17x4x16x5/call{call}", dict(extra, env_action=env_action, action=action, value=value, log_prob=log_prob, calls=pol.calls))

    # the pipeline: 16 words per env, 16 envs per wavefront, 65 envs = two blocks, the last ragged; both noises on
    pipe = AgentPipeline(65, 5, [-1.0] * 3, [1.0] * 3, dt=0.005, stack=2, action_in_observation=True, integrate_action=True,
                         action_noise=[0.1, 0.2, 0.3], action_lag=0.05, observation_noise=[0.01, 0.02, 0.03, 0.04, 0.05], seed=5)
    state = lambda: dict(pipe.state_tensors(), command=pipe.command, final_observation=pipe.final_observation)  # noqa: E731
    pipe.reset(randn(65, 5))
    digest("pipeline_65x5x3x2/reset_all", state())
    pipe.shape_action(randn(65, 3, scale=0.5))
    digest("pipeline_65x5x3x2/shape_action", state())
    terminated = torch.zeros(65, dtype=torch.uint8, device=dev)
    terminated[40] = 1
    pipe.observe(randn(65, 5), terminated, None, randn(65, 5))
    digest("pipeline_65x5x3x2/observe_one_terminated", state())
    mask = torch.zeros(65, dtype=torch.uint8, device=dev)
    mask[3], mask[64] = 1, 1
    pipe.reset(randn(65, 5), mask)
    digest("pipeline_65x5x3x2/masked_reset", state())

    # VecNormalize, training: 1 env (the one block's draw is the last) and 257 envs (two blocks of 129 and 128 rows)
    for n in (1, 257):
        norm = RunningNormalizer(n, 3, norm_obs=True, norm_reward=True, training=True)
        norm.reset(randn(n, 3))
        outs = {"norm_obs": torch.zeros(n, 3, device=dev), "episode_starts": torch.zeros(n, dtype=torch.uint8, device=dev)}
        for step in range(2):
            done = (torch.rand(n, generator=gen) < 0.3).to(torch.uint8).to(dev)
            reward = norm.step(randn(n, 3, scale=2.0), randn(n), done, None, out=outs)
            digest(f"vecnorm_{n}x3/step{step}", dict(outs, reward=reward, obs_stats=norm.obs_stats, ret_stats=norm.ret_stats, returns=norm.returns,
                                                     mean_f32=norm.obs_mean_f32, std_f32=norm.obs_std_f32, ticket=norm.workspace[:4]))

    # episodes, window 2: 200 envs = one block, 520 envs = three blocks of 174, 174 and 172; four episodes end per step
    for n in (200, 520):
        ep = EpisodeStatistics(n, window=2)
        for step in range(2):
            done = torch.zeros(n, dtype=torch.uint8, device=dev)
            done[[1 + step, 70, n // 2, n - 1]] = 1
            ep.step(randn(n), done, None)
            digest(f"episodes_{n}_window2/step{step}", dict(ep.state_tensors(), ticket=ep.workspace[:4]))

    # the PPO update. Every valid network has more than PPO_THREADS trainable words (one MFMA layer is 256), so the
    # fold always has several blocks: 4 with the [16] towers, some forty with [64, 64]. Four waves per gradient block here, so a
    # minibatch of n samples has ceil(ceil(n / 16) / 4) gradient partials: 2112 -> 33, 2048 -> 32, 100 -> 2.
    def ppo(label, widths, act_dim, T, N, batch, split):
        pol = policy(widths, act_dim, nn.Tanh, seed=3)
        buf = RolloutBuffer(T, N, obs_shape=(4,), action_shape=(act_dim,), device=dev)
        buf.observations.copy_(randn(T, N, 4))
        buf.actions.copy_(randn(T, N, act_dim, scale=0.3))
        buf.values.copy_(randn(T, N))
        buf.log_probs.copy_(-1.0 + randn(T, N, scale=0.1))
        buf.advantages, buf.returns = randn(T, N), randn(T, N)
        buf.pos, buf.full = T, True
        tr = PpoTrainer(pol, n_epochs=2, batch_size=batch, normalize_advantage=True, ent_coef=0.01, seed=9)
        if split:  # the data-parallel halves without a process group: a one-rank slot, the exchange does nothing
            tr._grad_exchange = SlotExchange(int(tr._lib.upkie_ppo_slot_bytes(ctypes.byref(pol.shape))) // 4, dev)
        tr.prepare(buf)
        if split:
            tr._adv_exchange = SlotExchange(int(tr._lib.upkie_ppo_advantage_slot_bytes(T * N, tr._mb)) // 4, dev)
        gen_host = torch.Generator().manual_seed(21)  # (the device randperm may differ between processes: host permutations)
        for e in range(tr.n_epochs):
            tr.perm[e].copy_(torch.randperm(T * N, generator=gen_host).to(torch.int32))
        stats = tr.update(buf, sync=False)
        digest(label, {"packed": pol.packed, "m": tr.m, "v": tr.v, "stats": stats, "adv_stats": tr.adv_stats, "control": tr.control,
                       "ticket": tr.workspace[:4], "slot": tr._grad_exchange.slots if split else None})

    ppo("ppo_16x5_2212_batch2112", [16], 5, 4, 553, 2112, False)  # minibatches of 2112 and 100 samples: 33 and 2 partials
    ppo("ppo_16x5_2048_batch2048", [16], 5, 4, 512, 2048, False)  # exactly 32 partials
    ppo("ppo_64x64x1_300_batch128", [64, 64], 1, 3, 100, 128, False)  # minibatches of 128, 128 and 44
    ppo("ppo_split_16x5_2212_batch2112", [16], 5, 4, 553, 2112, True)
    torch.cuda.synchronize()
    print("ab_trainer_bits child done", flush=True)


def main():
    args = sys.argv[1:]
    timeout = 300
    if "--timeout" in args:
        i = args.index("--timeout")
        timeout = int(args[i + 1])
        del args[i:i + 2]
    if len(args) < 2:
        sys.exit(__doc__)
    digests = []
    for path in args:
        env = dict(os.environ, UPKIE_HIP_LIBRARY=os.path.abspath(path))
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, timeout=timeout)
        if res.returncode != 0 or "ab_trainer_bits child done" not in res.stdout:
            print(res.stdout[-2000:], res.stderr[-4000:], sep="\n")
            sys.exit(f"{path}: the child ended with status {res.returncode}")
        digests.append(dict(line.split() for line in res.stdout.splitlines() if "/" in line and len(line.split()) == 2))
    different = 0
    for label in digests[0]:
        values = [d.get(label) for d in digests]
        same = all(v == values[0] for v in values)
        different += not same
        print(f"{label:64s} {values[0][:16]} " + ("same" if same else "DIFFERENT: " + " ".join(str(v)[:16] for v in values[1:])))
    print(f"{len(digests[0])} buffers under {len(args)} builds ({', '.join(args)}): " + (f"{different} DIFFER" if different else "every digest equal"))
    sys.exit(1 if different or any(set(d) != set(digests[0]) for d in digests) else 0)


if __name__ == "__main__":
    child() if sys.argv[1:2] == ["--child"] else main()
