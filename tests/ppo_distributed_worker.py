"""Run under `python -m torch.distributed.run` on a GPU box (tests/test_ppo_distributed_gpu.py; not a test file itself):
data-parallel PpoTrainer and RunningNormalizer.

  world1 (--nproc-per-node 1, UPKIE_FORCE_PROCESS_GROUP=1: a one-rank RCCL group): the split path with the group
    against the fused path without one, bit for bit.
  world2 (--nproc-per-node 2, gloo, both ranks on cuda:0): two ranks with different data against one learner /
    normaliser on the union.
  Both also run an asymmetric policy (a row of tests/asymmetric_shapes.py, critic rows of its own in the buffer) and,
  world1, a normaliser attached to its critic block.

Every rank writes its findings as JSON to `<out>.<rank>`."""

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402
import torch.nn as nn  # noqa: E402

from tests import asymmetric_reference as AR  # noqa: E402
from tests import asymmetric_shapes as AS  # noqa: E402
from tests import ppo_reference as R  # noqa: E402
from tests.test_ppo_gpu import CASES, T, _tower  # noqa: E402
from upkie_amd.distributed import init_distributed  # noqa: E402
from upkie_amd.normalize import RunningNormalizer  # noqa: E402
from upkie_amd.policies import MlpActorCritic  # noqa: E402
from upkie_amd.ppo import PpoTrainer, trainable_offset  # noqa: E402
from upkie_amd.rollout import RolloutBuffer  # noqa: E402

DEV = "cuda:0"


def _np(t):
    return t.detach().double().cpu().numpy()


def _rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _policy(case, wseed, seed):
    _, D, widths, A, act = case
    torch.manual_seed(wseed)
    actor, critic = _tower(D, widths, A, act).to(DEV), _tower(D, widths, 1, act).to(DEV)
    log_std = nn.Parameter(torch.full((A,), -0.5, device=DEV))
    return MlpActorCritic.from_modules(actor, critic, log_std, torch.full((A,), -1.0), torch.full((A,), 1.0), seed=seed)


def _setup(case, wseed, dseed, first=False):
    """tests/mlp_shapes.py's `trainer_case` with separate seeds for the weights (`wseed`, the same on every rank) and for the
    data and the policy's noise (`dseed`, one per rank)."""
    N, D, widths, A, act = case
    pol = _policy(case, wseed, dseed)
    buf = RolloutBuffer(T, N, obs_shape=(D,), action_shape=(A,), device=DEV)
    gen = torch.Generator(DEV).manual_seed(dseed + 7)
    buf.observations.copy_(torch.randn(T, N, D, device=DEV, generator=gen))
    for t in range(T):
        pol.act(buf.observations[t], out={"action": buf.actions[t], "value": buf.values[t], "log_prob": buf.log_probs[t]})
    _fill(buf, N, dseed, first)
    return pol, buf


def _setup_asymmetric(row, dseed, first=False):
    """`_setup` for a row of tests/asymmetric_shapes.py: an asymmetric policy (`AS.policy`: the row's weights on every
    rank, the noise under `dseed`), a buffer whose critic rows are drawn apart from the observations, data under `dseed`."""
    N, D, A, Dc = row.N, row.obs_dim, row.act_dim, row.critic_obs_dim
    pol, _, _, _ = AS.policy(row, log_std=nn.Parameter(torch.full((A,), -0.5, device=DEV)))
    pol.reseed(dseed)
    buf = RolloutBuffer(T, N, obs_shape=(D,), action_shape=(A,), device=DEV, critic_obs_shape=(Dc,))
    gen = torch.Generator(DEV).manual_seed(dseed + 7)
    buf.observations.copy_(torch.randn(T, N, D, device=DEV, generator=gen))
    buf.critic_observations.copy_(torch.randn(T, N, Dc, device=DEV, generator=gen))
    for t in range(T):
        pol.act(buf.observations[t], out={"action": buf.actions[t], "value": buf.values[t], "log_prob": buf.log_probs[t]},
                critic_obs=buf.critic_observations[t])
    _fill(buf, N, dseed, first)
    return pol, buf


def _fill(buf, N, dseed, first):
    """Old log-probs that make ratios clip (unless `first`), advantages, returns and old values around the policy's."""
    rng = np.random.default_rng(dseed)
    if not first:
        delta = rng.normal(0.0, 0.25, size=(T, N))
        for bound in (1.2, 0.8):
            near = np.abs(np.exp(-delta) - bound) < 1e-3
            delta[near] += 0.01
        buf.log_probs.add_(torch.as_tensor(delta, dtype=torch.float32, device=DEV))
    buf.advantages = torch.as_tensor(rng.normal(0.3 + 0.2 * dseed % 3, 1.0, size=(T, N)), dtype=torch.float32, device=DEV)
    buf.returns = (buf.values + torch.as_tensor(rng.normal(0.0, 1.0, size=(T, N)), dtype=torch.float32, device=DEV)).contiguous()
    buf.values.add_(torch.as_tensor(rng.normal(0.0, 0.2, size=(T, N)), dtype=torch.float32, device=DEV))
    buf.pos, buf.full = T, True


def _state(pol, tr):
    return [pol.packed.clone(), tr.m.clone(), tr.v.clone(), tr.scalars.clone()]


def _restore(pol, tr, st):
    for dst, src in zip((pol.packed, tr.m, tr.v, tr.scalars), st):
        dst.copy_(src)


def _gather(t: torch.Tensor, group):
    """Every rank's copy of `t` (host tensors, rank order)."""
    host = t.detach().cpu().contiguous()
    rows = [torch.empty_like(host) for _ in range(dist.get_world_size(group))]
    dist.all_gather(rows, host, group=group)
    return rows


# ---------------------------------------------------------------- world 1: split path == fused path, bit for bit
def _split_against_fused(pol, buf, group, total):
    """[packed, m, v, scalars, stats equal; training moved the weights] of the split path with the group against the fused
    path without one, from the same state."""
    kw = dict(n_epochs=2, batch_size=(total + 2) // 3, seed=1, ent_coef=0.003)
    fused = PpoTrainer(pol, **kw)
    fused.prepare(buf)
    s0 = _state(pol, fused)
    fused.update(buf, sync=False)
    want = _state(pol, fused) + [fused.stats.clone()]
    _restore(pol, fused, s0)
    split = PpoTrainer(pol, process_group=group, **kw)
    split.prepare(buf)
    assert torch.equal(split.perm, fused.perm)
    split.update(buf, sync=False)
    got = _state(pol, split) + [split.stats.clone()]
    torch.cuda.synchronize()
    return [bool(torch.equal(a, b)) for a, b in zip(got, want)] + [not torch.equal(want[0], s0[0])]


def world1(group):
    out = {}
    for case in CASES:
        pol, buf = _setup(case, 0, 3)
        out[f"ppo {case}"] = _split_against_fused(pol, buf, group, T * case[0])
    row = AS.ROWS[5]
    pol, buf = _setup_asymmetric(row, 3)
    assert pol.asymmetric and buf.critic_observations is not None
    out[f"ppo asymmetric {AS.row_id(row)}"] = _split_against_fused(pol, buf, group, T * row.N)
    for norm_reward, outputs in ((True, ("norm_obs", "episode_starts")), (False, ("episode_starts",))):
        out[f"vecnorm norm_reward={norm_reward}"] = _normalizer_world1(group, norm_reward, outputs)
    out["vecnorm critic tower"] = _critic_normalizer_world1(group)
    return out


def _normalizer_world1(group, norm_reward, outputs):
    N, D = 1000, 5
    case = (N, D, [40, 24], 3, "tanh")
    runs = []
    for g in (None, group):
        pol = _policy(case, 0, 0)  # (attached before its first call)
        norm = RunningNormalizer(N, D, norm_reward=norm_reward, device=DEV, process_group=g)
        norm.attach(pol)
        gen = torch.Generator(DEV).manual_seed(5)
        obs = torch.randn(N, D, device=DEV, generator=gen) * 2 + 0.5
        norm.reset(obs)
        seq = []
        for _ in range(20):
            obs = torch.randn(N, D, device=DEV, generator=gen) * 2 + 0.5
            reward = torch.randn(N, device=DEV, generator=gen)
            term = torch.rand(N, device=DEV, generator=gen) < 0.05
            trunc = torch.rand(N, device=DEV, generator=gen) < 0.02
            outs = {"norm_obs": torch.empty(N, D, device=DEV), "episode_starts": torch.empty(N, dtype=torch.uint8, device=DEV)}
            outs = {k: v for k, v in outs.items() if k in outputs}
            r = norm.step(obs, reward, term, trunc, out=outs).clone()
            seq.append([norm.obs_stats.clone(), norm.ret_stats.clone(), norm.returns.clone(), norm.obs_mean_f32.clone(), norm.obs_std_f32.clone(),
                        pol.packed.clone(), r] + [outs[k].clone() for k in outputs])
        runs.append(seq)
    torch.cuda.synchronize()
    return all(torch.equal(a, b) for sa, sb in zip(*runs) for a, b in zip(sa, sb))


def _critic_normalizer_world1(group):
    """A normaliser of the critic's rows, attached to an asymmetric policy's critic block: the same bits with the group as
    without, the policy's packed words included, and the actor's block is left alone."""
    row = AS.ROWS[5]
    N, D, Dc = row.N, row.obs_dim, row.critic_obs_dim
    runs = []
    for g in (None, group):
        pol, _, _, _ = AS.policy(row)  # (attached before its first call)
        norm = RunningNormalizer(N, Dc, norm_reward=False, clip_obs=3.0, device=DEV, process_group=g)
        norm.attach(pol, tower="critic")
        gen = torch.Generator(DEV).manual_seed(5)
        rows = torch.randn(N, Dc, device=DEV, generator=gen) * 2 + 0.5
        norm.reset(rows)
        seq = []
        for _ in range(20):
            rows = torch.randn(N, Dc, device=DEV, generator=gen) * 2 + 0.5
            reward = torch.randn(N, device=DEV, generator=gen)
            term = torch.rand(N, device=DEV, generator=gen) < 0.05
            nobs = torch.empty(N, Dc, device=DEV)
            norm.step(rows, reward, term, out={"norm_obs": nobs})
            value = pol.value(rows, out=torch.empty(N, device=DEV))
            seq.append([norm.obs_stats.clone(), norm.obs_mean_f32.clone(), norm.obs_std_f32.clone(), pol.packed.clone(), nobs, value.clone()])
        at = pol.critic_stats_offset()
        moved = float(pol.packed[at:at + Dc].abs().sum()) > 0.0 and bool(torch.equal(pol.packed[at:at + Dc], norm.obs_mean_f32))
        untouched = bool(torch.equal(pol.packed[:D], torch.zeros(D, device=DEV)))
        runs.append((seq, moved and untouched))
    torch.cuda.synchronize()
    return all(ok for _, ok in runs) and all(torch.equal(a, b) for sa, sb in zip(runs[0][0], runs[1][0]) for a, b in zip(sa, sb))


# ---------------------------------------------------------------- world 2: two gloo ranks == one learner on the union
def _union_perm(perms, N, mb):
    """Union minibatch j = rank 0's minibatch j, then rank 1's, each sample mapped to the union buffer [T, sum N]."""
    W = len(perms)
    mapped = []
    for r, p in enumerate(perms):
        t, n = p // N, p % N
        mapped.append(t * (W * N) + r * N + n)
    total = perms[0].numel()
    return torch.cat([m[s:s + mb] for s in range(0, total, mb) for m in mapped])


def _union_buffer(buf, group, case):
    N, D, _, A, _ = case
    W = dist.get_world_size(group)
    u = RolloutBuffer(T, W * N, obs_shape=(D,), action_shape=(A,), device=DEV)
    for name in ("observations", "actions", "values", "log_probs"):
        rows = _gather(getattr(buf, name), group)
        getattr(u, name).copy_(torch.cat(rows, dim=1))
    u.advantages = torch.cat(_gather(buf.advantages, group), dim=1).to(DEV).contiguous()
    u.returns = torch.cat(_gather(buf.returns, group), dim=1).to(DEV).contiguous()
    u.pos, u.full = T, True
    return u


def world2(group, rank):
    out = {}
    case = (500, 5, [40, 24], 3, "tanh")
    N, lr = case[0], 3e-4
    pol, buf = _setup(case, 10, 20 + rank)
    mb = (T * N + 3) // 4
    kw = dict(lr=lr, n_epochs=2, batch_size=mb, seed=11)
    tr = PpoTrainer(pol, process_group=group, **kw)
    if rank == 1:  # (replicas that start apart: broadcast_parameters makes them rank 0's)
        pol.packed[trainable_offset(pol.shape):] += 0.01
        tr.m.fill_(1.0)
    out["start_apart"] = not torch.equal(*_gather(pol.packed, group))
    tr.broadcast_parameters(0)
    s0 = _state(pol, tr)
    out["start_equal"] = bool(torch.equal(*_gather(s0[0], group)))
    tr.prepare(buf)
    perms = [tr.perm[e].clone() for e in range(2)]
    stats = tr.update(buf, sync=False).clone()
    after = _state(pol, tr)
    torch.cuda.synchronize()
    out["ranks_bit_equal"] = [bool(torch.equal(*_gather(t, group))) for t in after] + [bool(torch.equal(*_gather(stats, group)))]
    # a rank that trains alone on its shard ends elsewhere
    _restore(pol, tr, s0)
    alone = PpoTrainer(pol, **kw)
    alone.train(buf, sync=False)
    out["alone_differs"] = not torch.equal(pol.packed, after[0])
    # one learner on the union buffer, its permutation overwritten so that union minibatch j = the ranks' minibatches j
    ubuf = _union_buffer(buf, group, case)
    all_perms = [[p.long().cpu() for p in _gather(perms[e], group)] for e in range(2)]
    if rank == 0:
        _restore(pol, tr, s0)
        union = PpoTrainer(pol, lr=lr, n_epochs=2, batch_size=2 * mb, seed=11)
        union.prepare(ubuf)
        for e in range(2):
            union.perm[e].copy_(_union_perm(all_perms[e], N, mb).to(torch.int32))
        ustats = union.update(ubuf, sync=False)
        torch.cuda.synchronize()
        rel, absd = [], []
        for a, u in zip(after[:1], [pol.packed]):
            da, du = _np(a) - _np(s0[0]), _np(u) - _np(s0[0])
            # per tensor of the policy's sources (log_std, each weight and bias)
            idx = pol._index.cpu().numpy()
            sizes = [t.numel() for t in pol.sources()]
            flat_a, flat_u = np.zeros(sum(sizes) + 1), np.zeros(sum(sizes) + 1)
            flat_a[idx], flat_u[idx] = da, du
            start = sum(sizes[:4])
            for n in sizes[4:]:
                rel.append(_rel(flat_a[start:start + n], flat_u[start:start + n]))
                absd.append(float(np.max(np.abs(flat_a[start:start + n] - flat_u[start:start + n]))))
                start += n
        out["union_rel"], out["union_abs_over_lr"] = rel, [x / lr for x in absd]
        s, su = stats.double().cpu().numpy(), ustats.double().cpu().numpy()
        cols = [0, 1, 2, 3, 6]
        ok = np.isclose(s[..., cols], su[..., cols], rtol=2e-3, atol=2e-5)
        out["union_stats_ok"] = bool(ok.all())
        out["union_stats_worst"] = float(np.max(np.abs(s[..., cols] - su[..., cols]) / (2e-5 + 2e-3 * np.abs(su[..., cols]))))
    out["fp64_twin"] = _world2_twin(group, rank)
    out["asymmetric"] = _world2_asymmetric(group, rank)
    out["normalizer"] = _world2_normalizer(group, rank)
    return out


def _world2_twin(group, rank):
    """The first full-batch update against the fp64 twin on the union (tests/test_ppo_gpu.py's bound)."""
    case = (333, 6, [64, 64], 2, "relu")
    lr = 1e-3
    pol, buf = _setup(case, 1, 40 + rank, first=True)
    tr = PpoTrainer(pol, lr=lr, n_epochs=1, batch_size=T * case[0], seed=5, process_group=group)
    src0 = [_np(s) for s in pol.sources()]
    stats = tr.train(buf)
    torch.cuda.synchronize()
    D, A = case[1], case[3]
    cat = lambda t: np.concatenate([x.double().numpy().reshape(T * case[0], -1) for x in _gather(t, group)])  # noqa: E731
    x, act = cat(buf.observations), cat(buf.actions)
    v, lp, adv, ret = (cat(t)[:, 0] for t in (buf.values, buf.log_probs, buf.advantages, buf.returns))
    ref_stats, grads, ratio = R.minibatch(pol.shape, src0, x.reshape(-1, D), act.reshape(-1, A), v, lp, adv, ret)
    return _against_twin_update(pol, stats, ref_stats, grads, ratio, R.trainable(pol.shape, src0), 4, lr)


def _against_twin_update(pol, stats, ref_stats, grads, ratio, params0, first_trainable, lr):
    """One clipped Adam step of the twin's gradient from zero moments against the policy's sources after the update
    (`first_trainable`: where log_std sits among them), and the statistics row: tests/test_ppo_gpu.py's bound."""
    zeros = [0 * g for g in grads]
    params, m, _, _ = R.adam_step(params0, grads, zeros, zeros, 0, 0.5, lr)
    after = [_np(p) for p in pol.sources()[first_trainable:]]
    assert len(after) == len(params0) == len(grads)
    coef = min(1.0, 0.5 / (ref_stats[6] + 1e-6))
    worst = 0.0
    for p1, p0, pr, g in zip(after, params0, params, grads):
        p1 = p1.reshape(pr.shape)
        delta = 1e-5 * np.linalg.norm(g) * coef + 1e-6 * np.abs(g) * coef
        bound = lr * delta / (np.abs(g) * coef + 1e-5) + 2e-7 * np.abs(p0) + 1e-9
        worst = max(worst, float(np.max(np.abs((p1 - p0) - (pr - p0)) / bound)))
    s = stats.double().cpu().numpy()[0, 0]
    stats_ok = bool(np.allclose(s[[0, 1, 2, 3, 6]], ref_stats[[0, 1, 2, 3, 6]], rtol=1e-4, atol=1e-6))
    return {"worst_over_bound": worst, "stats_ok": stats_ok, "ratio_one": bool(np.all(np.abs(ratio - 1.0) < 1e-4))}


def _world2_asymmetric(group, rank):
    """An asymmetric policy on two ranks, each with its own observations and critic rows: the same bits on both after the
    update, and the first full-batch update against the composed fp64 twin on the union (`_world2_twin`'s bound)."""
    row = AS.ROWS[4]
    N, D, A, Dc = row.N, row.obs_dim, row.act_dim, row.critic_obs_dim
    lr = 1e-3
    pol, buf = _setup_asymmetric(row, 60 + rank, first=True)
    tr = PpoTrainer(pol, lr=lr, n_epochs=1, batch_size=T * N, seed=5, process_group=group)
    src0 = [_np(s) for s in pol.sources()]
    start_equal = bool(torch.equal(*_gather(pol.packed, group)))
    stats = tr.train(buf).clone()
    torch.cuda.synchronize()
    bit_equal = [bool(torch.equal(*_gather(t, group))) for t in _state(pol, tr) + [stats]]
    moved = not np.array_equal(_np(pol.sources()[AR.N_FIXED + 1]), src0[AR.N_FIXED + 1])
    data_apart = not torch.equal(*_gather(buf.critic_observations, group))
    cat = lambda t: np.concatenate([x.double().numpy().reshape(T * N, -1) for x in _gather(t, group)])  # noqa: E731
    x, xc, act = cat(buf.observations), cat(buf.critic_observations), cat(buf.actions)
    v, lp, adv, ret = (cat(t)[:, 0] for t in (buf.values, buf.log_probs, buf.advantages, buf.returns))
    ref_stats, grads, ratio = AR.minibatch(pol.shape, src0, x.reshape(-1, D), xc.reshape(-1, Dc), act.reshape(-1, A), v, lp, adv, ret)
    twin = _against_twin_update(pol, stats, ref_stats, grads, ratio, AR.trainable(pol.shape, src0), AR.N_FIXED, lr)
    return dict(twin, ranks_bit_equal=bit_equal, start_equal=start_equal, moved=moved, data_apart=data_apart)


def _ulps(a: torch.Tensor, b: torch.Tensor) -> float:
    """Largest |a - b| in units of the fp32 spacing at max(|a|, |b|, 1) (normalised outputs are of order 1)."""
    a, b = a.double().cpu().numpy(), b.double().cpu().numpy()
    scale = np.spacing(np.maximum(np.maximum(np.abs(a), np.abs(b)), 1.0).astype(np.float32)).astype(np.float64)
    return float(np.max(np.abs(a - b) / scale)) if a.size else 0.0


def _world2_normalizer(group, rank):
    N, D = 1000, 5
    W = dist.get_world_size(group)
    lo, hi = rank * N // W, (rank + 1) * N // W
    mine = RunningNormalizer(hi - lo, D, device=DEV, process_group=group)
    whole = RunningNormalizer(N, D, device=DEV)
    gen = torch.Generator(DEV).manual_seed(9)  # (the same inputs on every rank: each takes its slice)
    obs = torch.randn(N, D, device=DEV, generator=gen) * 2 + 0.5
    mine.reset(obs[lo:hi].contiguous())
    whole.reset(obs)
    worst_rel, bit_equal, returns_exact, worst_ulps = 0.0, True, True, 0.0
    for _ in range(20):
        obs = torch.randn(N, D, device=DEV, generator=gen) * 2 + 0.5
        reward = torch.randn(N, device=DEV, generator=gen)
        term = (torch.rand(N, device=DEV, generator=gen) < 0.05).to(torch.uint8)
        nobs_m, nobs_w = torch.empty(hi - lo, D, device=DEV), torch.empty(N, D, device=DEV)
        r_m = mine.step(obs[lo:hi].contiguous(), reward[lo:hi].contiguous(), term[lo:hi].contiguous(), out={"norm_obs": nobs_m}).clone()
        r_w = whole.step(obs, reward, term, out={"norm_obs": nobs_w}).clone()
        st_m = torch.cat([mine.obs_stats, mine.ret_stats])
        st_w = torch.cat([whole.obs_stats, whole.ret_stats])
        worst_rel = max(worst_rel, float(((st_m - st_w).abs() / st_w.abs().clamp_min(1e-300)).max()))
        bit_equal = bit_equal and bool(torch.equal(*_gather(st_m, group)))
        returns_exact = returns_exact and bool(torch.equal(mine.returns, whole.returns[lo:hi]))
        worst_ulps = max(worst_ulps, _ulps(nobs_m, nobs_w[lo:hi]), _ulps(r_m, r_w[lo:hi]))
    return {"worst_rel": worst_rel, "ranks_bit_equal": bit_equal, "returns_exact": returns_exact, "worst_ulps": worst_ulps}


def main():
    mode, out_path = sys.argv[1], sys.argv[2]
    backend = "gloo" if mode == "world2" else None
    rank, world, _ = init_distributed(backend=backend)
    torch.cuda.set_device(0 if mode == "world2" else int(os.environ.get("LOCAL_RANK", "0")))
    group = dist.group.WORLD
    try:
        result = world1(group) if mode == "world1" else world2(group, rank)
    finally:
        dist.barrier()
    with open(f"{out_path}.{rank}", "w") as f:
        json.dump(result, f)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
