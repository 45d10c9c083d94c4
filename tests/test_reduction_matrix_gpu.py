"""Every row of tests/reduction_shapes.py on the MI355X: `EpisodeStatistics` (csrc/episodes.hpp) through its scripted stream
against the Monitor twins, bit for bit behind every step, eager and replayed from a graph; `RunningNormalizer`
(csrc/vecnorm.hpp) in its four forms against the fp64 twin under the bounds of tests/test_vecnorm_gpu.py behind every step;
and the data-parallel form (launch A into a slot, launch M over the slots) with every shard in this one process.
tests/test_reduction_matrix.py shows without a GPU that the tables cover the grid geometries and that these checks are sharp."""

import types

import numpy as np
import pytest
import torch

from tests import reduction_shapes as S
from tests import vecnorm_reference as V
from tests.test_time_limits_gpu import _compare
from tests.test_vecnorm_gpu import _check_stats, _ulps
from upkie_amd.episodes import EpisodeStatistics
from upkie_amd.graphs import GraphedLoop
from upkie_amd.normalize import NORM_OBS, NORM_REWARD, TRAINING, RunningNormalizer, packed_offsets

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), device=DEV)


def _ticket(x):
    return int(x.workspace[:4].cpu().view(torch.int32))


# ================================================================ episode statistics
class _Stream:
    """A script on the device: terminated as bool, truncated as bytes (both are taken)."""

    def __init__(self, script):
        self.s = script
        self.rewards, self.terminated, self.truncated = _dev(script.rewards), _dev(script.terminated), _dev(script.truncated.astype(np.uint8))
        self.mask = _dev(script.mask)

    def step(self, stats, t):
        given = self.s.given[t]
        stats.step(self.rewards[t], self.terminated[t] if given != "truncated" else None, self.truncated[t] if given != "terminated" else None)
        if t == self.s.reset_after:
            stats.reset(self.mask)


@pytest.mark.parametrize("row", S.EPISODE_ROWS, ids=S.EPISODE_IDS)
def test_episode_statistics_bit_equal_to_the_twin_at_every_grid(row):
    script = S.episode_script(row)
    stream = _Stream(script)
    stats = EpisodeStatistics(row.N, window=row.window, device=DEV)
    twin = S.monitor_twin(row)
    worst = 0.0
    for t in range(len(script.given)):
        stream.step(stats, t)
        term, trunc = S.flags_of(script, t)
        twin.step(script.rewards[t], term, trunc)
        if t == script.reset_after:
            twin.reset(script.mask)
        _compare(stats, twin)
        if twin.ep_info_buffer:  # (the one comparison of `_compare` that is not of bits: the sequential mean against np.mean)
            ref = twin.safe_mean("r")
            worst = max(worst, abs(float(stats.means[0]) - ref) / (1e-12 * max(1.0, abs(ref))))
    assert _ticket(stats) == 0, "the ticket is back at zero"
    plan = S.episodes_plan(row)
    print(f"matrix episodes N {row.N} window {row.window} ({plan['blocks']} blocks of {plan['rows']}): {len(script.given)} steps, "
          f"{twin.total_episodes} episodes, every ring entry, mean, counter and running sum bit-equal; ep_rew_mean against np.mean: "
          f"worst error / bound {worst:.3f}")


def test_episode_statistics_replayed_from_a_graph():
    """The row with 257 blocks and a two-stage ring: the script eagerly and from one captured graph (the masked reset in
    it), equal bits, and the twin's."""
    row = next(r for r in S.EPISODE_ROWS if (r.N, r.window) == S.GRAPHED_EPISODE_ROW)
    script = S.episode_script(row)
    stream, T = _Stream(script), len(script.given)
    runs = []
    for graphed in (False, True):
        stats = EpisodeStatistics(row.N, window=row.window, device=DEV)
        slot = {"t": 0}

        def body():
            stream.step(stats, slot["t"])
            slot["t"] = (slot["t"] + 1) % T

        if graphed:
            slot["t"] = T - 1
            loop = GraphedLoop(body, unroll=T, warmup=1)
            for tensor in stats.state_tensors().values():
                tensor.zero_()  # (the warm-up step ran eagerly: start the replay from the same state; the workspace keeps what it left)
            loop.replay()
        else:
            for _ in range(T):
                body()
        torch.cuda.synchronize()
        assert _ticket(stats) == 0
        runs.append((stats, {k: v.cpu().clone() for k, v in stats.state_tensors().items()}))
    for k, eager in runs[0][1].items():
        replayed = runs[1][1][k]
        assert torch.equal(eager.view(torch.uint8), replayed.view(torch.uint8)), k
    twin = S.monitor_twin(row)
    S.run_episode_script(script, twin)
    _compare(runs[1][0], twin)


# ================================================================ the running normaliser
def _device_stats(norm, returns=None):
    return {"obs_mean": norm.obs_mean.cpu().numpy(), "obs_var": norm.obs_var.cpu().numpy(), "obs_count": float(norm.obs_count),
            "ret": tuple(float(x) for x in norm.ret_stats.cpu()), "returns": (norm.returns if returns is None else returns).cpu().numpy(),
            "mean_f32": norm.obs_mean_f32.cpu().numpy(), "std_f32": norm.obs_std_f32.cpu().numpy()}


def _worse(worst, ratios):
    for k, v in ratios.items():
        worst[k] = max(worst.get(k, 0.0), v)


def _fp32_expression(obs, norm, clip=10.0):
    """(u - m) / sd in fp32 with the device's own mirrors, clipped."""
    m, s = norm.obs_mean_f32.cpu().numpy(), norm.obs_std_f32.cpu().numpy()
    return np.clip((obs - m) / s, np.float32(-clip), np.float32(clip))


CASES = [(row, form) for row in S.VECNORM_ROWS for form in S.FORMS]


@pytest.mark.parametrize("row, form", CASES, ids=[f"{i}-{f}" for i in S.VECNORM_IDS for f in S.FORMS])
def test_normaliser_against_the_twin_at_every_grid(row, form):
    """two_launch: launch A then launch B, with `norm_obs` and `episode_starts` outputs; one_launch: norm_reward off and no
    normalised observations asked, so launch A writes the per-env outputs; reset_first: `reset(obs)` (cols = D) and then the
    steps; no_norm_obs: cols = 1. The checks and bounds are tests/test_vecnorm_gpu.py's, behind every step."""
    N, D = row.N, row.D
    obs, reward, term, trunc = S.vecnorm_inputs(N, D)
    T = obs.shape[0]
    norm = RunningNormalizer(N, D, norm_obs=form != "no_norm_obs", norm_reward=form != "one_launch", device=DEV)
    twin = S.twin_of(N, D, form)
    d_obs, d_rew, d_term, d_trunc = _dev(obs), _dev(reward), _dev(term), _dev(trunc).bool()
    norm_obs = torch.full((N, D), np.nan, device=DEV)
    starts = torch.full((N,), 7, dtype=torch.uint8, device=DEV)
    out = {"episode_starts": starts} if form == "one_launch" else {"norm_obs": norm_obs, "episode_starts": starts}
    worst = {}
    if form == "reset_first":
        norm.returns.fill_(3.0)
        norm.reset(d_obs[T - 1])
        twin.reset(obs[T - 1])
        _check_stats(norm, twin)
        _worse(worst, S.stats_ratios(_device_stats(norm), twin))
    for t in range(T):
        r = norm.step(d_obs[t], d_rew[t], d_term[t], d_trunc[t], out=out)
        want_obs, want_r, want_starts = twin.step(obs[t], reward[t], term[t], trunc[t])
        if form == "one_launch":
            assert np.array_equal(r.cpu().numpy(), reward[t]), "the raw reward"
        else:
            assert _ulps(r.cpu().numpy(), want_r) <= 1, t
            got = norm_obs.cpu().numpy()
            np.testing.assert_allclose(got, want_obs, rtol=2e-6, atol=2e-6)
            assert np.array_equal(got, _fp32_expression(obs[t], norm) if form != "no_norm_obs" else obs[t]), t
        np.testing.assert_array_equal(starts.cpu().numpy(), want_starts)
        _check_stats(norm, twin)
        _worse(worst, S.stats_ratios(_device_stats(norm), twin))
    if form != "no_norm_obs":
        np.testing.assert_array_equal(norm.normalize_obs(d_obs[T - 1]).cpu().numpy(), _fp32_expression(obs[T - 1], norm))
    assert _ticket(norm) == 0, "the ticket is back at zero"
    print(f"matrix vecnorm {N}x{D} {form}: worst error / bound: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


# ---------------------------------------------------------------- the data-parallel form in one process
def _arguments(norm, obs, reward, term, trunc, packed, norm_obs, reward_out, starts):
    """The arguments every vecnorm launch begins with (upkie_amd.normalize.RunningNormalizer._launch), for a training step."""
    return (norm.num_envs, norm.obs_dim, obs.data_ptr(), reward.data_ptr(), term.data_ptr(), trunc.data_ptr(), norm.obs_stats.data_ptr(),
            norm.ret_stats.data_ptr(), norm.returns.data_ptr(), norm.workspace.data_ptr(), TRAINING | NORM_OBS | NORM_REWARD, norm.gamma,
            norm.epsilon, norm.clip_obs, norm.clip_reward, norm.obs_mean_f32.data_ptr(), norm.obs_std_f32.data_ptr(), packed.data_ptr(),
            norm_obs.data_ptr(), reward_out.data_ptr(), starts.data_ptr())


@pytest.mark.parametrize("D, shards", S.SHARDED, ids=[f"D{d}-" + "+".join(map(str, s)) for d, s in S.SHARDED])
def test_data_parallel_form_with_every_shard_in_one_process(D, shards):
    """K normalisers without a group, one per shard of unequal size: `upkie_vecnorm_moments_local` of each into row k of one
    [K, slot_doubles] tensor (what the exchange leaves on every rank), then `upkie_vecnorm_merge` on every shard with
    world = K. Every shard then holds the same bits, the statistics are those of one normaliser over the concatenated
    envs, and with K = 1 every output is the fused step's, bit for bit."""
    K, N = len(shards), sum(shards)
    obs, reward, term, trunc = S.vecnorm_inputs(N, D)
    T = obs.shape[0]
    edges = np.concatenate([[0], np.cumsum(shards)])
    norms = [RunningNormalizer(n, D, device=DEV) for n in shards]
    library = norms[0]._lib
    slot_doubles = int(library.upkie_vecnorm_slot_bytes(D)) // 8
    assert slot_doubles == 3 * (D + 1)
    slots = torch.full((K, slot_doubles), np.nan, dtype=torch.float64, device=DEV)
    mean_at, std_at = packed_offsets(D)
    data = [[_dev(np.ascontiguousarray(x[:, a:b])) for x in (obs, reward, term, trunc)] for a, b in zip(edges[:-1], edges[1:])]
    packed = [torch.zeros(std_at + D, device=DEV) for _ in shards]
    outs = [(torch.empty(n, D, device=DEV), torch.empty(n, device=DEV), torch.empty(n, dtype=torch.uint8, device=DEV)) for n in shards]
    twin = V.VecNormalizeTwin(N, D)
    fused = RunningNormalizer(N, D, device=DEV) if K == 1 else None
    worst, count = {}, 1e-4
    for t in range(T):
        args = [_arguments(norm, *(x[t] for x in data[k]), packed[k], *outs[k]) for k, norm in enumerate(norms)]
        for k, norm in enumerate(norms):
            norm._launcher(library.upkie_vecnorm_moments_local, *args[k], slots[k].data_ptr())
        for k, norm in enumerate(norms):
            norm._launcher(library.upkie_vecnorm_merge, *args[k], slots.data_ptr(), K)
        torch.cuda.synchronize()
        first = norms[0]
        for k, norm in enumerate(norms[1:], 1):
            for name in ("obs_stats", "ret_stats", "obs_mean_f32", "obs_std_f32"):
                a, b = getattr(first, name), getattr(norm, name)
                assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), (t, k, name)
            assert torch.equal(packed[0], packed[k])
        assert torch.equal(packed[0][mean_at:mean_at + D], first.obs_mean_f32) and torch.equal(packed[0][std_at:std_at + D], first.obs_std_f32)
        count += float(N)
        assert float(first.obs_count) == count == float(first.ret_count), "the counts grow by the total env count"
        want_obs, want_r, want_starts = twin.step(obs[t], reward[t], term[t], trunc[t])
        whole = types.SimpleNamespace(obs_mean=first.obs_mean, obs_var=first.obs_var, ret_stats=first.ret_stats, obs_count=first.obs_count,
                                      returns=torch.cat([n.returns for n in norms]), obs_mean_f32=first.obs_mean_f32,
                                      obs_std_f32=first.obs_std_f32)
        _check_stats(whole, twin)
        _worse(worst, S.stats_ratios(_device_stats(first, whole.returns), twin))
        got_obs, got_r, got_starts = (torch.cat([o[i] for o in outs]).cpu().numpy() for i in range(3))
        assert _ulps(got_r, want_r) <= 1, t
        np.testing.assert_array_equal(got_starts, want_starts)
        np.testing.assert_allclose(got_obs, want_obs, rtol=2e-6, atol=2e-6)
        assert np.array_equal(got_obs, _fp32_expression(obs[t], first)), t
        if fused is not None:
            f_obs, f_starts = torch.empty(N, D, device=DEV), torch.empty(N, dtype=torch.uint8, device=DEV)
            f_r = fused.step(*(x[t] for x in data[0]), out={"norm_obs": f_obs, "episode_starts": f_starts})
            for a, b in ((fused.obs_stats, first.obs_stats), (fused.ret_stats, first.ret_stats), (fused.returns, first.returns),
                         (fused.obs_mean_f32, first.obs_mean_f32), (fused.obs_std_f32, first.obs_std_f32), (f_obs, outs[0][0]),
                         (f_r, outs[0][1]), (f_starts, outs[0][2])):
                assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), t
    assert all(_ticket(n) == 0 for n in norms)
    print(f"matrix vecnorm sharded D {D} shards {'+'.join(map(str, shards))}: worst error / bound: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
