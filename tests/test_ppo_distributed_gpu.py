"""Data-parallel PpoTrainer and RunningNormalizer on the MI355X (tests/ppo_distributed_worker.py under
`torch.distributed.run`): a one-rank RCCL group gives the same bits as no group; two gloo ranks sharing cuda:0 train
as one learner on the union of their samples and keep the same bits on both ranks, with a symmetric policy and with an
asymmetric one (critic rows of its own, a normaliser on the critic's block); the sharded example runs."""

import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "ppo_distributed_worker.py")


def _run(nproc, port, args, env, timeout=900):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr", "127.0.0.1",
           "--master-port", str(port)] + args
    return subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)


def _results(out, nproc):
    res = []
    for rank in range(nproc):
        with open(f"{out}.{rank}") as f:
            res.append(json.load(f))
    return res


@pytest.fixture(scope="module")
def world1(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ppo_dist") / "world1")
    env = dict(os.environ, UPKIE_FORCE_PROCESS_GROUP="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    result = _run(1, 29751, [WORKER, "world1", out], env)
    assert result.returncode == 0, result.stderr[-3000:]
    return _results(out, 1)[0]


@pytest.fixture(scope="module")
def world2(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ppo_dist") / "world2")
    result = _run(2, 29753, [WORKER, "world2", out], dict(os.environ, OMP_NUM_THREADS="1"))
    assert result.returncode == 0, result.stderr[-3000:]
    return _results(out, 2)


def test_one_rank_rccl_group_trainer_is_bit_identical_to_no_group(world1):
    cases = {k: v for k, v in world1.items() if k.startswith("ppo")}
    assert len(cases) == 6 and sum("asymmetric" in k for k in cases) == 1
    for case, flags in cases.items():
        # packed, m, v, scalars, stats equal; and training moved the weights
        assert flags == [True] * 6, (case, flags)


def test_one_rank_rccl_group_normalizer_is_bit_identical_to_no_group(world1):
    assert world1["vecnorm norm_reward=True"] and world1["vecnorm norm_reward=False"], world1


def test_one_rank_rccl_group_critic_normalizer_is_bit_identical_to_no_group(world1):
    """`attach(pol, tower="critic")` with the group: statistics, mirrors, the policy's packed words, the normalised rows
    and the values the critic then gives."""
    assert world1["vecnorm critic tower"] is True, world1


def test_two_gloo_ranks_asymmetric_update_same_bits_and_the_fp64_twin_on_the_union(world2):
    """An asymmetric policy, each rank with critic rows of its own: packed, m, v, scalars and stats are the same bits on
    both ranks, and the first full-batch update is the composed twin's on the union of the samples."""
    for rank, res in enumerate(world2):
        a = res["asymmetric"]
        print(f"\nasymmetric world2 rank={rank} worst_over_bound={a['worst_over_bound']:.3e}")
        assert a["start_equal"] and a["data_apart"] and a["moved"], a
        assert a["ranks_bit_equal"] == [True] * 5, (rank, a["ranks_bit_equal"])
        assert a["ratio_one"] and a["stats_ok"], a
        assert a["worst_over_bound"] <= 1.0, a


def test_two_gloo_ranks_hold_the_same_bits_and_differ_from_a_lone_rank(world2):
    for rank, res in enumerate(world2):
        assert res["start_apart"] and res["start_equal"], "broadcast_parameters made the replicas identical"
        assert res["ranks_bit_equal"] == [True] * 5, (rank, res["ranks_bit_equal"])
        assert res["alone_differs"], rank


def test_two_gloo_ranks_match_one_learner_on_the_union(world2):
    res = world2[0]
    print("per-tensor relative deltas:", res["union_rel"], "max |delta| / lr:", res["union_abs_over_lr"])
    assert max(res["union_rel"]) <= 2e-2, res["union_rel"]
    assert max(res["union_abs_over_lr"]) <= 16.0, res["union_abs_over_lr"]
    assert res["union_stats_ok"], res["union_stats_worst"]


def test_two_gloo_ranks_first_update_against_the_fp64_twin_on_the_union(world2):
    for res in world2:
        twin = res["fp64_twin"]
        assert twin["ratio_one"] and twin["stats_ok"], twin
        assert twin["worst_over_bound"] <= 1.0, twin


def test_two_gloo_ranks_normalizer_matches_one_normalizer_on_the_union(world2):
    for res in world2:
        n = res["normalizer"]
        assert n["ranks_bit_equal"] and n["returns_exact"], n
        assert n["worst_rel"] <= 1e-12, n
        assert n["worst_ulps"] <= 2.0, n


def test_sharded_example_runs_on_two_gloo_ranks():
    env = dict(os.environ, EXAMPLE_STEPS="16", EXAMPLE_BACKEND="gloo", OMP_NUM_THREADS="1")
    result = _run(2, 29755, [os.path.join(ROOT, "examples", "ppo_mlp_train_sharded.py")], env, timeout=600)
    assert result.returncode == 0, result.stderr[-3000:]
    lines = [ln for ln in result.stdout.splitlines() if ln.startswith("iteration")]
    assert len(lines) >= 2 and all("nan" not in ln for ln in lines), result.stdout
    assert "weights equal on all ranks" in result.stdout, result.stdout
