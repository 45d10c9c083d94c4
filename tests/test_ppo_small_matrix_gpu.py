"""Every row of tests/ppo_small_shapes.py on the MI355X, each kernel through the C entry point it already has with synthetic
inputs: the advantage statistics (launch 0, and 0a / 0b with 1, 2 and 3 shards in this one process), the explained variance
(phase -1, and phases 0 / 1 / 2 with 1, 2 and 3 shards), launch B and launch C through `upkie_ppo_minibatch_apply` (three
consecutive applies from non-zero m and v, one row again from a captured graph), the controlled form's stop, skip and
counters, and GAE -- against the fp64 twins under the bounds stated in tests/ppo_small_shapes.py.
tests/test_ppo_small_matrix.py shows without a GPU that the tables cover what they claim and that these checks are sharp."""

import ctypes as C

import numpy as np
import pytest
import torch

from tests import ppo_small_shapes as S
from upkie_amd import abi, lib
from upkie_amd.launch import launcher, ptr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64


@pytest.fixture(scope="module")
def api():
    library = lib.load()
    lib.require(library, "upkie_ppo_minibatch_apply_controlled")
    return library, launcher(DEV)


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), device=DEV)


def _same_bytes(a, b):
    return torch.equal(a.reshape(-1).contiguous().view(torch.uint8), b.reshape(-1).contiguous().view(torch.uint8))


# ================================================================ launch 0, 0a, 0b
@pytest.mark.parametrize("row", S.ADV_ROWS, ids=S.ADV_IDS)
def test_advantage_statistics_at_every_size(row, api):
    lb, launch = api
    M = S.adv_plan(row)["M"]
    shards = [tuple(_dev(a) for a in S.adv_inputs(row, s)) for s in range(max(S.SHARD_WORLDS))]
    worst, fused = {}, {}

    def check(out, world, normalize, what):
        got = out.cpu().numpy()
        assert (got[2 * M:] == -7.0).all(), f"{what}: the words behind out are untouched"
        got = got[:2 * M].reshape(M, 2)
        want, _ = S.adv_twin(row, world, normalize)
        exact = (want[:, 0] == 0.0) & (want[:, 1] == 1.0)
        assert exact.all() or normalize, what
        assert np.array_equal(got[exact], want[exact]), f"{what}: (0, 1) exactly without normalisation or below two samples"
        worst[what] = S.adv_ratio(got, row, world, normalize)

    for normalize in (1, 0):
        out = torch.full((2 * M + S.ADV_GUARD,), -7.0, dtype=F64, device=DEV)
        launch(lb.upkie_ppo_advantage_stats, row.total, row.batch, ptr(shards[0][1]), ptr(shards[0][0]), normalize, ptr(out))
        check(out, 1, normalize, "launch 0" if normalize else "launch 0 unnormalised")
        fused[normalize] = out
    for world in S.SHARD_WORLDS:
        slots = torch.full((world, 2 * M), float("nan"), dtype=F64, device=DEV)
        for r in range(world):
            adv, perm = shards[r]
            launch(lb.upkie_ppo_advantage_partials, row.total, row.batch, ptr(perm), ptr(adv), 0, None, world, ptr(slots[r]))
        for r in range(world):
            adv, perm = shards[r]
            launch(lb.upkie_ppo_advantage_partials, row.total, row.batch, ptr(perm), ptr(adv), 1, ptr(slots), world, ptr(slots[r]))
        assert not torch.isnan(slots).any(), "every word of every slot is written"
        for normalize in (1, 0):
            out = torch.full((2 * M + S.ADV_GUARD,), -7.0, dtype=F64, device=DEV)
            launch(lb.upkie_ppo_advantage_finish, row.total, row.batch, normalize, ptr(slots), world, ptr(out))
            check(out, world, normalize, f"0a 0b world {world}" if normalize else f"0a 0b world {world} unnormalised")
            if world == 1:
                assert _same_bytes(out, fused[normalize]), "one shard gives the fused form's bits"
    plan = S.adv_plan(row)
    print(f"matrix advantage {row.total}/{row.batch} (M {M}, last {plan['last']}, {plan['sweeps']} sweeps): (0, 1) exact where it belongs; worst error / "
          "bound: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items() if "unnormalised" not in k))
    assert max(worst.values()) <= 1.0, worst


# ================================================================ explained variance
@pytest.mark.parametrize("row", S.EV_ROWS, ids=S.EV_IDS)
def test_explained_variance_at_every_size(row, api):
    lb, launch = api
    shards = [tuple(_dev(a) for a in S.ev_inputs(row, s)) for s in range(max(S.SHARD_WORLDS))]
    ret, val = shards[0]
    outs = torch.full((2, 2), -7.0, dtype=F64, device=DEV)
    for i in range(2):
        launch(lb.upkie_ppo_explained_variance, row.n, ptr(ret), ptr(val), -1, None, 1, None, ptr(outs[i]))
    assert _same_bytes(outs[0], outs[1]) and float(outs[0, 1]) == -7.0, "two calls give the same bits; the word behind out is untouched"
    worst = {"phase -1": S.ev_ratio(float(outs[0, 0]), row, 1)}
    for world in S.SHARD_WORLDS:
        slots = torch.full((world, 4), float("nan"), dtype=F64, device=DEV)
        out = torch.full((2,), -7.0, dtype=F64, device=DEV)
        for phase in (0, 1):
            for r in range(world):
                launch(lb.upkie_ppo_explained_variance, row.n, ptr(shards[r][0]), ptr(shards[r][1]), phase, ptr(slots), world, ptr(slots[r]), None)
        launch(lb.upkie_ppo_explained_variance, row.n, ptr(ret), ptr(val), 2, ptr(slots), world, None, ptr(out))
        assert not torch.isnan(slots).any() and float(out[1]) == -7.0
        worst[f"world {world}"] = S.ev_ratio(float(out[0]), row, world)
        if world == 1:
            assert _same_bytes(out[0], outs[0, 0]), "one shard gives the bits of phase -1"
    want, _ = S.ev_twin(row)
    print(f"matrix explained variance {row.n} {row.kind}: {float(outs[0, 0])!r} (twin {want!r}); worst error / bound: "
          + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


# ================================================================ launch B and launch C
def _config():
    cfg = abi.UpkiePpoConfig()
    cfg.clip_range, cfg.clip_range_vf, cfg.obs_normalized = 0.2, 0.0, 0
    cfg.ent_coef, cfg.vf_coef, cfg.max_grad_norm = (float(S.CFG32[k]) for k in ("ent_coef", "vf_coef", "max_grad_norm"))
    cfg.adam_beta1, cfg.adam_beta2, cfg.adam_eps = (float(S.CFG32[k]) for k in ("beta1", "beta2", "eps"))
    return cfg


WORKSPACE_GUARD = 64  # bytes behind the workspace that must stay as they were


class _Apply:
    """A row's device state and `upkie_ppo_minibatch_apply` (or, with a control block, `..._apply_controlled`) on it."""

    def __init__(self, row, api, controlled=False):
        self.row, (self.lb, self.launch) = row, api
        self.p, self.inp = S.fold_plan(row), S.fold_inputs(row)
        self.shape, self.cfg = S.fold_shape(row), _config()
        assert int(self.lb.upkie_ppo_workspace_bytes(C.byref(self.shape), S.FOLD_MAX_MINIBATCH)) == self.p["workspace_bytes"]
        assert int(self.lb.upkie_ppo_slot_bytes(C.byref(self.shape))) == 4 * self.p["slot_words"]
        self.slots = _dev(self.inp.slots)
        self.workspace = torch.zeros(self.p["workspace_bytes"] + WORKSPACE_GUARD, dtype=torch.uint8, device=DEV)
        self.control = torch.zeros(abi.PPO_CTRL_WORDS if controlled else 2, dtype=F64, device=DEV)
        self.controlled = controlled
        self.stats = torch.empty((S.FOLD_APPLIES + 2, 8), dtype=torch.float32, device=DEV)
        self.initial = tuple(_dev(a.copy()) for a in (self.inp.packed, self.inp.m, self.inp.v))
        self.packed, self.m, self.v = (torch.empty_like(a) for a in self.initial)
        self.reset()

    def reset(self):
        """The row's state again, in the same tensors (a captured graph holds their addresses)."""
        for dst, src in zip((self.packed, self.m, self.v), self.initial):
            dst.copy_(src)
        self.control.zero_()
        self.control[0] = S.LR
        self.workspace.zero_()
        self.workspace[self.p["workspace_bytes"]:] = 0xAB
        self.stats.fill_(float("nan"))

    def apply(self, k, slots=None, row_of_stats=None, minibatch_start=0):
        slots = self.slots[k] if slots is None else slots
        head = (C.byref(self.shape), C.byref(self.cfg)) + ((minibatch_start,) if self.controlled else ())
        fn = self.lb.upkie_ppo_minibatch_apply_controlled if self.controlled else self.lb.upkie_ppo_minibatch_apply
        self.launch(fn, *head, S.fold_count(self.row), S.FOLD_MAX_MINIBATCH, ptr(slots), self.row.world, ptr(self.packed), ptr(self.m), ptr(self.v),
                    ptr(self.control), ptr(self.workspace), ptr(self.stats[k if row_of_stats is None else row_of_stats]))

    def state(self):
        return tuple(t.cpu().numpy() for t in (self.packed, self.m, self.v)) + (int(self.control[1]),)

    def gradient(self):
        at, words = self.p["grad_at"], self.p["train_words"]
        return self.workspace[at:at + 4 * words].view(torch.float32).cpu().numpy()

    def check_workspace(self):
        assert int(self.workspace[:4].view(torch.int32)) == 0, "the ticket is back at zero"
        assert (self.workspace[self.p["workspace_bytes"]:] == 0xAB).all(), "the bytes behind the workspace are untouched"

    def bits(self):
        return [t.clone() for t in (self.packed, self.m, self.v, self.control, self.stats, self.workspace[self.p["grad_at"]:])]


def _three_applies(state, check=True):
    worst = {}
    before = state.state() if check else None  # (nothing is read back inside a capture)
    for k in range(S.FOLD_APPLIES):
        state.apply(k)
        if not check:
            continue
        after = state.state()
        row_of_stats = state.stats[k].cpu().numpy()
        assert np.isnan(row_of_stats[7]), "the word behind the statistics row is untouched"
        ratios = S.apply_ratios(state.row, k, before, state.gradient(), row_of_stats[:7], after)
        state.check_workspace()
        assert max(ratios.values()) <= 1.0, (k, ratios)
        for name, value in ratios.items():
            worst[name] = max(worst.get(name, 0.0), value)
        before = after
    return worst


@pytest.mark.parametrize("row", S.FOLD_ROWS, ids=S.FOLD_IDS)
def test_fold_and_adam_at_every_shape_and_world(row, api):
    """Behind each of three consecutive applies (t = 1, 2, 3 from non-zero m and v; the first and the third above
    max_grad_norm, the second below): the workspace's gradient bit-equal to the sequential fp32 sum in slot order,
    stats[0..6], t, m, v and the trainable words within their bounds of `adam_step` fed that gradient and the device's own
    state before the apply, padding words exactly 0, the fixed words and everything before train_off bit-unchanged, the
    ticket back at 0."""
    state = _Apply(row, api)
    worst = _three_applies(state)
    p = state.p
    print(f"matrix apply {S.FOLD_IDS[S.FOLD_ROWS.index(row)]} ({p['train_words']} words, {p['fold_blocks']} blocks, body {p['body']} tail {p['tail']}): "
          "gradient bit-equal; worst error / bound: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items() if k in ("stats", "m", "v", "delta")))


def test_three_applies_replayed_from_a_graph(api):
    """The row with a body and a one-slot tail: its three applies eagerly and from one captured graph, equal bits."""
    row = next(r for r in S.FOLD_ROWS if (r.obs_dim, r.world) == S.GRAPHED_FOLD_ROW)
    state = _Apply(row, api)
    _three_applies(state)
    torch.cuda.synchronize()
    eager = state.bits()
    state.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _three_applies(state, check=False)
    state.reset()  # (a capture launches nothing; the replay starts from the row's state either way)
    graph.replay()
    torch.cuda.synchronize()
    state.check_workspace()
    for a, b in zip(eager, state.bits()):
        assert _same_bytes(a, b)
    assert int(state.control[1]) == S.FOLD_APPLIES


def test_controlled_form_stops_skips_and_counts(api):
    """`upkie_ppo_minibatch_apply_controlled` with approx_kl chosen through the slots' loss sums: below 1.5 target_kl it
    steps and counts; above, it writes the row, sets STOPPED, bumps MINIBATCHES_RUN and leaves t, m, v and packed as they
    were; the next apply writes a NaN row and changes nothing; after `upkie_ppo_update_begin` the next apply steps; N_UPDATES
    rises only at minibatch_start == 0. The applies that step are the row's three in order, so the bounds of
    `adam_bounds` (t = 1, 2, 3 from the row's state) are theirs."""
    row = next(r for r in S.FOLD_ROWS if (r.obs_dim, r.world) == S.CONTROLLED_FOLD_ROW)
    state = _Apply(row, api, controlled=True)
    lb, launch, p, count = state.lb, state.launch, state.p, S.fold_count(row)
    target_kl = 0.01
    launch(lb.upkie_ppo_control_set, ptr(state.control), S.LR, 0.2, 0.0, target_kl)

    def slots_with_kl(k, kl):
        sums = S.fold_inputs(row).sums[k].copy()
        sums[:, 2] = kl * count / row.world
        host = S.fold_inputs(row).slots[k].copy()
        for r in range(row.world):
            host[r, p["slot_stats_at"]:].view(np.float64)[:] = sums[r]
        return _dev(host), sums

    def control():
        c = state.control.cpu().numpy()
        return {k: c[getattr(abi, "PPO_CTRL_" + k)] for k in ("T", "STOPPED", "N_UPDATES", "MINIBATCHES_RUN", "LR", "TARGET_KL")}

    def run(k, kl, stats_row, start, stepped):
        slots, sums = slots_with_kl(k, kl)
        before = state.state()
        state.apply(k, slots=slots, row_of_stats=stats_row, minibatch_start=start)
        got = state.stats[stats_row].cpu().numpy()
        assert np.isnan(got[7])
        ratios = S.apply_ratios(row, k, before, state.gradient(), got[:7], state.state(), sums=sums, stepped=stepped)
        state.check_workspace()
        assert max(ratios.values()) <= 1.0, (stats_row, ratios)
        return got

    assert control() == {"T": 0, "STOPPED": 0, "N_UPDATES": 0, "MINIBATCHES_RUN": 0, "LR": S.LR, "TARGET_KL": target_kl}
    run(0, 0.5 * target_kl, 0, 0, True)
    assert control() == {"T": 1, "STOPPED": 0, "N_UPDATES": 1, "MINIBATCHES_RUN": 1, "LR": S.LR, "TARGET_KL": target_kl}
    run(1, 1.4 * target_kl, 1, 64, True)  # (below 1.5 target_kl: it steps; not the first minibatch: no new epoch)
    assert control() == {"T": 2, "STOPPED": 0, "N_UPDATES": 1, "MINIBATCHES_RUN": 2, "LR": S.LR, "TARGET_KL": target_kl}
    got = run(2, 1.6 * target_kl, 2, 128, False)
    assert abs(float(got[4]) - 1.6 * target_kl) < 1e-7 and control() == {"T": 2, "STOPPED": 1, "N_UPDATES": 1, "MINIBATCHES_RUN": 3, "LR": S.LR,
                                                                       "TARGET_KL": target_kl}
    frozen = state.bits()
    state.stats[3].zero_()
    state.apply(0, row_of_stats=3, minibatch_start=0)  # (even at minibatch_start 0: no epoch is entered after a stop)
    torch.cuda.synchronize()
    assert torch.isnan(state.stats[3, :7]).all() and float(state.stats[3, 7]) == 0.0, "a NaN row, and the word behind it untouched"
    state.stats[3].copy_(frozen[4][3])
    for a, b in zip(frozen, state.bits()):
        assert _same_bytes(a, b), "an apply after the stop changes nothing: weights, m, v, the control block, the workspace's gradient"
    state.check_workspace()
    launch(lb.upkie_ppo_update_begin, ptr(state.control))
    assert control() == {"T": 2, "STOPPED": 0, "N_UPDATES": 1, "MINIBATCHES_RUN": 0, "LR": S.LR, "TARGET_KL": target_kl}
    run(2, 0.1 * target_kl, 4, 0, True)
    assert control() == {"T": 3, "STOPPED": 0, "N_UPDATES": 2, "MINIBATCHES_RUN": 1, "LR": S.LR, "TARGET_KL": target_kl}
    print(f"matrix controlled apply {S.FOLD_IDS[S.FOLD_ROWS.index(row)]}: stepped twice, stopped at approx_kl {float(got[4]):.6f} > 1.5 x {target_kl}, "
          "skipped with a NaN row, re-armed and stepped; N_UPDATES 2")


# ================================================================ generalized advantage estimation
@pytest.mark.parametrize("row", S.GAE_ROWS, ids=S.GAE_IDS)
def test_gae_at_every_size(row, api):
    lb, launch = api
    rewards, values, starts, last_values, last_dones = (_dev(a) for a in S.gae_inputs(row))
    n, G = row.T * row.N, S.GAE_GUARD
    big = torch.full((2, n + 2 * G), float("nan"), device=DEV)
    adv, ret = big[0, G:G + n], big[1, G:G + n]
    launch(lb.upkie_rollout_gae, row.T, row.N, ptr(rewards), ptr(values), ptr(starts), ptr(last_values), ptr(last_dones), row.gamma, row.lam,
           adv.data_ptr(), ret.data_ptr())
    host = big.cpu().numpy()
    assert np.isnan(host[:, :G]).all() and np.isnan(host[:, G + n:]).all(), "the guards before and after the outputs remain NaN"
    worst = S.gae_ratio(host[0, G:G + n].reshape(row.T, row.N), host[1, G:G + n].reshape(row.T, row.N), row)
    print(f"matrix gae T {row.T} N {row.N} gamma {row.gamma} lambda {row.lam} {row.starts}: worst error / (atol {S.GAE_ATOL} + rtol {S.GAE_RTOL} |x|) "
          f"{worst:.3g}")
    assert worst <= 1.0
