"""Run under `python -m torch.distributed.run --nproc-per-node 2` on a GPU box (tests/test_ppo_learn_gpu.py; not a test
file itself): two gloo ranks sharing cuda:0 train with target_kl as one learner on the union of their samples. Every
rank must stop at the same minibatch with the same bits, and at the minibatch where one controlled learner on the union
buffer stops. Every rank writes its findings as JSON to `<out>.<rank>`."""

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from tests import ppo_learn_reference as L  # noqa: E402
from tests.ppo_distributed_worker import T, _gather, _restore, _setup, _state, _union_buffer, _union_perm  # noqa: E402
from upkie_amd.distributed import init_distributed  # noqa: E402
from upkie_amd.ppo import PpoTrainer  # noqa: E402


def run(group, rank):
    out = {}
    case = (500, 5, [40, 24], 3, "tanh")
    N, lr, E = case[0], 1e-2, 3
    pol, buf = _setup(case, 10, 20 + rank, first=True)
    mb = (T * N + 3) // 4
    kw = dict(lr=lr, n_epochs=E, batch_size=mb, seed=11)
    tr = PpoTrainer(pol, process_group=group, controlled=True, **kw)
    tr.broadcast_parameters(0)
    s0 = _state(pol, tr)
    tr.prepare(buf)
    perms = [tr.perm[e].clone() for e in range(E)]
    # one learner on the union (every rank computes it: both hold the same union buffer), first without a stop
    ubuf = _union_buffer(buf, group, case)
    all_perms = [[p.long().cpu() for p in _gather(perms[e], group)] for e in range(E)]
    union = PpoTrainer(pol, lr=lr, n_epochs=E, batch_size=2 * mb, seed=11, controlled=True)
    union.prepare(ubuf)
    for e in range(E):
        union.perm[e].copy_(_union_perm(all_perms[e], N, mb).to(torch.int32))
    kls = union.update(ubuf, sync=False).double().cpu().numpy().reshape(-1, 7)[:, 4]
    chosen = L.choose_target_kl(kls)
    out["chosen"], out["union_kls"] = chosen is not None, [float(x) for x in kls]
    if chosen is None:
        return out
    box = [chosen]
    dist.broadcast_object_list(box, src=0, group=group)
    target_kl, k = box[0]
    out["expected"] = list(divmod(int(k), 4))
    _restore(pol, union, s0)
    union.control[6] = 0.0  # n_updates: count this update alone
    union.set_target_kl(target_kl)
    ustats = union.update(ubuf, sync=False).double().cpu().numpy().reshape(-1, 7)
    urec = union.log()
    out["union_stopped_at"] = list(urec["early_stopped_at"]) if urec["early_stopped_at"] else None
    out["union_t"], out["union_n_updates"] = union.state_dict()["t"], urec["n_updates"]
    # the two ranks
    _restore(pol, tr, s0)
    tr.set_target_kl(target_kl)
    stats = tr.update(buf, sync=False).clone()
    rec = tr.log()  # (collective: the explained variance runs over both ranks' samples)
    torch.cuda.synchronize()
    after = _state(pol, tr)
    out["ranks_bit_equal"] = [bool(torch.equal(*_gather(t, group))) for t in after + [tr.control]]
    rows = stats.double().cpu().numpy().reshape(-1, 7)
    both = _gather(torch.nan_to_num(stats, nan=-1.0), group)
    out["ranks_bit_equal"].append(bool(torch.equal(*both)))
    out["stopped_at"] = list(rec["early_stopped_at"]) if rec["early_stopped_at"] else None
    out["t"], out["n_updates"] = tr.state_dict()["t"], rec["n_updates"]
    out["nan_after"] = bool(np.isnan(rows[k + 1:]).all() and not np.isnan(rows[:k + 1]).any())
    cols = [0, 1, 2, 3, 6]
    out["rows_close"] = bool(np.isclose(rows[:k + 1][:, cols], ustats[:k + 1][:, cols], rtol=2e-3, atol=2e-5).all())
    want_ev = L.explained_variance(ubuf.values.double().cpu().numpy(), ubuf.returns.double().cpu().numpy())
    out["explained_variance_error"] = abs(rec["explained_variance"] - want_ev)
    return out


def main():
    out_path = sys.argv[1]
    rank, _, _ = init_distributed(backend="gloo")
    torch.cuda.set_device(0)
    group = dist.group.WORLD
    try:
        result = run(group, rank)
    finally:
        dist.barrier()
    with open(f"{out_path}.{rank}", "w") as f:
        json.dump(result, f)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
