"""What the control block of the PPO update (target_kl, schedules: upkie_amd.ppo.PpoTrainer, csrc/ppo.hpp) costs, at obs
4, [64, 64] tanh towers, act 1, event-timed medians, one JSON line per measurement:

  minibatch: one 131072-sample minibatch update replayed from a hipGraph, with the present entry points (`plain`) and
    with the controlled ones (`controlled`). ``--parent-library PATH`` adds the same `plain` measurement on another build
    of libupkie_hip.so (the parent commit's), every variant in a child process of its own, the variants interleaved over
    ``--rounds`` rounds; the spread of a variant is the range of its medians over the rounds.
  stop: a graphed 10 x 4 update of 4 x 32768 samples that stops at the first minibatch of epoch 2 against the full one
    (the skipped minibatches still cost three launches each, which return at once).
  explained_variance: the one-block reduction at 128 x 4096 samples against the advantage-statistics launch over the
    same count (4 minibatches, and 1 minibatch: one block, the same shape of work)."""
import argparse
import json
import os
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_ppo_update import emit, graphed, setup, timed  # noqa: E402

from upkie_amd.ppo import PpoTrainer  # noqa: E402

SAMPLES = 131072


def commit():
    try:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        return subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True, cwd=root).stdout.strip() or None
    except OSError:
        return None


def minibatch(variant, reps):
    pol, _, _, _, buf = setup(32, SAMPLES // 32, 64)
    tr = PpoTrainer(pol, n_epochs=1, batch_size=SAMPLES, controlled=True, target_kl=1e9) if variant == "controlled" else \
        PpoTrainer(pol, n_epochs=1, batch_size=SAMPLES)
    tr.prepare(buf)
    return timed(graphed(lambda: tr.update(buf, sync=False)), reps)


def stop(reps, out, meta):
    pol, _, _, _, buf = setup(32, 4096, 64)
    tr = PpoTrainer(pol, lr=1e-2, n_epochs=10, batch_size=32768, controlled=True)  # (lr large enough that approx_kl grows)
    tr.prepare(buf)
    state = [t.clone() for t in (pol.packed, tr.m, tr.v, tr.control)]
    replay = graphed(lambda: tr.update(buf, sync=False))

    def run():
        for dst, src in zip((pol.packed, tr.m, tr.v, tr.control), state):
            dst.copy_(src)
        replay()

    def restore_only():
        for dst, src in zip((pol.packed, tr.m, tr.v, tr.control), state):
            dst.copy_(src)

    base = timed(restore_only, reps)
    full = timed(run, reps)
    kls = tr.stats[:, :, 4].double().cpu().numpy().reshape(-1)
    # a threshold between the first epoch's approx_kl and epoch 2's first: the update stops at (1, 0); when approx_kl did not
    # grow over the first epoch, one below the first minibatch's: it stops at (0, 0) and skips 39 minibatches
    target = float(0.5 * (kls[:4].max() + kls[4]) / 1.5) if kls[4] > kls[:4].max() else float(kls[0] / 3.0)
    rec = dict(meta, what="stop", shape="10 epochs x 4 minibatches of 32768, [64, 64]", full_us=full["median_us"] - base["median_us"],
               approx_kl_first_five=[float(x) for x in kls[:5]])
    if target > 0.0:
        tr.set_target_kl(target)
        state[3] = tr.control.clone()
        stopped = timed(run, reps)
        at = tr.log()["early_stopped_at"]
        rec.update(stopped_us=stopped["median_us"] - base["median_us"], stopped_at=at, ratio=(stopped["median_us"] - base["median_us"]) /
                   (full["median_us"] - base["median_us"]), skipped_minibatches=40 - (at[0] * 4 + at[1]) - 1 if at else None)
    emit(rec, out)


def explained_variance(reps, out, meta):
    pol, _, _, _, buf = setup(128, 4096, 64)
    total = 128 * 4096
    for mbs in (4, 1):
        tr = PpoTrainer(pol, n_epochs=1, batch_size=total // mbs)
        tr.prepare(buf)
        lb, p = tr._lib, (lambda t: t.data_ptr())
        stream = torch.cuda.current_stream().cuda_stream
        adv = timed(lambda: lb.upkie_ppo_advantage_stats(total, total // mbs, p(tr.perm[0]), p(tr.advantages), 1, p(tr.adv_stats[0]), stream), reps)
        ev = timed(tr.explained_variance, reps)
        emit(dict(meta, what="explained_variance", shape=f"{total} samples", advantage_stats_minibatches=mbs, advantage_stats_us=adv["median_us"],
                  explained_variance_us=ev["median_us"], ratio=ev["median_us"] / adv["median_us"]), out)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-library", default=None, help="libupkie_hip.so of the parent commit, for the A/B of the unused path")
    ap.add_argument("--child", default=None, choices=["plain", "controlled"], help="(internal) measure one variant and print its JSON")
    ap.add_argument("--skip", default="", help="comma-separated parts to skip: minibatch, stop, explained_variance")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child:
        print("RESULT " + json.dumps(minibatch(args.child, args.reps)), flush=True)
        sys.exit(0)
    meta = {"commit": commit(), "device": torch.cuda.get_device_name(0)}
    skip = set(args.skip.split(","))
    if "minibatch" not in skip:
        variants = [("plain", None), ("controlled", None)] + ([("parent_plain", args.parent_library)] if args.parent_library else [])
        medians = {name: [] for name, _ in variants}
        for _ in range(args.rounds):
            for name, library in variants:
                env = dict(os.environ)
                if library:
                    env["UPKIE_HIP_LIBRARY"] = os.path.abspath(library)
                child = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "controlled" if name == "controlled" else "plain",
                                        "--reps", str(args.reps)], capture_output=True, text=True, env=env, timeout=600)
                if child.returncode != 0:
                    sys.exit(f"{name}: the child failed\n{child.stderr[-2000:]}")
                line = [ln for ln in child.stdout.splitlines() if ln.startswith("RESULT ")][-1]
                medians[name].append(json.loads(line[7:])["median_us"])
        for name, xs in medians.items():
            emit(dict(meta, what="minibatch", variant=name, shape=f"{SAMPLES} samples, [64, 64], graph replay", median_us=sorted(xs)[len(xs) // 2],
                      rounds_us=xs, spread_us=max(xs) - min(xs)), args.out)
    if "stop" not in skip:
        stop(args.reps, args.out, meta)
    if "explained_variance" not in skip:
        explained_variance(args.reps, args.out, meta)
