"""Greedy refinement of point-estimate partitions (ZMatrix.partition_refine, msc_zmatrix_partition_refine) at m = 16 384
rows and S = 1 024 samples of a planted partition (--kt clusters, every row relabelled uniformly with probability --noise):
  samples      the 1, 64 and 256 samples of lowest binder_num as starts: the time of a call that runs no sweep (dense copy,
               gather, the starts' losses, ids, numbering), of one that runs exactly one sweep, and of one that runs to
               convergence; the sweeps that took (a start that has converged returns at once, so late sweeps are cheap: the
               first sweep is the one in which every start works); binder_num of the best start before, of the best
               result after, against the best sample;
  all-in-one   the one start whose columns all land in one bin, measured apart;
  host         query.refine_partition on numpy, the same generator at --host-m rows, one start (the best sample), beside
               the device on the same data: what the numpy path costs where it finishes.  Nothing is extrapolated.
Device times are device events around the whole call on an accumulator whose counts are up to date, the median of --steps
runs after --warmup.  Prints one JSON line and writes a readable table to --out.

    python tools/bench_refine.py [--steps 3] [--warmup 1] [--out profiles/refine.txt]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import common_amd  # noqa: E402
from common_amd import query  # noqa: E402


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def planted(g, dev, m, S, Kt, noise):
    truth = torch.randint(0, Kt, (m,), dtype=torch.int32, device=dev, generator=g)
    A = truth.repeat(S, 1)
    flip = torch.rand((S, m), device=dev, generator=g) < noise
    other = torch.randint(0, Kt + 2, (S, m), dtype=torch.int32, device=dev, generator=g)
    return torch.where(flip, other, A).contiguous()


def timed(zm, starts, max_sweeps, steps, warmup):
    ts = []
    for it in range(warmup + steps):
        t = event_ms(lambda: zm.partition_refine(starts, max_sweeps=max_sweeps))
        if it >= warmup:
            ts.append(t)
    return float(np.median(ts))


def case(ctx, zm, starts, best_sample, args):
    t0 = timed(zm, starts, 0, args.steps, args.warmup)
    t1 = timed(zm, starts, 1, args.steps, args.warmup)
    tn = timed(zm, starts, args.max_sweeps, args.steps, args.warmup)
    name = ctx.last_kernel("zmatrix")
    before = zm.partition_refine(starts, max_sweeps=0)[1]
    labels, after, sweeps, moves = zm.partition_refine(starts, max_sweeps=args.max_sweeps)
    check = zm.partition_loss(labels)[0] if zm._rows is None else after
    sw = sweeps.cpu().numpy()
    return {
        "starts": int(starts.shape[0]),
        "no_sweep_ms": round(t0, 3),
        "first_sweep_ms": round(t1 - t0, 3),
        "to_convergence_ms": round(tn, 3),
        "sweeps_min_median_max": [int(sw.min()), int(np.median(sw)), int(sw.max())],
        "converged": bool((sw < args.max_sweeps).all()),
        "ms_per_sweep_mean": round((tn - t0) / max(1, int(sw.max())), 3),
        "moves_max": int(moves.max()),
        "binder_num_best_start": int(before.min()),
        "binder_num_best_refined": int(after.min()),
        "binder_num_best_sample": int(best_sample),
        "refined_over_best_sample": round(float(after.min()) / float(best_sample), 4),
        "binder_num_equals_loss_kernel": bool(torch.equal(check, after)),
        "last_kernel": name,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=16384)
    ap.add_argument("--S", type=int, default=1024)
    ap.add_argument("--kt", type=int, default=20)
    ap.add_argument("--noise", type=float, default=0.2)
    ap.add_argument("--max-sweeps", type=int, default=20)
    ap.add_argument("--host-m", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine.txt"))
    args = ap.parse_args()
    ctx = common_amd.Context(0)
    dev = ctx.torch_device
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    m, S, K = args.m, args.S, args.kt + 2
    out = {"m": m, "S": S, "kt": args.kt, "noise": args.noise, "max_sweeps": args.max_sweeps, "cases": {}}
    A = planted(g, dev, m, S, args.kt, args.noise)
    zm = common_amd.ZMatrix(ctx, m, K)
    zm.add(A)
    losses = zm.partition_loss(A)[0]
    rank = torch.argsort(losses, stable=True)
    best = int(losses.min())
    for ns in (1, 64, 256):
        out["cases"]["samples_%d" % ns] = case(ctx, zm, A[rank[:ns]].contiguous(), best, args)
    one = torch.zeros((1, m), dtype=torch.int32, device=dev)
    out["cases"]["all_in_one"] = case(ctx, zm, one, best, args)
    zm.close()
    # the numpy path where it finishes, and the device beside it on the same data
    hm = args.host_m
    B = planted(g, dev, hm, S, args.kt, args.noise)
    zh = common_amd.ZMatrix(ctx, hm, K)
    zh.add(B)
    hl = zh.partition_loss(B)[0]
    start = B[int(torch.argmin(hl))][None].contiguous()
    d = case(ctx, zh, start, int(hl.min()), args)
    got = zh.partition_refine(start, max_sweeps=args.max_sweeps)
    Bh, sh = B.cpu().numpy(), start.cpu().numpy()
    C = query._host_counts_of(list(Bh))[1]
    t = time.perf_counter()
    want = query._refine_host(C, sh, args.max_sweeps, min(hm, 1024), None)
    host_s = time.perf_counter() - t
    same = all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(got, want))
    out["host"] = {"m": hm, "starts": 1, "numpy_refine_ms": round(host_s * 1e3, 1), "sweeps": int(want[2][0]),
                   "numpy_ms_per_sweep": round(host_s * 1e3 / max(1, int(want[2][0])), 1),
                   "device_to_convergence_ms": d["to_convergence_ms"], "device_ms_per_sweep_mean": d["ms_per_sweep_mean"],
                   "device_equals_numpy": bool(same), "counts_excluded_from_both": True}
    zh.close()
    print(json.dumps(out))
    lines = ["greedy refinement under Binder's loss: m = %d, S = %d, planted %d clusters, noise %.2f, at most %d sweeps"
             % (m, S, args.kt, args.noise, args.max_sweeps),
             "%-12s %6s %10s %12s %12s %10s %9s %16s %16s %16s" % ("case", "starts", "no sweep", "first sweep", "to converge",
                                                                    "ms/sweep", "sweeps", "best start", "best refined",
                                                                    "best sample")]
    for name, c in out["cases"].items():
        lines.append("%-12s %6d %8.3fms %10.3fms %10.3fms %10.3f %9s %16d %16d %16d"
                     % (name, c["starts"], c["no_sweep_ms"], c["first_sweep_ms"], c["to_convergence_ms"],
                        c["ms_per_sweep_mean"], "/".join(str(v) for v in c["sweeps_min_median_max"]),
                        c["binder_num_best_start"], c["binder_num_best_refined"], c["binder_num_best_sample"]))
    h = out["host"]
    lines.append("host numpy at m = %d, one start: %.1f ms for %d sweeps (%.1f ms a sweep); the device on the same data: %.3f ms "
                 "(%.3f ms a sweep); equal outputs: %s" % (h["m"], h["numpy_refine_ms"], h["sweeps"], h["numpy_ms_per_sweep"],
                                                         h["device_to_convergence_ms"], h["device_ms_per_sweep_mean"],
                                                         h["device_equals_numpy"]))
    lines.append(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
