"""Greedy refinement under the exact expected variation of information (Context.partition_refine_vi,
msc_partition_refine_vi) at m = 16 384 rows and S = 1 024 samples of a planted partition (--kt clusters, every row
relabelled uniformly with probability --noise; the generator of tools/bench_refine.py):
  samples      the 1, 64 and 256 samples of lowest exact expected VI as starts: the time of a call that runs no sweep (the
               starts' ids and numbering alone), of one that runs exactly one sweep (the samples' ids, the rows' stretch
               indices, the counting of the cells, one sweep), and of one that runs to convergence; the sweeps that took (a
               start that has converged returns at once); the exact float64 expected VI of the best sample, the best start
               and the best result; the 256 once more with max_clusters = 64, which lets one chunk hold them all;
  host         query._refine_vi_host on numpy, the same generator at --host-m rows, one start (the best sample), with
               max_clusters = --host-clusters on both sides (the numpy path reads S x max_clusters cells a row), beside
               the device on the same data.  Nothing is extrapolated.
Device times are device events around whole warm calls, the median of --steps runs after --warmup.  Prints one JSON line
and writes a readable table to --out.

    python tools/bench_refine_vi.py [--steps 3] [--warmup 1] [--out profiles/refine_vi.txt]
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


def timed(ctx, A, starts, max_sweeps, max_clusters, steps, warmup):
    ts = []
    for it in range(warmup + steps):
        t = event_ms(lambda: ctx.partition_refine_vi(A, starts, max_sweeps=max_sweeps, max_clusters=max_clusters))
        if it >= warmup:
            ts.append(t)
    return float(np.median(ts))


def case(ctx, A, starts, vi_best_sample, args, max_clusters=None):
    t0 = timed(ctx, A, starts, 0, max_clusters, args.steps, args.warmup)
    t1 = timed(ctx, A, starts, 1, max_clusters, args.steps, args.warmup)
    tn = timed(ctx, A, starts, args.max_sweeps, max_clusters, args.steps, args.warmup)
    name = ctx.last_kernel("zmatrix")
    labels, decrease, sweeps, moves = ctx.partition_refine_vi(A, starts, max_sweeps=args.max_sweeps, max_clusters=max_clusters)
    ctx.synchronize()
    S, m = int(A.shape[0]), int(A.shape[1])
    vi0 = query.expected_loss(A, starts, ctx=ctx).vi.cpu().numpy()
    vi1 = query.expected_loss(A, labels, ctx=ctx).vi.cpu().numpy()
    sw = sweeps.cpu().numpy()
    off = np.abs((vi0 - vi1) - decrease.cpu().numpy() / (float(S) * m * 2.0 ** 24)).max()
    return {
        "starts": int(starts.shape[0]),
        "no_sweep_ms": round(t0, 3),
        "first_sweep_ms": round(t1, 3),
        "to_convergence_ms": round(tn, 3),
        "sweeps_min_median_max": [int(sw.min()), int(np.median(sw)), int(sw.max())],
        "converged": bool((sw < args.max_sweeps).all()),
        "ms_per_sweep_mean": round((tn - t0) / max(1, int(sw.max())), 3),
        "us_per_row_first_sweep": round((t1 - t0) * 1e3 / m, 3),
        "moves_max": int(moves.max()),
        "clusters_of_best_refined": int(labels[int(np.argmin(vi1))].max()) + 1,
        "vi_best_sample": float(vi_best_sample),
        "vi_best_start": float(vi0.min()),
        "vi_best_refined": float(vi1.min()),
        "decrease_against_float64_vi_bits": float(off),
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
    ap.add_argument("--host-clusters", type=int, default=32)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_vi.txt"))
    args = ap.parse_args()
    ctx = common_amd.Context(0)
    dev = ctx.torch_device
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    m, S = args.m, args.S
    out = {"m": m, "S": S, "kt": args.kt, "noise": args.noise, "max_sweeps": args.max_sweeps, "cases": {}}
    A = planted(g, dev, m, S, args.kt, args.noise)
    vi = query.expected_loss(A, ctx=ctx).vi
    rank = torch.argsort(vi, stable=True)
    best = float(vi.min())
    for ns in (1, 64, 256):
        out["cases"]["samples_%d" % ns] = case(ctx, A, A[rank[:ns]].contiguous(), best, args)
    # the same 256 starts with an id capacity of 64: their cells (2 bytes x sum L_s x 64 a start) fit the default budget in
    # one chunk, where max_clusters = 1024 takes them 46 at a time
    out["cases"]["256_cap_64"] = case(ctx, A, A[rank[:256]].contiguous(), best, args, max_clusters=64)
    # the numpy path where it finishes, and the device beside it on the same data
    hm, hk = args.host_m, args.host_clusters
    B = planted(g, dev, hm, S, args.kt, args.noise)
    hv = query.expected_loss(B, ctx=ctx).vi
    start = B[int(torch.argmin(hv))][None].contiguous()
    d = case(ctx, B, start, float(hv.min()), args, max_clusters=hk)
    got = ctx.partition_refine_vi(B, start, max_sweeps=args.max_sweeps, max_clusters=hk)
    ctx.synchronize()
    Bh, sh = B.cpu().numpy(), start.cpu().numpy()
    t = time.perf_counter()
    want = query._refine_vi_host(Bh, sh, args.max_sweeps, hk, None)
    host_s = time.perf_counter() - t
    same = all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(got, want))
    out["host"] = {"m": hm, "starts": 1, "max_clusters": hk, "numpy_refine_ms": round(host_s * 1e3, 1),
                   "sweeps": int(want[2][0]), "numpy_ms_per_sweep": round(host_s * 1e3 / max(1, int(want[2][0])), 1),
                   "device_to_convergence_ms": d["to_convergence_ms"], "device_ms_per_sweep_mean": d["ms_per_sweep_mean"],
                   "device_equals_numpy": bool(same)}
    print(json.dumps(out))
    lines = ["greedy refinement under the exact expected VI: m = %d, S = %d, planted %d clusters, noise %.2f, at most %d sweeps"
             % (m, S, args.kt, args.noise, args.max_sweeps),
             "%-12s %6s %10s %12s %12s %10s %8s %9s %12s %12s %12s" % ("case", "starts", "no sweep", "one sweep", "to converge",
                                                                       "ms/sweep", "us/row", "sweeps", "best sample",
                                                                       "best start", "best refined")]
    for name, c in out["cases"].items():
        lines.append("%-12s %6d %8.3fms %10.3fms %10.3fms %10.3f %8.3f %9s %12.6f %12.6f %12.6f"
                     % (name, c["starts"], c["no_sweep_ms"], c["first_sweep_ms"], c["to_convergence_ms"],
                        c["ms_per_sweep_mean"], c["us_per_row_first_sweep"],
                        "/".join(str(v) for v in c["sweeps_min_median_max"]), c["vi_best_sample"], c["vi_best_start"],
                        c["vi_best_refined"]))
    h = out["host"]
    lines.append("host numpy at m = %d, one start, max_clusters = %d: %.1f ms for %d sweeps (%.1f ms a sweep); the device on the "
                 "same data: %.3f ms (%.3f ms a sweep); equal outputs: %s"
                 % (h["m"], h["max_clusters"], h["numpy_refine_ms"], h["sweeps"], h["numpy_ms_per_sweep"],
                    h["device_to_convergence_ms"], h["device_ms_per_sweep_mean"], h["device_equals_numpy"]))
    lines.append(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
