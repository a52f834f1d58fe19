"""Distances between partitions (Context.partition_distances, msc_partition_distances) at m = 16 384 rows and S = 1 024
samples of a planted partition (--kt clusters, every row relabelled uniformly with probability --noise):
  candidates   64 and 1 024 candidates (the first samples) against all the samples: the table of every pair stays in LDS;
  samples      the samples against themselves (b = None: half the pairs are computed, each written twice);
  all-in-one   the one candidate whose rows all land in one cell of every sample's table (the wave-uniform add), apart;
  1024 clusters  1 and 64 candidates of 1 024 clusters: 1 024 x K_sample cells do not fit LDS, the global route;
  estimates    the winner by the exact expected VI (query.expected_loss) beside the winner by the bound
               (ZMatrix.partition_loss's vi_lb, its candidate-independent term put back), among the samples: the exact
               expected VI of both;
  host         query.partition_distances on numpy, the same generator at --host-m rows, --host-cands candidates, beside the
               device on the same data: what the numpy path costs where it finishes.  Nothing is extrapolated.
Device times are device events around the whole call (canonicalisation, the host's wait for the cluster counts, the pair
kernel), the median of --steps warm runs after --warmup.  Prints one JSON line and writes a readable table to --out.

    python tools/bench_distances.py [--steps 3] [--warmup 1] [--out profiles/distances.txt]
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


def case(ctx, a, b, args):
    ts = []
    for it in range(args.warmup + args.steps):
        t = event_ms(lambda: ctx.partition_distances(a, b))
        if it >= args.warmup:
            ts.append(t)
    ms = float(np.median(ts))
    na, nb = int(a.shape[0]), int(a.shape[0] if b is None else b.shape[0])
    got = ctx.partition_distances(a, b)
    return {"na": na, "nb": nb, "pairs": na * nb, "ms": round(ms, 3), "us_per_pair": round(1e3 * ms / (na * nb), 4),
            "clusters_a_max": int(got[4].max()), "clusters_b_max": int(got[7].max()), "last_kernel": ctx.last_kernel("zmatrix")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=16384)
    ap.add_argument("--S", type=int, default=1024)
    ap.add_argument("--kt", type=int, default=20)
    ap.add_argument("--noise", type=float, default=0.2)
    ap.add_argument("--host-m", type=int, default=2048)
    ap.add_argument("--host-cands", type=int, default=16)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distances.txt"))
    args = ap.parse_args()
    ctx = common_amd.Context(0)
    dev = ctx.torch_device
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    m, S = args.m, args.S
    out = {"m": m, "S": S, "kt": args.kt, "noise": args.noise, "cases": {}}
    A = planted(g, dev, m, S, args.kt, args.noise)
    out["cases"]["candidates_64"] = case(ctx, A[:64], A, args)
    out["cases"]["candidates_1024"] = case(ctx, A[:1024], A, args)
    out["cases"]["samples_themselves"] = case(ctx, A, None, args)
    out["cases"]["all_in_one"] = case(ctx, torch.zeros((1, m), dtype=torch.int32, device=dev), A, args)
    many = (torch.arange(m, dtype=torch.int32, device=dev) % 1024).repeat(64, 1)
    many = torch.stack([many[i].roll(i) for i in range(64)]).contiguous()
    out["cases"]["clusters_1024_x1"] = case(ctx, many[:1], A, args)
    out["cases"]["clusters_1024_x64"] = case(ctx, many, A, args)
    # the two estimates among the samples
    exact = query.expected_loss(A, ctx=ctx).vi.cpu().numpy()
    zm = common_amd.ZMatrix(ctx, m, args.kt + 2)
    zm.add(A)
    bound = zm.partition_loss(A)[1].cpu().numpy()
    zm.close()
    # vi_lb leaves out the bound's candidate-independent term (1 / (m S)) sum_s nlogn_s: put back, the two compare
    term = float(ctx.partition_distances(A[:1], A)[6].cpu().numpy().mean()) / m
    bound = bound + term
    ie, ib = int(np.argmin(exact)), int(np.argmin(bound))
    out["estimates"] = {"exact_winner": ie, "bound_winner": ib, "exact_vi_of_exact_winner": float(exact[ie]),
                        "exact_vi_of_bound_winner": float(exact[ib]), "vi_lb_of_exact_winner": float(bound[ie]),
                        "vi_lb_of_bound_winner": float(bound[ib]), "lb_term": term, "exact_minus_lb_min": float((exact - bound).min()),
                        "exact_minus_lb_max": float((exact - bound).max())}
    # the numpy path where it finishes, and the device beside it on the same data
    hm, hc = args.host_m, args.host_cands
    B = planted(g, dev, hm, S, args.kt, args.noise)
    d = case(ctx, B[:hc], B, args)
    got = query.partition_distances(B[:hc], B, ctx=ctx)
    Bh = B.cpu().numpy()
    t = time.perf_counter()
    want = query.partition_distances(Bh[:hc], Bh)
    host_s = time.perf_counter() - t
    out["host"] = {"m": hm, "na": hc, "nb": S, "numpy_ms": round(host_s * 1e3, 1),
                   "numpy_us_per_pair": round(host_s * 1e6 / (hc * S), 2), "device_ms": d["ms"],
                   "device_us_per_pair": d["us_per_pair"],
                   "binder_equal": bool(np.array_equal(got.binder.cpu().numpy(), want.binder)),
                   "vi_max_abs_diff": float(np.abs(got.vi.cpu().numpy() - want.vi).max())}
    print(json.dumps(out))
    lines = ["distances between partitions: m = %d, S = %d, planted %d clusters, noise %.2f" % (m, S, args.kt, args.noise),
             "%-20s %6s %6s %9s %12s %12s %8s %8s  %s" % ("case", "na", "nb", "pairs", "call", "per pair", "K_a max",
                                                          "K_b max", "pair kernel (the last launched)")]
    for name, c in out["cases"].items():
        lines.append("%-20s %6d %6d %9d %10.3fms %10.4fus %8d %8d  %s" % (name, c["na"], c["nb"], c["pairs"], c["ms"],
                                                                         c["us_per_pair"], c["clusters_a_max"],
                                                                         c["clusters_b_max"], c["last_kernel"]))
    e = out["estimates"]
    lines.append("estimates among the samples: exact-VI winner %d with expected VI %.6f bits (vi_lb %.6f); bound winner %d with "
                 "expected VI %.6f bits (vi_lb %.6f); vi_lb with its candidate-independent term, %.6f, put back; exact - vi_lb "
                 "over the samples: %.4f .. %.4f"
                 % (e["exact_winner"], e["exact_vi_of_exact_winner"], e["vi_lb_of_exact_winner"], e["bound_winner"],
                    e["exact_vi_of_bound_winner"], e["vi_lb_of_bound_winner"], e["lb_term"], e["exact_minus_lb_min"],
                    e["exact_minus_lb_max"]))
    h = out["host"]
    lines.append("host numpy at m = %d, %d x %d pairs: %.1f ms (%.2f us a pair); the device on the same data: %.3f ms (%.4f us a "
                 "pair); binder equal: %s, vi within %.3g" % (h["m"], h["na"], h["nb"], h["numpy_ms"], h["numpy_us_per_pair"],
                                                             h["device_ms"], h["device_us_per_pair"], h["binder_equal"],
                                                             h["vi_max_abs_diff"]))
    lines.append(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
