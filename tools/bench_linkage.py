"""Single linkage and block ordering of a device-resident z-matrix (msc_linkage_single) at n = 1 024, 4 096 and 16 384,
each accumulated from S = 64 and S = 1 024 samples of 24 groups (half of the samples with the groups merged in fours):
  device call   Context.linkage_single(z) with both outputs, wall clock (kernel, edge copy, sort, relabelling, leaf walk);
  kernel        the same call with no output asked for: k_linkage_prim and the copy of the 3 (n - 1) edge values, between
                device events on the context's stream; per Prim step beside it, and against the 227 ns of one dependent
                load that hits the Infinity Cache;
  host tail     wall clock of the call with both outputs less wall clock of the call with none;
  host route    what zmatrix_heuristic_block_ordering did with a device tensor before: download, condensed copy of 1 - z,
                scipy's linkage, leaves_list;
median and minimum of --steps runs after --warmup.  The device order is compared with the host route's at every size.
--check-wide adds one exact comparison each at n = 16 400 (32 columns a thread) and n = 32 800 (64), untimed.
Prints one JSON line.

    python tools/bench_linkage.py [--steps 5] [--warmup 1] [--sizes 1024,4096,16384] [--check-wide]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import common_amd  # noqa: E402

CACHE_HIT_NS = 227.0


def zmatrix_of(ctx, n, S, K=24, seed=1):
    g = torch.Generator(device=ctx.torch_device)
    g.manual_seed(seed)
    z = torch.randint(0, K, (S, n), dtype=torch.int32, device=ctx.torch_device, generator=g)
    z[::2] = z[::2] // 4
    zm = common_amd.ZMatrix(ctx, n, K)
    zm.add(z)
    res = zm.result()
    zm.close()
    return res


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def host_route(z):
    import scipy.cluster.hierarchy as hier
    h = z.cpu().numpy()
    n = h.shape[0]
    dist = 1. - np.array(h[np.triu_indices(n, k=1)])
    return np.array(hier.leaves_list(hier.linkage(dist)))


def stats(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(np.min(v)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096,16384")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--check-wide", action="store_true")
    args = ap.parse_args()
    ctx = common_amd.Context(0)
    out = {"cache_hit_ns": CACHE_HIT_NS, "steps": args.steps, "cases": []}
    for n in [int(s) for s in args.sizes.split(",") if s]:
        for S in (64, 1024):
            z = zmatrix_of(ctx, n, S)
            full, kern, none, host = [], [], [], []
            order = None
            for it in range(args.warmup + args.steps):
                f, (_, order) = wall_ms(lambda: ctx.linkage_single(z))
                k = event_ms(lambda: ctx.linkage_single(z, linkage=False, order=False))
                e, _ = wall_ms(lambda: ctx.linkage_single(z, linkage=False, order=False))
                h, want = wall_ms(lambda: host_route(z))
                if it >= args.warmup:
                    full.append(f), kern.append(k), none.append(e), host.append(h)
            case = {"n": n, "S": S, "distinct_values": int(torch.unique(z).numel()), "kernel_name": ctx.last_kernel("zmatrix"),
                    "device_call": stats(full), "kernel_and_edge_copy_events": stats(kern),
                    "host_tail": stats(np.array(full) - np.array(none)), "host_route": stats(host),
                    "order_equals_host_route": bool(np.array_equal(order, want))}
            step_ns = float(np.median(kern)) * 1e6 / (n - 1)
            case["kernel_ns_per_step"] = round(step_ns, 1)
            case["step_over_cache_hit"] = round(step_ns / CACHE_HIT_NS, 2)
            case["host_route_over_device_call"] = round(float(np.median(host) / np.median(full)), 1)
            out["cases"].append(case)
            del z
    if args.check_wide:
        import scipy.cluster.hierarchy as hier
        from scipy.spatial.distance import squareform
        out["wide"] = []
        for n in (16400, 32800):
            z = zmatrix_of(ctx, n, 64)
            ms, (lk, order) = wall_ms(lambda: ctx.linkage_single(z))
            name = ctx.last_kernel("zmatrix")
            d = np.float32(1.) - z.cpu().numpy()
            del z
            np.fill_diagonal(d, 0)
            want = hier.linkage(squareform(d, checks=False))          # (the same condensed order as triu_indices)
            del d
            out["wide"].append({"n": n, "kernel_name": name, "device_call_ms": round(ms, 3),
                                "linkage_equals_scipy": bool(np.array_equal(lk, want)),
                                "order_equals_scipy": bool(np.array_equal(order, hier.leaves_list(want)))})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
