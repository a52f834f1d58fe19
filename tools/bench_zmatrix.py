"""The z-matrix accumulator at m = 16 384 rows and S = 1 024 samples, for nlabels 64 and 256 (8-bit labels) and 1 024
(16-bit labels):
  add     ZMatrix.add of the [S, m] samples in one call (the pack kernels and, as batches fill, the count updates);
  finish  ZMatrix.result() after it (the update of the last partial batch, if any, and the m x m float32 matrix);
both timed with device events, the median of --steps runs after --warmup, each on a reset accumulator.  Beside them the
count update's rate in (i <= j, sample) triples a second and its fraction of the vector-issue roof (7.9e13
lane-instructions/s at 1.25 instructions a triple in the 8-bit form, 2.5 in the 16-bit form), and the host numpy path
(common_amd.query.zmatrix on numpy input) timed on --host-samples samples and EXTRAPOLATED linearly to S.
Prints one JSON line.

    python tools/bench_zmatrix.py [--steps 5] [--warmup 1] [--host-samples 4]
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
from common_amd import query  # noqa: E402

ROOF_LANE_OPS = 256 * 4 * 32 * 2.4e9     # CUs x SIMDs x lanes x clock: one wave64 instruction every 2 cycles a SIMD


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=16384)
    ap.add_argument("--S", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-samples", type=int, default=4)
    args = ap.parse_args()
    ctx = common_amd.Context(0)
    m, S = args.m, args.S
    triples = m * (m + 1) / 2 * S
    out = {"m": m, "S": S, "roof_lane_instr_per_s": ROOF_LANE_OPS, "device": {}}
    g = torch.Generator(device=ctx.torch_device)
    g.manual_seed(1)
    res = torch.empty((m, m), dtype=torch.float32, device=ctx.torch_device)
    for K in (64, 256, 1024):
        z = torch.randint(0, K, (S, m), dtype=torch.int32, device=ctx.torch_device, generator=g)
        zm = common_amd.ZMatrix(ctx, m, K)
        adds, fins = [], []
        for it in range(args.warmup + args.steps):
            zm.reset()
            a = event_ms(lambda: zm.add(z))
            f = event_ms(lambda: zm.result(out=res))
            if it >= args.warmup:
                adds.append(a)
                fins.append(f)
        total_s = (np.median(adds) + np.median(fins)) / 1e3
        per_triple = 1.25 if K <= 256 else 2.5
        roof_s = triples * per_triple / ROOF_LANE_OPS
        out["device"][str(K)] = {
            "label_bits": 8 if K <= 256 else 16,
            "add_ms": round(float(np.median(adds)), 3),
            "flush_finish_ms": round(float(np.median(fins)), 3),
            "total_ms": round(total_s * 1e3, 3),
            "triples_per_s": float("%.4g" % (triples / total_s)),
            "roof_ms": round(roof_s * 1e3, 3),
            "fraction_of_roof": round(roof_s / total_s, 3),
            "last_kernel": ctx.last_kernel("zmatrix"),
        }
        zm.close()
        del z
    # host numpy path: a few samples, extrapolated linearly in S
    rng = np.random.default_rng(2)
    hs = args.host_samples
    A = [rng.integers(0, 64, m).astype(np.int32) for _ in range(hs)]
    t0 = time.perf_counter()
    query.zmatrix(A)
    t = time.perf_counter() - t0
    out["host_numpy"] = {"samples_timed": hs, "seconds_timed": round(t, 3),
                         "seconds_for_S_extrapolated": round(t / hs * S, 1), "extrapolated": True, "nlabels": 64}
    out["speedup_vs_host_extrapolated_nlabels64"] = round(t / hs * S / (out["device"]["64"]["total_ms"] / 1e3), 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
