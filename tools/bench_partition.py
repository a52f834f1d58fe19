"""Posterior expected losses of candidate partitions at m = 16 384 rows, S = 1 024 samples and 1 024 candidates, with
K = 64 and K = 1 024 labels in the samples and the candidates:
  sums   ZMatrix.partition_sums of the [ncand, m] candidates (gather + k_zm_partition_sums, w and size written);
  loss   ZMatrix.partition_loss of the same (the all-in-one pass for T, then gather + sums + reduction a chunk at a time);
both timed with device events on an accumulator whose counts are already up to date, the median of --steps runs after
--warmup.  Beside them the sums kernel's lane-instructions per (pair, candidate) against the vector-issue roof (7.9e13
lane-instructions/s; 2.5 vector instructions a pair: a compare, a select and half an add3), and the torch route in the
same process on the same counts: per candidate counts.double() @ one_hot(labels), then a gather of every row's own
column -- float64, because a row sum passes 2^24 here -- timed on --torch-cands candidates and EXTRAPOLATED linearly.
The two routes' w are compared on those candidates.  Prints one JSON line.

    python tools/bench_partition.py [--steps 5] [--warmup 1] [--torch-cands 16]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import common_amd  # noqa: E402

ROOF_LANE_OPS = 256 * 4 * 32 * 2.4e9     # CUs x SIMDs x lanes x clock: one wave64 instruction every 2 cycles a SIMD
INSTR_PER_PAIR = 2.5


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def torch_route(counts_f64, cands, K):
    """w [ncand, m] float64: per candidate a one-hot matmul of the counts and a gather"""
    out = []
    for c in range(cands.shape[0]):
        lab = cands[c].long()
        per_label = counts_f64 @ torch.nn.functional.one_hot(lab, K).to(torch.float64)
        out.append(per_label.gather(1, lab[:, None])[:, 0])
    return torch.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=16384)
    ap.add_argument("--S", type=int, default=1024)
    ap.add_argument("--ncand", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--torch-cands", type=int, default=16)
    args = ap.parse_args()
    ctx = common_amd.Context(0)
    m, S, nc = args.m, args.S, args.ncand
    pairs = float(m) * m * nc
    roof_s = pairs * INSTR_PER_PAIR / ROOF_LANE_OPS
    out = {"m": m, "S": S, "ncand": nc, "roof_lane_instr_per_s": ROOF_LANE_OPS, "instr_per_pair": INSTR_PER_PAIR,
           "roof_ms": round(roof_s * 1e3, 3), "cases": {}}
    g = torch.Generator(device=ctx.torch_device)
    g.manual_seed(1)
    for K in (64, 1024):
        z = torch.randint(0, K, (S, m), dtype=torch.int32, device=ctx.torch_device, generator=g)
        z[::2] = z[::2] // 16                                # half of the samples with a sixteenth of the groups
        cands = torch.randint(0, K, (nc, m), dtype=torch.int32, device=ctx.torch_device, generator=g)
        q = min(S, nc // 4)
        cands[:q] = z[:q]                                    # a quarter of them are samples
        zm = common_amd.ZMatrix(ctx, m, K)
        zm.add(z)
        counts = zm.counts()
        sums, loss = [], []
        for it in range(args.warmup + args.steps):
            a = event_ms(lambda: zm.partition_sums(cands))
            name = ctx.last_kernel("zmatrix")
            b = event_ms(lambda: zm.partition_loss(cands))
            if it >= args.warmup:
                sums.append(a)
                loss.append(b)
        w, _ = zm.partition_sums(cands)
        tc = min(args.torch_cands, nc)
        cf = counts.double()
        torch_route(cf, cands[:2], K)                        # warm
        t_ms = event_ms(lambda: torch_route(cf, cands[:tc], K))
        same = bool(torch.equal(torch_route(cf, cands[:tc], K).to(torch.int64), w[:tc]))
        sums_s = float(np.median(sums)) / 1e3
        out["cases"][str(K)] = {
            "sums_ms": round(sums_s * 1e3, 3),
            "loss_ms": round(float(np.median(loss)), 3),
            "pair_candidates_per_s": float("%.4g" % (pairs / sums_s)),
            "fraction_of_roof": round(roof_s / sums_s, 3),
            "last_kernel": name,
            "torch_f64_candidates_timed": tc,
            "torch_f64_ms_timed": round(t_ms, 3),
            "torch_f64_ms_for_ncand_extrapolated": round(t_ms / tc * nc, 1),
            "extrapolated": True,
            "torch_w_equal": same,
            "speedup_vs_torch_f64_extrapolated": round(t_ms / tc * nc / (sums_s * 1e3), 1),
        }
        zm.close()
        del z, cands, counts, cf, w
    print(json.dumps(out))


if __name__ == "__main__":
    main()
