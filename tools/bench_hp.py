"""Grid hyper-parameter inference on the C3 feature mix (16 each of bb, gp, dd(32), nich; K = 256; suff-stats of ~1 M rows):
one grid Gibbs step (State.hp_gibbs) over every feature with a default grid (48: dd has none, 10 000 points each) plus a
100-point alpha grid, timed with device events around the synchronous call; the same scores taken point by point
through set_hp + score_data + download on a sample of points, extrapolated.  Prints one JSON line.

    python tools/bench_hp.py [--steps 20] [--warmup 3] [--sample 200]
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
from common_amd import hypers, models  # noqa: E402

F64_WAVE_INSTR_PER_SIMD_CYCLE = 0.25    # one f64 vector instruction issues every ~4 cycles on a SIMD


def c3_state(ctx, K, rows_per_group, rng):
    descs = [models.bb, models.gp, models.dd(32), models.nich] * 16
    st = common_amd.State(ctx, descs, K)
    n = rng.poisson(rows_per_group, K).astype(np.uint32)
    for f, d in enumerate(descs):
        rec = np.zeros(K, dtype=common_amd.ss_dtype(d.family, d.dim))
        if d.family == common_amd.BB:
            h = rng.binomial(n, rng.uniform(0.05, 0.95, K)).astype(np.uint32)
            rec["heads"], rec["tails"] = h, n - h
        elif d.family == common_amd.GP:
            rec["count"] = n
            rec["sum"] = rng.poisson(3.0 * n).astype(np.uint32)
            rec["log_prod"] = (1.5 * n).astype(np.float32)
        elif d.family == common_amd.DD:
            c = np.stack([rng.multinomial(int(k), np.ones(32) / 32) for k in n]).astype(np.uint32)
            rec["counts"], rec["count_sum"] = c, c.sum(1)
        else:
            rec["count"] = n
            rec["mean"] = rng.normal(0, 3, K).astype(np.float32)
            rec["count_times_variance"] = (rng.uniform(0.5, 2.0, K) * n).astype(np.float32)
        st.set_ss(f, rec)
    st.set_group_counts(n)
    st.set_alpha(1.0)
    return st, descs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sample", type=int, default=200)
    ap.add_argument("--K", type=int, default=256)
    args = ap.parse_args()
    ctx = common_amd.Context(0)
    rng = np.random.default_rng(1)
    K = args.K
    st, descs = c3_state(ctx, K, (1 << 20) // K, rng)
    alphas = np.logspace(-2, 2, 100)
    gibbs = hypers.FeatureHpGibbs(st, descs, cluster_grid=alphas)
    nfeat = len(gibbs.features)
    npoints = sum(len(gibbs.points[f]) for f in gibbs.features)
    for s in range(args.warmup):
        gibbs.step(seed=7, sweep=s)
    ms = []
    for s in range(args.steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        gibbs.step(seed=7, sweep=args.warmup + s)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    step_ms = float(np.median(ms))

    # point by point: set_hp + score_data of every feature and group + download, as the library allowed before
    out = torch.empty((len(descs), K), dtype=torch.float32, device=ctx.torch_device)
    feats = gibbs.features
    picks = [(feats[i % nfeat], int(rng.integers(0, 10000))) for i in range(args.sample)]
    for f, g in picks[:10]:
        st.set_hp(f, common_amd.pack_hp(descs[f].family, gibbs.points[f][g], descs[f].dim))
        st.score_data(out)[f].cpu()
    t0 = time.perf_counter()
    for f, g in picks:
        st.set_hp(f, common_amd.pack_hp(descs[f].family, gibbs.points[f][g], descs[f].dim))
        st.score_data(out)[f].cpu()
    per_point_ms = (time.perf_counter() - t0) * 1e3 / len(picks)
    pbp_ms = per_point_ms * (npoints + len(alphas))

    evals = npoints * K
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count
    clock_ghz = 2.4
    f64_instr_rate = num_cus * 4 * F64_WAVE_INSTR_PER_SIMD_CYCLE * clock_ghz * 1e9 * 64   # lane-instructions / s
    res = {
        "bench": "hp_grid_gibbs_c3_mix",
        "features_with_grid": nfeat, "grid_points": npoints, "alpha_points": len(alphas), "K": K,
        "score_data_evaluations": evals,
        "hp_gibbs_step_ms_median": round(step_ms, 4), "hp_gibbs_step_ms_min": round(float(np.min(ms)), 4),
        "steps_timed": args.steps,
        "evaluations_per_s": evals / (step_ms * 1e-3),
        "point_by_point_ms_per_point_measured": round(per_point_ms, 4), "point_by_point_sample": len(picks),
        "point_by_point_step_ms_EXTRAPOLATED": round(pbp_ms, 1),
        "speedup_vs_point_by_point": round(pbp_ms / step_ms, 1),
        "f64_vector_lane_instr_per_s_assumed": f64_instr_rate,
        "f64_instr_per_evaluation_if_at_roof": f64_instr_rate * step_ms * 1e-3 / evals,
    }
    print(json.dumps(res))


if __name__ == "__main__":
    main()
