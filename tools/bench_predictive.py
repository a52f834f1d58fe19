"""Posterior predictive sampling on the C3 feature mix (16 each of bb, gp, dd(32), nich; K = 256; 1 M rows, 20 % of the
entries masked at a fixed seed), timed with device events around synchronised calls after a warm-up:
  (a) State.impute with z = None: every row's group drawn, then its masked entries
  (b) the same call with z given: the value draws alone
  (c) every entry of one niw d = 32 feature over 1 M rows at K = 256
  (d) the host route: get_ss of every feature (measured), then the C++ host sampler (group::sample_value of
      include/microscopes_amd/hip_models.hpp) one entry at a time, timed on a sample of entries by
      tools/bench_host_sample.cpp and extrapolated to (a)'s entry count
Prints one JSON line.

    python tools/bench_predictive.py [--steps 10] [--warmup 2] [--rows 1048576] [--sample 1000000]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import common_amd  # noqa: E402
from common_amd import models  # noqa: E402
from tools.bench_hp import c3_state  # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


def c3_view(ctx, descs, N, frac, seed):
    g = torch.Generator(device=ctx.torch_device)
    g.manual_seed(seed)
    dev = ctx.torch_device
    cols, masks = [], []
    for d in descs:
        if d.family == common_amd.BB:
            c = torch.randint(0, 2, (N,), device=dev, generator=g).to(torch.bool)
        elif d.family == common_amd.GP:
            c = torch.randint(0, 12, (N,), device=dev, generator=g, dtype=torch.int32)
        elif d.family == common_amd.DD:
            c = torch.randint(0, 32, (N,), device=dev, generator=g, dtype=torch.int32)
        else:
            c = torch.randn((N,), device=dev, generator=g) * 3
        cols.append(c.contiguous())
        masks.append((torch.rand((N,), device=dev, generator=g) < frac).to(torch.uint8))
    return common_amd.DataView.from_tensors(ctx, cols, masks), masks


def niw_state(ctx, K, d, rows_per_group, rng):
    st = common_amd.State(ctx, [models.niw(d)], K)
    st.set_hp(0, dict(mu=np.zeros(d), kappa=1.0, psi=np.eye(d), nu=float(d + 2)))
    rec = np.zeros(K, dtype=common_amd.ss_dtype(common_amd.NIW, d))
    n = rng.poisson(rows_per_group, K).astype(np.uint32) + 1
    m = rng.normal(0, 2, (K, d))
    rec["count"] = n
    rec["sum_x"] = (n[:, None] * m).astype(np.float32)
    rec["sum_xxT"] = (n[:, None, None] * (np.eye(d)[None] + np.einsum("ki,kj->kij", m, m))).astype(np.float32)
    st.set_ss(0, rec)
    st.set_group_counts(n)
    return st


def host_route(st, descs, K, rows, entries, sample):
    """get_ss of every feature (measured here), then the C++ host sampler -- group::sample_value, one entry at a time --
    timed per entry on `sample` entries by tools/bench_host_sample.cpp and extrapolated to `entries`"""
    t0 = time.perf_counter()
    for f in range(len(descs)):
        st.get_ss(f)
    get_ss_ms = (time.perf_counter() - t0) * 1e3
    lib = os.path.join(ROOT, "common_amd", "lib")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "bench_host_sample")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                               os.path.join(ROOT, "tools", "bench_host_sample.cpp"), "-L" + lib, "-lmicroscopes_hip",
                               "-Wl,-rpath," + lib, "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"])
        r = json.loads(subprocess.check_output([exe, str(sample), str(K), str(rows)], timeout=600).decode())
    per_entry_us = r["host_us_per_entry"]
    return get_ss_ms, per_entry_us, get_ss_ms + per_entry_us * entries * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--K", type=int, default=256)
    ap.add_argument("--sample", type=int, default=1000000)
    ap.add_argument("--only", default="abcd", help="which of the measurements to take (profiling runs take one)")
    args = ap.parse_args()
    ctx = common_amd.Context(0)
    rng = np.random.default_rng(1)
    K, N = args.K, args.rows
    st, descs = c3_state(ctx, K, N // K, rng)
    view, masks = c3_view(ctx, descs, N, 0.2, 20261015)
    masked = int(sum(int(m.sum().item()) for m in masks))
    res = {"bench": "predictive_c3_mix", "rows": N, "features": len(descs), "K": K, "masked_entries": masked,
           "steps_timed": args.steps}
    z = torch.from_numpy(rng.integers(0, K, N).astype(np.int32)).to(ctx.torch_device)
    outs = {}

    def impute(zz):
        o, _ = st.impute(view, z=zz, seed=5, sweep=0, out=outs)
        outs.update(o)

    if "a" in args.only:
        res["a_impute_group_draw_ms_median"], res["a_impute_group_draw_ms_min"] = timed(lambda: impute(None), args.steps,
                                                                                       args.warmup)
        zs = z.clone()
        res["c3_assignment_pass_ms_median"], _ = timed(lambda: st.sweep_assign(view, zs, seed=5, sweep=0), args.steps,
                                                        args.warmup)
    if "b" in args.only:
        res["b_impute_values_only_ms_median"], res["b_impute_values_only_ms_min"] = timed(lambda: impute(z), args.steps,
                                                                                         args.warmup)
        res["b_entries_drawn"] = masked
        res["b_entries_written"] = N * len(descs)
    if "c" in args.only:
        d = 32
        sn = niw_state(ctx, K, d, N // K, rng)
        vn = common_amd.DataView.from_tensors(ctx, [torch.randn((N, d), device=ctx.torch_device)])
        on = {}

        def niw():
            o, _ = sn.sample_predictive(vn, z=z, seed=5, sweep=0, out=on)
            on.update(o)
        res["c_niw32_all_entries_ms_median"], res["c_niw32_all_entries_ms_min"] = timed(niw, args.steps, args.warmup)
    if "d" in args.only:
        get_ss_ms, per_entry_us, host_ms = host_route(st, descs, K, N, masked, args.sample)
        res["d_host_get_ss_ms_measured"] = round(get_ss_ms, 3)
        res["d_host_us_per_entry_measured"] = round(per_entry_us, 4)
        res["d_host_entries_sampled"] = args.sample
        res["d_host_route_ms_EXTRAPOLATED"] = round(host_ms, 1)
        if "a_impute_group_draw_ms_median" in res:
            res["speedup_a_vs_host_route"] = round(host_ms / res["a_impute_group_draw_ms_median"], 1)
        if "b_impute_values_only_ms_median" in res:
            res["speedup_b_vs_host_route"] = round(host_ms / res["b_impute_values_only_ms_median"], 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
