"""Time per row visit of the sequential Gibbs sweep (msc_sweep_sequential) against the per-entity route on the same state
and rows (entity_op leave + score_value(crp_prior=True) of the row + copy back + host draw + entity_op join), N = 1e4
rows, K in {16, 64, 256, 1024}, three column mixes: one nich column, 16 bb columns, the C3 mix at D = 64 (16 each of
bb, gp, dd(32), nich).  The sequential sweep is timed with device events around whole sweeps after a warm-up sweep; the
per-entity route with the host clock over `--route-rows` rows, extrapolated per row.  Also the exact-posterior distance
of both samplers on the data of tests/test_gpu_sequential.py::test_exact_posterior_of_six_rows (--posterior).
With --phases (and MSC_LIB_PATH naming the experiment build `make -C common_amd/csrc VARIANT=seqphase
EXTRA=-DMSC_SEQ_PHASES`): the kernel's own s_memtime stamps split the timed sweeps' visits into read / leave / score / draw /
join, reported as shares and as microseconds of the measured visit.  Prints one JSON line per shape.

    python tools/bench_sequential.py [--rows 10000] [--steps 3] [--route-rows 300] [--posterior] [--phases]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import common_amd  # noqa: E402
from common_amd import BB, DD, GP, NICH  # noqa: E402
from tools.bench_configs import make_columns  # noqa: E402

MIXES = {"nich1": [(NICH, 0)], "bb16": [(BB, 0)] * 16, "c3_d64": [(BB, 0), (GP, 0), (DD, 32), (NICH, 0)] * 16}


PHASES = ("read", "leave", "score", "draw", "join")


def shape(ctx, mix, N, K, steps, route_rows, phases=False):
    spec = MIXES[mix]
    cols, z = make_columns(ctx, spec, N, K, seed=K + len(spec))
    view = common_amd.DataView.from_tensors(ctx, cols)
    st = common_amd.State(ctx, spec, K)
    st.set_alpha(1.0)
    st.accumulate(view, z)
    # the sequential sweep: whole sweeps over the N rows
    st.sweep_sequential(view, z, 1, 0)
    torch.cuda.synchronize()
    cyc = (C.c_ulonglong * 6)()
    if phases:
        ctx.lib.msc_seq_phase_cycles(cyc)            # (clears what the warm-up sweep stamped)
    ms = []
    for s in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        st.sweep_sequential(view, z, 1, 1 + s)
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    seq_us = min(ms) * 1e3 / N
    split = None
    if phases:
        ctx.lib.msc_seq_phase_cycles(cyc)
        tot = float(sum(cyc[:5])) or 1.0
        split = {p: dict(share=round(cyc[i] / tot, 3), us=round(seq_us * cyc[i] / tot, 2)) for i, p in enumerate(PHASES)}
        split["cycles_per_visit"] = round(tot / max(1, cyc[5]), 0)
    # the per-entity route on the same state and rows
    zh = z.cpu().numpy()
    out = torch.empty((1, K), dtype=torch.float32, device=ctx.torch_device)
    rng = np.random.default_rng(0)
    ctx.synchronize()
    t0 = time.perf_counter()
    for r in range(route_rows):
        g = int(zh[r])
        st.entity_op(view, r, g, join=False)
        st.score_value(view, out=out, row0=r, nrows=1, crp_prior=True)
        sc = out.cpu().numpy()[0].astype(np.float64)
        p = np.exp(sc - sc.max())
        c = np.cumsum(p)
        j = min(int(np.searchsorted(c, rng.random() * c[-1], side="right")), K - 1)
        st.entity_op(view, r, j, join=True)
        zh[r] = j
    ctx.synchronize()
    route_us = (time.perf_counter() - t0) * 1e6 / route_rows
    out = dict(mix=mix, K=K, N=N, features=len(spec), seq_us_per_row=round(seq_us, 3),
               route_us_per_row=round(route_us, 2), speedup=round(route_us / seq_us, 1))
    if split:
        out["phases"] = split
    return out


def posterior(ctx, sweeps_seq=200000, sweeps_batched=20000):
    """TV / KL to the exact posterior of the six-row data sets of the GPU test, for both samplers"""
    from oracle import oracle as orc
    from tests import seq_helpers as sh
    from tests.gpu_helpers import make_feature, recarray_of
    rng = np.random.default_rng(2024)
    N, K, alpha = 6, 7, 1.0
    datasets = {"bb3": [make_feature(orc.BB, N, 2, rng) for _ in range(3)],
                "nich_bb": [make_feature(orc.NICH, N, 2, rng), make_feature(orc.BB, N, 2, rng)]}
    datasets["nich_bb"][0]["values"] = np.array([0.2, -0.4, 0.1, 2.5, 2.9, 5.0], dtype=np.float32)
    res = []
    for name, feats in datasets.items():
        Fs = [orc.Family(f["family"], f["hp"], f["dim"], "f64") for f in feats]
        parts, p = sh.exact_posterior([(F, f["values"]) for F, f in zip(Fs, feats)], alpha)
        view = common_amd.DataView.from_recarray(ctx, recarray_of(feats))
        out = dict(data=name)
        for kind in ("sequential", "batched"):
            st = common_amd.State(ctx, [(f["family"], f["dim"]) for f in feats], K)
            for i, F in enumerate(Fs):
                st.set_hp(i, F.hp)
            st.set_alpha(alpha)
            zt = torch.full((N,), -1, dtype=torch.int32, device=ctx.torch_device)
            st.accumulate(view, zt)
            if kind == "sequential":
                tr = torch.empty(sweeps_seq * N, dtype=torch.int32, device=ctx.torch_device)
                st.sweep_sequential(view, zt, 77, 0, nsweeps=sweeps_seq, trace=tr)
                traces = tr.cpu().numpy().reshape(sweeps_seq, N)
            else:
                tr = torch.empty((sweeps_batched, N), dtype=torch.int32, device=ctx.torch_device)
                for s in range(sweeps_batched):
                    st.sweep_step(view, zt, 77, s)
                    tr[s].copy_(zt)
                traces = tr.cpu().numpy()
            tv, kl = sh.tv_kl(sh.partition_frequencies(traces, parts), p)
            out[kind] = dict(sweeps=len(traces), tv=round(tv, 4), kl=round(kl, 5))
        res.append(out)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--route-rows", type=int, default=300)
    ap.add_argument("--posterior", action="store_true")
    ap.add_argument("--phases", action="store_true")
    a = ap.parse_args()
    ctx = common_amd.Context(device=0)
    for mix in ("nich1", "bb16", "c3_d64"):
        for K in (16, 64, 256, 1024):
            print(json.dumps(shape(ctx, mix, a.rows, K, a.steps, a.route_rows, a.phases)), flush=True)
    if a.posterior:
        for r in posterior(ctx):
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
