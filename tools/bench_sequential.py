"""Time per row visit of the sequential Gibbs sweep (msc_sweep_sequential) against the per-entity route on the same state
and rows (entity_op leave + score_value(crp_prior=True) of the row + copy back + host draw + entity_op join), N = 1e4
rows, K in {16, 64, 256, 1024}, three column mixes: one nich column, 16 bb columns, the C3 mix at D = 64 (16 each of
bb, gp, dd(32), nich).  The sequential sweep is timed with device events around whole sweeps after a warm-up sweep; the
per-entity route with the host clock over `--route-rows` rows, extrapolated per row.  Also the exact-posterior distance
of both samplers on the data of tests/test_gpu_sequential.py::test_exact_posterior_of_six_rows (--posterior).
With --phases (and MSC_LIB_PATH naming the experiment build `make -C common_amd/csrc VARIANT=seqphase
EXTRA=-DMSC_SEQ_PHASES`): the kernel's own s_memtime stamps split the timed sweeps' visits into read / leave / score / draw /
join, reported as shares and as microseconds of the measured visit.  Prints one JSON line per shape.

With --chains C[,C...]: ChainEnsemble.sweep (msc_chains_sweep, a workgroup per chain) instead, one sweep of C chains
timed warm with device events around the call, on one nich column and on the C3 mix at D = 64, K = 256; beside it the
route without the ensemble, back-to-back State.sweep_sequential calls on the same states (timed on --loop-chains of them
and scaled to C: the calls run one after another, one compute unit each).  Writes microseconds per visit per chain,
aggregate visits per second and the ratio to that loop into --out, with the date and the commit.

With --chains ... --tempered: for each of the two shapes and every chain count, ChainEnsemble.sweep(beta=) at beta = 1 and
at beta = 0.5 (msc_chains_sweep_tempered) next to the untempered ChainEnsemble.sweep on the same ensemble -- every timed
call is listed, so the spread of repeated calls stands beside the ratios -- then one iteration of run_tempered (sweep +
joint + exchange) on four-rung ladders and a 33-temperature ais.  Writes --out (default profiles/chains_tempered.txt).

    python tools/bench_sequential.py [--rows 10000] [--steps 3] [--route-rows 300] [--posterior] [--phases]
    python tools/bench_sequential.py --chains 1,16,64,256,512 [--sweep-rows 10000] [--out profiles/chains.txt]
    python tools/bench_sequential.py --chains 256 --tempered --rows 4096 --sweep-rows 4096 --steps 7
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


def chains(ctx, mix, N, K, counts, steps, sweep_rows, loop_chains):
    """one result per chain count: a timed sweep of rows [0, sweep_rows) by every chain of an ensemble, and by a loop of
    single-chain calls over the same states"""
    spec = MIXES[mix]
    cols, z = make_columns(ctx, spec, N, K, seed=K + len(spec))
    view = common_amd.DataView.from_tensors(ctx, cols)
    R = min(sweep_rows, N)

    def timed(fn):
        ms = []
        for s in range(steps + 1):                        # (the first is the warm-up)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn(s)
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return min(ms[1:])

    res = []
    for nc in counts:
        ens = common_amd.ChainEnsemble(ctx, spec, K, nc, alpha=1.0)
        ens.assign(view, z)
        torch.cuda.synchronize()
        ens_ms = timed(lambda s: ens.sweep(view, 1, 1000, sweep=s, nrows=R))
        L = min(nc, loop_chains)

        def loop(s):
            for c in range(L):
                ens.states[c].sweep_sequential(view, ens.z[c], 1000 + c, 100 + s, nrows=R)
        loop_ms = timed(loop) * nc / L
        ens.close()
        res.append(dict(mix=mix, K=K, N=N, features=len(spec), chains=nc, rows_swept=R,
                        us_per_visit_per_chain=round(ens_ms * 1e3 / R, 3),
                        visits_per_s=round(nc * R / (ens_ms * 1e-3)),
                        loop_us_per_visit=round(loop_ms * 1e3 / (nc * R), 3), loop_states_timed=L,
                        ratio_to_loop=round(loop_ms / ens_ms, 2)))
        print(json.dumps(res[-1]), flush=True)
    return res


def tempered(ctx, mix, N, K, counts, steps):
    """one result per chain count: whole sweeps of the N rows by every chain, untempered and at beta = 1 and 0.5, the three
    taken in turn `steps` times after a warm-up round; an iteration of run_tempered; a 33-temperature ais"""
    from common_amd import tempering
    spec = MIXES[mix]
    cols, z = make_columns(ctx, spec, N, K, seed=K + len(spec))
    view = common_amd.DataView.from_tensors(ctx, cols)
    dev = ctx.torch_device

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    res = []
    for nc in counts:
        ens = common_amd.ChainEnsemble(ctx, spec, K, nc, alpha=1.0)
        ens.assign(view, z)
        torch.cuda.synchronize()
        betas = {"untempered": None, "beta_1": torch.ones(nc, dtype=torch.float32, device=dev),
                 "beta_0.5": torch.full((nc,), 0.5, dtype=torch.float32, device=dev)}
        ms = {k: [] for k in betas}
        for s in range(steps + 1):                        # (the first round is the warm-up)
            for k, b in betas.items():
                t = timed(lambda: ens.sweep(view, 1, 1000, sweep=s, beta=b))
                if s:
                    ms[k].append(round(t, 3))
        base = float(np.median(ms["untempered"]))
        out = dict(mix=mix, K=K, N=N, features=len(spec), chains=nc, sweep_ms=ms,
                   untempered_spread=round((max(ms["untempered"]) - min(ms["untempered"])) / base, 4),
                   ratio_beta_1=round(float(np.median(ms["beta_1"])) / base, 4),
                   ratio_beta_0_5=round(float(np.median(ms["beta_0.5"])) / base, 4))
        if nc % 4 == 0:
            ladder = tempering.ladder(4, "linear")
            state = ens.run_tempered(view, 1, 1000, ladder, sweep=100)      # (warm-up)
            it = []
            for s in range(steps):
                it.append(round(timed(lambda: ens.run_tempered(view, 1, 1000, ladder, sweep=101 + s, state=state)), 3))
            out["run_tempered_iteration_ms"] = it
        t0 = time.perf_counter()
        r = ens.ais(view, np.linspace(0.0, 1.0, 33), 1000)
        out["ais_33_temperatures_s"] = round(time.perf_counter() - t0, 3)
        out["ais_log_evidence"], out["ais_ess"] = round(r.log_evidence, 3), round(r.ess, 2)
        ens.close()
        res.append(out)
        print(json.dumps(out), flush=True)
    return res


def commit_id():
    import subprocess
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL,
                                       text=True).strip()
    except Exception:
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", default=None, help="chain counts, e.g. 1,16,64,256,512: time ChainEnsemble.sweep instead")
    ap.add_argument("--sweep-rows", type=int, default=10000, help="--chains: rows of the N a timed sweep visits")
    ap.add_argument("--loop-chains", type=int, default=16, help="--chains: states the single-chain loop is timed on")
    ap.add_argument("--commit", default=None, help="--chains: the commit the figures belong to (default: git's HEAD)")
    ap.add_argument("--tempered", action="store_true", help="--chains: time the sweep at a temperature and its drivers")
    ap.add_argument("--out", default=None, help="default profiles/chains.txt, with --tempered profiles/chains_tempered.txt")
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--route-rows", type=int, default=300)
    ap.add_argument("--posterior", action="store_true")
    ap.add_argument("--phases", action="store_true")
    a = ap.parse_args()
    ctx = common_amd.Context(device=0)
    if a.chains:
        import datetime
        counts = [int(c) for c in a.chains.split(",")]
        if a.out is None:
            a.out = os.path.join(ROOT, "profiles", "chains_tempered.txt" if a.tempered else "chains.txt")
        if a.tempered:
            lines = ["# The sweep at a temperature (msc_chains_sweep_tempered, k_sweep_seq_chains_tempered) and its drivers: %s, %s, "
                     "commit %s" % (torch.cuda.get_device_name(0), datetime.date.today().isoformat(), a.commit or commit_id()),
                     "# sweep_ms: every timed call, one whole sweep of the N rows by every chain, device events around the call, "
                     "the three kinds taken in turn %d times after a warm-up round; untempered_spread = (max - min) / median of "
                     "the untempered calls; ratio_* = median tempered / median untempered;" % a.steps,
                     "# run_tempered_iteration_ms: one iteration (sweep + joint + exchange) on ladders of four rungs, events "
                     "around the call; ais_33_temperatures_s: seat + 33 sweeps + 32 joints and weight steps, host clock"]
            for mix in ("nich1", "c3_d64"):
                lines += [json.dumps(r) for r in tempered(ctx, mix, a.rows, 256, counts, a.steps)]
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")
            return
        lines = ["# Many sequential chains in one launch (msc_chains_sweep, k_sweep_seq_chains): %s, %s, commit %s"
                 % (torch.cuda.get_device_name(0), datetime.date.today().isoformat(), a.commit or commit_id()),
                 "# one sweep of rows_swept rows by every chain, best of %d warm calls, device events around the call;"
                 % a.steps,
                 "# loop: back-to-back State.sweep_sequential calls on the same states, timed on loop_states_timed of "
                 "them and scaled to `chains`"]
        for mix in ("nich1", "c3_d64"):
            lines += [json.dumps(r) for r in chains(ctx, mix, a.rows, 256, counts, a.steps, a.sweep_rows, a.loop_chains)]
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
        return
    for mix in ("nich1", "bb16", "c3_d64"):
        for K in (16, 64, 256, 1024):
            print(json.dumps(shape(ctx, mix, a.rows, K, a.steps, a.route_rows, a.phases)), flush=True)
    if a.posterior:
        for r in posterior(ctx):
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
