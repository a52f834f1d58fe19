"""Time of split-merge proposals on a chain ensemble: the one-launch call (msc_chains_split_merge, ens.split_merge) beside
the loop it replaces (ens.states[c].split_merge for every chain) on the same build, the two routes alternated, warm, device
events around every call, the median of --reps:
    nich   one nich column
    c3     the mix bb + gp + dd(32) + nich x 16 (D = 64)
at K = 256 slots (32 true clusters, every chain started from them), N = 4 096 and 65 536 rows, --proposals proposals a
call, launch_iters 0 / 2 / 5, for --chains chains.  Per shape: milliseconds per call of either route, loop / ensemble, and
from the ensemble's times the microseconds per proposal, what one launch pass adds (the slope over launch_iters) and that
slope per (row, feature) -- what chains.cpp's sm_proposal_us is fitted to.  A shape the call refuses (one proposal
estimated beyond a launch's budget) is recorded as such.  Writes every line to --out as it is measured.

    python tools/bench_chains_splitmerge.py [nich] [c3] [--chains 1,16,64,256] [--rows 4096,65536] [--proposals 8]
                                            [--reps 5] [--out profiles/chains_splitmerge.txt]
"""
import argparse
import datetime
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import common_amd  # noqa: E402
from common_amd import BB, DD, GP, NICH  # noqa: E402
from tools.bench_blocked import commit_id  # noqa: E402
from tools.bench_configs import make_columns  # noqa: E402

MIXES = {"nich": [(NICH, 0)], "c3": [(BB, 0), (GP, 0), (DD, 32), (NICH, 0)] * 16}
LAUNCH_ITERS = (0, 2, 5)
K, CLUSTERS = 256, 32


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def shape(ctx, mix, N, nchains, nprop, reps, emit):
    spec = MIXES[mix]
    cols, z = make_columns(ctx, spec, N, CLUSTERS, 73)
    view = common_amd.DataView.from_tensors(ctx, cols)
    one = common_amd.ChainEnsemble(ctx, spec, K, nchains, alpha=1.0)
    loop = common_amd.ChainEnsemble(ctx, spec, K, nchains, alpha=1.0)
    per = {}
    for li in LAUNCH_ITERS:
        one.assign(view, z)
        loop.assign(view, z)
        sweep = [0]

        def run_one():
            one.split_merge(view, 73, sweep=sweep[0], nproposals=nprop, launch_iters=li)

        def run_loop():
            for c, st in enumerate(loop.states):
                st.split_merge(view, loop.z[c], 73 + c, sweep[0], nproposals=nprop, launch_iters=li)

        res = dict(mix=mix, D=len(spec), N=N, K=K, chains=nchains, proposals=nprop, launch_iters=li)
        try:
            run_one()                              # warm (and the pair states' creation)
        except common_amd.MicroscopesHipError as e:
            if e.code != -4:
                raise
            res["ensemble"] = "refused: one proposal estimated beyond a launch's budget"
            run_one = None
        run_loop()
        t_one, t_loop = [], []
        for r in range(reps):
            sweep[0] = (r + 1) * nprop
            if run_one is not None:
                t_one.append(_time(run_one))
            t_loop.append(_time(run_loop))
        res["loop_ms"] = round(statistics.median(t_loop), 4)
        if run_one is not None:
            res["ensemble_ms"] = round(statistics.median(t_one), 4)
            res["loop_over_ensemble"] = round(res["loop_ms"] / res["ensemble_ms"], 2)
            per[li] = 1000.0 * res["ensemble_ms"] / nprop
            res["ensemble_us_per_proposal"] = round(per[li], 2)
        emit(res)
    if len(per) == len(LAUNCH_ITERS):
        slope = (per[5] - per[0]) / 5.0
        emit(dict(mix=mix, N=N, chains=nchains, pass_us=round(slope, 2), fixed_us=round(per[0] - 2.0 * slope, 2),
                  pass_us_per_row_feature=round(slope / (N * len(spec)), 6)))
    one.close()
    loop.close()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mixes", nargs="*", default=[])
    ap.add_argument("--chains", default="1,16,64,256")
    ap.add_argument("--rows", default="4096,65536")
    ap.add_argument("--proposals", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--commit", default=None, help="the parent commit the figures are measured beside (default: git's HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chains_splitmerge.txt"))
    a = ap.parse_args()
    ctx = common_amd.Context(device=0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    fh = open(a.out, "w")

    def emit(rec):
        line = rec if isinstance(rec, str) else json.dumps(rec)
        print(line, flush=True)
        fh.write(line + "\n")
        fh.flush()

    emit("# Split-merge proposals on a chain ensemble: one launch (msc_chains_split_merge) beside the loop of "
         "msc_split_merge over the chains, same build: %s, %s, parent commit %s" %
         (torch.cuda.get_device_name(0), datetime.date.today().isoformat(), a.commit or commit_id()))
    emit("# median of %d warm calls of %d proposals, the two routes alternated, device events around each call; K = %d, %d "
         "true clusters" % (a.reps, a.proposals, K, CLUSTERS))
    for mix in (a.mixes or ["nich", "c3"]):
        for N in [int(x) for x in a.rows.split(",")]:
            for nchains in [int(x) for x in a.chains.split(",")]:
                shape(ctx, mix, N, nchains, a.proposals, a.reps, emit)
    fh.close()


if __name__ == "__main__":
    main()
