"""The log joint of every chain of an ensemble (ChainEnsemble.score_joint, msc_chains_score_joint) against the loop it
replaces, on one nich column and on the 64-column C3 mix (16 each of bb, gp, dd(32), nich) at K = 256, states
accumulated from --rows rows:
  ensemble   one ens.score_joint() and the download of its [chains, nfeatures + 3] doubles;
  loop       the host route, which needs nothing this call adds: per state score_data() (floats, every slot), its
             download and a host sum over the occupied slots, plus score_assignment on the host from the downloaded
             group counts (lgamma in double);
  run / run_tracked   ens.run of --iters iterations on a view of --run-rows rows without and with a JointTracker
             (every=1, keep_best): what tracing the joint adds to an iteration.
Timed warm with a host clock around work that ends in a device synchronisation, the two routes alternated on the SAME
ensemble, --repeats rounds after one warm-up round; the median and the spread (min, max) are reported, and how far the
two totals are apart (the loop's is a float sum).  One JSON line per mix, printed and appended to --out.

    python tools/bench_joint.py [--chains 256] [--K 256] [--rows 4096] [--repeats 7] [--out profiles/chains_joint.txt]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import common_amd  # noqa: E402
from common_amd import models  # noqa: E402
from tools.bench_configs import make_columns  # noqa: E402

_LGAMMA = np.vectorize(math.lgamma, otypes=[np.float64])


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def host_joint(ens, out):
    """the loop the ensemble call replaces -> totals [chains]"""
    totals = np.zeros(ens.nchains)
    for c, st in enumerate(ens.states):
        sd = st.score_data(out).cpu().numpy()
        cnt = st.get_group_counts()
        occ = cnt > 0
        a = float(st.get_alpha())
        n = float(cnt.sum())
        assign = occ.sum() * math.log(a) + float(_LGAMMA(cnt[occ].astype(np.float64)).sum()) + math.lgamma(a) - \
            math.lgamma(n + a)
        totals[c] = assign + float(sd[:, occ].astype(np.float64).sum())
    return totals


def stats(ms):
    return dict(median=round(float(np.median(ms)), 3), min=round(float(np.min(ms)), 3), max=round(float(np.max(ms)), 3))


def case(ctx, name, descs, args):
    spec = [(d.family, d.dim) for d in descs]
    K, nchains = args.K, args.chains
    cols, z = make_columns(ctx, spec, args.rows, K, seed=73)
    view = common_amd.DataView.from_tensors(ctx, cols)
    ens = common_amd.ChainEnsemble(ctx, spec, K, nchains, alpha=1.0)
    zs = torch.stack([torch.roll(z, c) for c in range(nchains)])           # every chain its own partition
    ens.assign(view, zs)
    out = torch.empty((len(spec), K), dtype=torch.float32, device=ctx.torch_device)
    got = {}
    t = dict(ensemble=[], loop=[])
    for r in range(args.repeats + 1):                                        # (the first round is the warm-up)
        t["ensemble"].append(wall_ms(lambda: got.__setitem__("ens", ens.score_joint().cpu().numpy())))
        t["loop"].append(wall_ms(lambda: got.__setitem__("loop", host_joint(ens, out))))
    apart = float(np.max(np.abs(got["ens"][:, 0] - got["loop"]) / np.maximum(1.0, np.abs(got["loop"]))))
    rec = dict(what="chains_joint", mix=name, K=K, rows=args.rows, features=len(spec), chains=nchains, repeats=args.repeats,
               ensemble_ms=stats(t["ensemble"][1:]), loop_ms=stats(t["loop"][1:]), totals_apart_rel=apart)
    rec["loop_over_ensemble"] = round(rec["loop_ms"]["median"] / rec["ensemble_ms"]["median"], 1)
    # run with and without a tracker, on a view of its own (a sequential sweep is a chain of row visits)
    rcols, rz = make_columns(ctx, spec, args.run_rows, K, seed=74)
    rview = common_amd.DataView.from_tensors(ctx, rcols)
    ens.assign(rview, rz)
    tracker = common_amd.JointTracker(ens)
    tr = dict(run=[], run_tracked=[])
    for r in range(args.repeats + 1):
        tr["run"].append(wall_ms(lambda: ens.run(rview, args.iters, 11, sweep=2 * r * args.iters)))
        tr["run_tracked"].append(wall_ms(lambda: ens.run(rview, args.iters, 11, sweep=(2 * r + 1) * args.iters, joint=tracker)))
    rec.update(run_rows=args.run_rows, run_iters=args.iters, run_ms=stats(tr["run"][1:]),
               run_tracked_ms=stats(tr["run_tracked"][1:]))
    rec["tracker_ms_per_iteration"] = round((rec["run_tracked_ms"]["median"] - rec["run_ms"]["median"]) / args.iters, 4)
    rec["run_tracked_over_run"] = round(rec["run_tracked_ms"]["median"] / rec["run_ms"]["median"], 3)
    ens.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=256)
    ap.add_argument("--K", type=int, default=256)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--run-rows", type=int, default=256)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--mixes", default="nich1,c3")
    ap.add_argument("--out", default=os.path.join("profiles", "chains_joint.txt"))
    args = ap.parse_args()
    ctx = common_amd.Context(0)
    mixes = {"nich1": [models.nich], "c3": [models.bb, models.gp, models.dd(32), models.nich] * 16}
    for name in args.mixes.split(","):
        line = json.dumps(case(ctx, name, mixes[name], args))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
