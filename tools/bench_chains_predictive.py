"""The ensemble's imputation (ChainEnsemble.impute, msc_chains_sample_predictive) against what a caller did before it on
the same build -- State.predictive_logp of every member, a torch.multinomial on the stacked softmax for the row's chain,
State.impute(z=None) of every member over every row and a torch.where by chosen chain -- timed with device events
around synchronised calls after a warm-up (median and min of --steps runs):
  impute   ens.impute(view, out=out)                  (masked_only: half the entries are masked)
  parts    the same call's kernels one by one: the per-chain rows (ens.predictive_logp(per_chain=True), an upper bound
           of that share: it writes mix too), and the rest
  loop     the loop described above
for one nich column and for C3's mix (16 each of bb, gp, dd(32), nich), both at K = 256, on held-out blocks of --rows
rows.  Every chain holds its own suff-stats (drawn as tools/bench_chains_marginal.py draws them).  One JSON line.

    python tools/bench_chains_predictive.py [--chains 256] [--rows 4096,65536] [--shapes nich,c3] [--steps 15] [--warmup 3]
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
from common_amd import models  # noqa: E402
from tools.bench_chains_marginal import C3, ensemble  # noqa: E402
from tools.bench_predictive import c3_view, timed  # noqa: E402


def loop_impute(ens, view, lw, seed):
    logp = torch.stack([st.predictive_logp(view) for st in ens.states]) + lw
    chosen = torch.multinomial(torch.softmax(logp, dim=0).T, 1)[:, 0]
    out = None
    for c, st in enumerate(ens.states):
        vals, _ = st.impute(view, seed=seed)
        vals = {f: t.view(torch.int32) if t.dtype == torch.uint32 else t for f, t in vals.items()}   # (torch.where has no uint32)
        if out is None:
            out = {f: t.clone() for f, t in vals.items()}
        else:
            for f, t in vals.items():
                out[f] = torch.where(chosen == c, t, out[f])
    return out


def measure(ctx, ens, view, steps, warmup, loop_steps):
    dev, n = ctx.torch_device, int(view.nrows)
    lw = torch.full((ens.nchains, 1), -float(np.log(ens.nchains)), dtype=torch.float32, device=dev)
    out = ens.impute(view, seed=3)[0]
    res = {
        "impute": timed(lambda: ens.impute(view, seed=3, out=out), steps, warmup),
        "chain_rows": timed(lambda: ens.predictive_logp(view, per_chain=True), steps, warmup),
        "loop": timed(lambda: loop_impute(ens, view, lw, 3), loop_steps, 1),
    }
    res["loop_over_impute"] = round(res["loop"][0] / res["impute"][0], 2)
    res["rows_per_ms"] = round(n / res["impute"][0], 1)
    return {k: ([round(x, 4) for x in v] if isinstance(v, tuple) else v) for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=256)
    ap.add_argument("--rows", default="4096,65536")
    ap.add_argument("--shapes", default="nich,c3")
    ap.add_argument("--K", type=int, default=256)
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--loop-steps", type=int, default=None, help="runs of the loop (default: --steps)")
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    ctx = common_amd.Context(device=0)
    rng = np.random.default_rng(20261020)
    out = {"chains": a.chains, "K": a.K, "steps": a.steps, "masked": 0.5, "unit": "ms [median, min]",
           "date": time.strftime("%Y-%m-%d"), "build": ctx.build_info()}
    for shape in a.shapes.split(","):
        descs = [models.nich] if shape == "nich" else C3
        ens = ensemble(ctx, descs, a.K, a.chains, rng)
        for n in (int(r) for r in a.rows.split(",")):
            view, _ = c3_view(ctx, descs, n, 0.5, 11)
            out["%s_%d" % (shape, n)] = measure(ctx, ens, view, a.steps, a.warmup, a.loop_steps or a.steps)
            del view
        ens.close()
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
