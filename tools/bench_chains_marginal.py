"""The ensemble's posterior-averaged row predictive density (ChainEnsemble.predictive_logp, msc_chains_score_marginal)
against what a caller did before it -- a loop of State.predictive_logp over the member states, a stack and
torch.logsumexp -- on the same build, timed with device events around synchronised calls after a warm-up (median and min
of --steps runs):
  mix            ens.predictive_logp(view, out=out)
  mix_per_chain  ... with per_chain=True (the [chains, rows] matrix is written too)
  loop           torch.logsumexp(torch.stack([st.predictive_logp(view) for st in ens.states]) + lw, 0)
for one nich column and for C3's mix (16 each of bb, gp, dd(32), nich), both at K = 256, on held-out blocks of --rows
rows.  Every chain holds its own suff-stats (drawn as tools/bench_marginal.py draws a state's).  One JSON line.

    python tools/bench_chains_marginal.py [--chains 256] [--rows 4096,65536] [--shapes nich,c3] [--steps 15] [--warmup 3]
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
from tools.bench_marginal import c3_columns  # noqa: E402
from tools.bench_predictive import timed  # noqa: E402

C3 = [models.bb, models.gp, models.dd(32), models.nich] * 16


def fill_state(st, descs, K, rows_per_group, rng):
    """suff-stats of every feature as tools/bench_hp.py c3_state draws them (a nich column: bench_marginal.py nich_state)"""
    n = np.maximum(rng.poisson(rows_per_group, K), 2).astype(np.uint32)
    for f, d in enumerate(descs):
        rec = np.zeros(K, dtype=common_amd.ss_dtype(d.family, d.dim))
        if d.family == common_amd.BB:
            h = rng.binomial(n, rng.uniform(0.05, 0.95, K)).astype(np.uint32)
            rec["heads"], rec["tails"] = h, n - h
        elif d.family == common_amd.GP:
            rec["count"], rec["sum"], rec["log_prod"] = n, rng.poisson(3.0 * n).astype(np.uint32), (1.5 * n).astype(np.float32)
        elif d.family == common_amd.DD:
            c = rng.multinomial(n, np.ones(d.dim) / d.dim).astype(np.uint32)
            rec["counts"], rec["count_sum"] = c, c.sum(1)
        else:
            rec["count"], rec["mean"] = n, rng.normal(0, 3, K).astype(np.float32)
            rec["count_times_variance"] = (rng.uniform(0.5, 2.0, K) * n).astype(np.float32)
        st.set_ss(f, rec)
    st.set_group_counts(n)


def ensemble(ctx, descs, K, nchains, rng):
    ens = common_amd.ChainEnsemble(ctx, descs, K, nchains, alpha=1.5)
    for st in ens.states:
        fill_state(st, descs, K, 4096, rng)
    return ens


def measure(ctx, ens, view, steps, warmup):
    dev, n = ctx.torch_device, int(view.nrows)
    out = torch.empty(n, dtype=torch.float32, device=dev)
    lw = torch.full((ens.nchains, 1), -float(np.log(ens.nchains)), dtype=torch.float32, device=dev)
    res = {
        "mix": timed(lambda: ens.predictive_logp(view, out=out), steps, warmup),
        "mix_per_chain": timed(lambda: ens.predictive_logp(view, out=out, per_chain=True), steps, warmup),
        "loop": timed(lambda: torch.logsumexp(torch.stack([st.predictive_logp(view) for st in ens.states]) + lw, dim=0),
                      steps, warmup),
    }
    res["loop_kernel"] = ctx.last_kernel("marginal")
    res["loop_over_mix"] = round(res["loop"][0] / res["mix"][0], 2)
    return {k: ([round(x, 4) for x in v] if isinstance(v, tuple) else v) for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=256)
    ap.add_argument("--rows", default="4096,65536")
    ap.add_argument("--shapes", default="nich,c3")
    ap.add_argument("--K", type=int, default=256)
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    ctx = common_amd.Context(device=0)
    rng = np.random.default_rng(20261020)
    out = {"chains": a.chains, "K": a.K, "steps": a.steps, "unit": "ms [median, min]", "date": time.strftime("%Y-%m-%d"),
           "build": ctx.build_info()}
    for shape in a.shapes.split(","):
        descs = [models.nich] if shape == "nich" else C3
        ens = ensemble(ctx, descs, a.K, a.chains, rng)
        for n in (int(r) for r in a.rows.split(",")):
            if shape == "nich":
                g = torch.Generator(device=ctx.torch_device)
                g.manual_seed(7)
                view = common_amd.DataView.from_tensors(ctx, [(torch.randn((n,), device=ctx.torch_device, generator=g) * 3).contiguous()])
            else:
                view = c3_columns(ctx, descs, n, 11)
            out["%s_%d" % (shape, n)] = measure(ctx, ens, view, a.steps, a.warmup)
            del view
        ens.close()
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
