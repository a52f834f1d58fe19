"""Row predictive log-density (State.predictive_logp) against the two things it stands beside, timed with device events
around synchronised calls after a warm-up (median and min of --steps runs):
  (i)   predictive_logp: plain, with want_map, with leave-one-out, with both
  (ii)  what a caller did before it: score_value(crp_prior=True) into a preallocated [rows, K] matrix, then
        torch.logsumexp over it (the score pass alone is reported beside it)
  (iii) sweep_assign of the same state and rows: the same scoring plus a draw
for the shapes C2 (one nich column, 10^6 x 256), a C5 shard's (one nich column, K = 1024), C3's mix (16 each of bb, gp,
dd(32), nich) at K = 256 (both routes: the fused tile kernel and score pass + k_row_lse, forced with MSC_MARGINAL_TILE)
and at K = 512 (generic: score pass into scratch + k_row_lse).  One JSON line.

    python tools/bench_marginal.py [--steps 15] [--warmup 3] [--rows 1000000] [--shapes c2,c5,c3,c3k512]
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
from tools.bench_hp import c3_state  # noqa: E402
from tools.bench_predictive import timed  # noqa: E402


def nich_state(ctx, K, N, rng):
    st = common_amd.State(ctx, [models.nich], K)
    st.set_hp(0, dict(mu=0.0, kappa=1.0, sigmasq=1.0, nu=1.0))
    n = np.maximum(rng.poisson(N / K, K), 2).astype(np.uint32)
    rec = np.zeros(K, dtype=common_amd.ss_dtype(common_amd.NICH, 0))
    rec["count"], rec["mean"] = n, rng.normal(0, 10, K)
    rec["count_times_variance"] = n * rng.uniform(0.5, 2.0, K)
    st.set_ss(0, rec)
    st.set_group_counts(n)
    st.set_alpha(1.5)
    g = torch.Generator(device=ctx.torch_device)
    g.manual_seed(7)
    x = torch.randn((N,), device=ctx.torch_device, generator=g) * 10
    return st, common_amd.DataView.from_tensors(ctx, [x.contiguous()])


def c3_columns(ctx, descs, N, seed):
    g = torch.Generator(device=ctx.torch_device)
    g.manual_seed(seed)
    dev, cols = ctx.torch_device, []
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
    return common_amd.DataView.from_tensors(ctx, cols)


def measure(ctx, st, view, N, K, steps, warmup):
    dev = ctx.torch_device
    z = torch.randint(0, K, (N,), device=dev, dtype=torch.int32)
    out = torch.empty(N, dtype=torch.float32, device=dev)
    mat = torch.empty((N, K), dtype=torch.float32, device=dev)
    res = {}
    for name, kw in (("logp", {}), ("logp_map", dict(want_map=True)), ("logp_loo", dict(z=z)),
                     ("logp_loo_map", dict(z=z, want_map=True))):
        res[name] = timed(lambda: st.predictive_logp(view, out=out, **kw), steps, warmup)
    res["kernel"] = ctx.last_kernel("marginal")
    if len(st.features) > 1 and K <= 256:        # both routes of a mixed plan, whatever route_marginal picks (MSC_MARGINAL_TILE)
        for name, v in (("logp_tile_route", "1"), ("logp_generic_route", "0")):
            os.environ["MSC_MARGINAL_TILE"] = v
            res[name] = timed(lambda: st.predictive_logp(view, out=out), steps, warmup)
            res[name + "_loo"] = timed(lambda: st.predictive_logp(view, out=out, z=z), steps, warmup)
            res[name + "_kernel"] = ctx.last_kernel("marginal")
        del os.environ["MSC_MARGINAL_TILE"]
    res["score_then_logsumexp"] = timed(lambda: torch.logsumexp(st.score_value(view, out=mat, crp_prior=True), dim=1), steps, warmup)
    res["score_alone"] = timed(lambda: st.score_value(view, out=mat, crp_prior=True), steps, warmup)
    res["score_loo_then_logsumexp"] = timed(lambda: torch.logsumexp(st.score_value(view, out=mat, z=z, crp_prior=True), dim=1), steps, warmup)
    zs = z.clone()

    def sweep():
        zs.copy_(z)
        st.sweep_assign(view, zs, seed=3, sweep=0)
    res["sweep_assign"] = timed(sweep, steps, warmup)
    res["z_copy"] = timed(lambda: zs.copy_(z), steps, warmup)
    res["sweep_kernel"] = ctx.last_kernel("sweep")
    return {k: ([round(x, 4) for x in v] if isinstance(v, tuple) else v) for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--shapes", default="c2,c5,c3,c3k512")
    a = ap.parse_args()
    ctx = common_amd.Context(device=0)
    rng = np.random.default_rng(20261016)
    N = a.rows
    out = {"rows": N, "steps": a.steps, "unit": "ms [median, min]", "date": time.strftime("%Y-%m-%d"), "build": ctx.build_info()}
    for shape in a.shapes.split(","):
        if shape in ("c2", "c5"):
            K = 256 if shape == "c2" else 1024
            st, view = nich_state(ctx, K, N, rng)
        else:
            K = 256 if shape == "c3" else 512
            st, descs = c3_state(ctx, K, N // K, rng)
            view = c3_columns(ctx, descs, N, 11)
        out[shape] = dict(K=K, **measure(ctx, st, view, N, K, a.steps, a.warmup))
        del st, view
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
