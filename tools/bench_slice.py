"""Slice sampling on the C3 feature mix (tools/bench_hp.py's state: 16 each of bb, gp, dd(32), nich; K = 256):
  (a) one FeatureHpSlice step over every feature with default hyper-priors (48: dd has none; 2 coordinates each) plus
      alpha under log_exponential(1), timed with device events around the synchronous call, and the mean evaluations an
      update took;
  (b) the host route for the same step: set_hp + score_data + download per evaluation of a target, timed on a sample of
      evaluations in the same run and multiplied by (a)'s evaluation count;
  (c) one theta_slice over 16 bbnc columns x K = 256.
Prints one JSON line.

    python tools/bench_slice.py [--steps 50] [--warmup 5] [--sample 200]

With --chains the ensemble's step instead (ChainEnsemble.hp_slice, msc_chains_hp_slice), on one nich column and on the
C3 mix at K = 256, states accumulated from --rows rows, for every ensemble size of the list.  Timed warm, with device
events around the synchronous call, the two routes alternated on the SAME ensemble, median of --repeats:
  ensemble   one ens.hp_slice over every default coordinate plus alpha;
  loop       the route it replaces: ens.states[c].hp_slice for every chain (a launch, two copies, a wait each);
  sweep      the first ens.sweep of ONE row after each, which carries the rebuild of the score and CRP tables the step
             made stale (after the ensemble call they are current already).
One JSON line per (mix, chains), printed and appended to --out (default profiles/chains_hp.txt).

    python tools/bench_slice.py --chains 1,16,64,256 [--repeats 5] [--rows 4096] [--out profiles/chains_hp.txt]
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
from common_amd import hypers, scalar_functions as sf  # noqa: E402
from tools.bench_hp import c3_state  # noqa: E402


def timed(fn, steps, warmup):
    for s in range(warmup):
        fn(s)
    ms = []
    for s in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(warmup + s)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def chains_case(ctx, name, descs, K, rows, nchains, repeats):
    from common_amd.chains import chain_seeds
    from tools.bench_configs import make_columns
    spec = [(d.family, d.dim) for d in descs]
    cols, z = make_columns(ctx, spec, rows, K, seed=73)
    view = common_amd.DataView.from_tensors(ctx, cols)
    ens = common_amd.ChainEnsemble(ctx, spec, K, nchains, alpha=1.0)
    ens.assign(view, z)
    sl = hypers.EnsembleHpSlice(ens, descs, cparam={"alpha": (sf.log_exponential(1.0), 1.0)})
    keys = chain_seeds(7, nchains)

    def loop(s):
        for c, st in enumerate(ens.states):
            st.hp_slice(sl.coords, keys[c], s)
    t = dict(ensemble=[], sweep_after_ensemble=[], loop=[], sweep_after_loop=[])
    evals = []
    for r in range(repeats + 1):                            # (the first round is the warm-up)
        torch.cuda.synchronize()
        t["ensemble"].append(event_ms(lambda: evals.append(int(ens.hp_slice(sl.coords, 7, sweep=2 * r)[1].sum()))))
        t["sweep_after_ensemble"].append(event_ms(lambda: ens.sweep(view, 1, 11, sweep=2 * r, nrows=1)))
        t["loop"].append(event_ms(lambda: loop(2 * r + 1)))
        t["sweep_after_loop"].append(event_ms(lambda: ens.sweep(view, 1, 11, sweep=2 * r + 1, nrows=1)))
    ens.close()
    rec = dict(what="chains_hp", mix=name, K=K, rows=rows, features=len(descs), chains=nchains, updates_per_chain=len(sl.coords),
               evaluations_per_update_mean=round(float(np.mean(evals[1:])) / (nchains * len(sl.coords)), 2), repeats=repeats)
    for k, v in t.items():
        rec[k + "_ms"] = [round(x, 3) for x in v[1:]]
        rec[k + "_ms_median"] = round(float(np.median(v[1:])), 3)
    rec["loop_over_ensemble"] = round(rec["loop_ms_median"] / rec["ensemble_ms_median"], 2)
    rec["ensemble_faster_than_loop"] = bool(rec["ensemble_ms_median"] < rec["loop_ms_median"])
    return rec


def chains_main(args):
    from common_amd import models
    ctx = common_amd.Context(0)
    sizes = [int(c) for c in args.chains.split(",")]
    mixes = [("nich1", [models.nich]), ("c3", [models.bb, models.gp, models.dd(32), models.nich] * 16)]
    for name, descs in mixes:
        for nchains in sizes:
            line = json.dumps(chains_case(ctx, name, descs, args.K, args.rows, nchains, args.repeats))
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as fh:
                    fh.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", default=None, help="ensemble sizes, e.g. 1,16,64,256: time the ensemble's step")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join("profiles", "chains_hp.txt"))
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sample", type=int, default=200)
    ap.add_argument("--K", type=int, default=256)
    args = ap.parse_args()
    if args.chains is not None:
        return chains_main(args)
    ctx = common_amd.Context(0)
    rng = np.random.default_rng(1)
    K = args.K
    st, descs = c3_state(ctx, K, (1 << 20) // K, rng)

    # (a) the device step
    sl = hypers.FeatureHpSlice(st, descs, cparam={"alpha": (sf.log_exponential(1.0), 1.0)})
    evals = []

    def step(s):
        sl.step(seed=7, sweep=s)
        evals.append(int(sl.last_evals.sum()))
    ms = timed(step, args.steps, args.warmup)
    step_ms = float(np.median(ms))
    updates = len(sl.coords)
    # the bare call (State.hp_slice) without FeatureHpSlice's read-back of 48 hp blocks into dicts
    call_ms = timed(lambda s: st.hp_slice(sl.coords, seed=7, sweep=1000 + s), args.steps, args.warmup)
    evals_per_step = float(np.mean(evals[args.warmup:]))

    # (b) the host route: one evaluation of a feature coordinate's target = set_hp + score_data + a download
    out = torch.empty((len(descs), K), dtype=torch.float32, device=ctx.torch_device)
    feats = sl.features
    hp0 = {f: st.get_hp(f).copy() for f in feats}
    picks = [(feats[i % len(feats)], float(rng.uniform(0.5, 2.0))) for i in range(args.sample)]

    def host_eval(f, scale):
        hp = hp0[f].copy()
        hp[-1 if descs[f].family == common_amd.NICH else 0] *= scale
        st.set_hp(f, hp)
        st.score_data(out)[f].cpu()
    for f, x in picks[:10]:
        host_eval(f, x)
    t0 = time.perf_counter()
    for f, x in picks:
        host_eval(f, x)
    per_eval_ms = (time.perf_counter() - t0) * 1e3 / len(picks)
    for f in feats:
        st.set_hp(f, hp0[f])
    host_ms = per_eval_ms * evals_per_step

    # (c) theta over 16 bbnc columns x K
    tst = common_amd.State(ctx, [(common_amd.BBNC, 0)] * 16, K)
    for f in range(16):
        rec = np.zeros(K, dtype=common_amd.ss_dtype(common_amd.BBNC, 0))
        n = rng.poisson((1 << 20) // K, K).astype(np.uint32)
        rec["heads"] = rng.binomial(n, rng.uniform(0.05, 0.95, K))
        rec["tails"] = n - rec["heads"]
        rec["p"] = rng.uniform(0.05, 0.95, K)
        tst.set_ss(f, rec)
    tst.set_group_counts(np.full(K, 1, np.uint32))
    tparams = {f: {"p": 0.1} for f in range(16)}
    tev = []
    tms = timed(lambda s: tev.append(sum(tst.theta_slice(tparams, seed=3, sweep=s).values())), args.steps, args.warmup)

    res = {
        "bench": "slice_c3_mix",
        "K": K, "features_sliced": len(feats), "updates_per_step": updates,
        "hp_slice_step_ms_median": round(step_ms, 4), "hp_slice_step_ms_min": round(float(np.min(ms)), 4),
        "hp_slice_call_ms_median": round(float(np.median(call_ms)), 4),
        "evaluations_per_step_mean": round(evals_per_step, 1),
        "evaluations_per_update_mean": round(evals_per_step / updates, 2),
        "steps_timed": args.steps,
        "host_route_ms_per_evaluation_measured": round(per_eval_ms, 4), "host_route_sample": len(picks),
        "host_route_step_ms_EXTRAPOLATED": round(host_ms, 2),
        "speedup_vs_host_route": round(host_ms / step_ms, 1),
        "theta_slice_16x%d_ms_median" % K: round(float(np.median(tms)), 4),
        "theta_evaluations_per_slot_mean": round(float(np.mean(tev[args.warmup:])) / (16 * K), 2),
    }
    print(json.dumps(res))


if __name__ == "__main__":
    main()
