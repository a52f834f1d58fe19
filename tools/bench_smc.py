"""Cost of the particle filter over rows (ChainEnsemble.visit / clone / smc) on one nich column, K = 64, N = 4096, 256
particles.  Prints one JSON line per measurement and, with --out, appends them to that file.

  outputs   ens.visit of all rows with the log weights and the per-visit increments set, against ens.sweep of the same
            rows from the same all-unassigned start: alternated, median of --repeats each, device events around the call
  smc       a whole ens.smc() with the default block: host clock around the call ending in a synchronise (median of
            --repeats), the checkpoints that resampled, and where the host clock went inside one more run whose visit /
            read-back / resampling / clone steps each end in a synchronise (that run is slower than the plain one: its
            shares, not its total, are the figure).  Kernel shares come from a trace of `--only smc`:
              rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_smc.py --only smc --repeats 1
  spread    the standard deviation of log_evidence over --seeds seeds, at 64 and at 256 particles

    python tools/bench_smc.py [--rows 4096] [--groups 64] [--particles 256] [--repeats 5] [--seeds 8] [--only outputs,smc,spread]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import common_amd  # noqa: E402
from common_amd import NICH  # noqa: E402
from common_amd import smc as S  # noqa: E402
from tools.bench_configs import make_columns  # noqa: E402

SPEC = [(NICH, 0)]


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as fh:
            fh.write(line + "\n")


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def outputs(ctx, view, N, K, P, repeats):
    ens = common_amd.ChainEnsemble(ctx, SPEC, K, P, alpha=1.0)
    visit_ms, sweep_ms = [], []
    for r in range(repeats + 1):                            # (the first round is the warm-up)
        ens.seat(view)
        torch.cuda.synchronize()
        visit_ms.append(event_ms(lambda: ens.visit(view, 0, N, 1000, sweep=r, want_logp=True)))
        ens.seat(view)
        torch.cuda.synchronize()
        sweep_ms.append(event_ms(lambda: ens.sweep(view, 1, 1000, sweep=r)))
    ens.close()
    v, s = statistics.median(visit_ms[1:]), statistics.median(sweep_ms[1:])
    return dict(what="outputs", N=N, K=K, particles=P, repeats=repeats, visit_ms=[round(x, 3) for x in visit_ms[1:]],
                sweep_ms=[round(x, 3) for x in sweep_ms[1:]], visit_ms_median=round(v, 3), sweep_ms_median=round(s, 3),
                visit_over_sweep=round(v / s, 4), us_per_visit_per_chain=round(v * 1e3 / N, 3))


def smc_run(ctx, view, N, K, P, repeats):
    ens = common_amd.ChainEnsemble(ctx, SPEC, K, P, alpha=1.0)
    wall, res = [], None
    for r in range(repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = ens.smc(view, 2000 + r)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    rec = dict(what="smc", N=N, K=K, particles=P, block=max(1, N // 64), checkpoints=len(res.ess) - 1,
               resampled=len(res.resampled_at), log_evidence=round(res.log_evidence, 4), truncated=res.truncated,
               wall_ms=[round(x, 2) for x in wall[1:]], wall_ms_median=round(statistics.median(wall[1:]), 2) if repeats else None)
    # where the host clock goes: the same steps by hand, every one ending in a synchronise
    block, t = max(1, N // 64), dict(seat=0.0, visit=0.0, readback=0.0, host=0.0, clone=0.0, rebuild_and_visit_after_clone=0.0)
    rng = np.random.Generator(np.random.Philox(key=7))

    def timed(key, fn):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        t[key] += (time.perf_counter() - t0) * 1e3
        return out

    timed("seat", lambda: ens.seat(view))
    cloned = False
    for pos0 in range(0, N, block):
        npos = min(block, N - pos0)
        timed("rebuild_and_visit_after_clone" if cloned else "visit", lambda: ens.visit(view, pos0, npos, 2000))
        cloned = False
        if pos0 + npos == N:
            break
        logw = timed("readback", lambda: ens.logw.cpu().numpy())
        t0 = time.perf_counter()
        a = S.systematic_ancestors(logw, rng.random()) if S.ess(logw) < 0.5 * P else None
        t["host"] += (time.perf_counter() - t0) * 1e3
        if a is not None:
            timed("clone", lambda: (ens.clone(a), ens.logw.zero_()))
            cloned = True
    ens.close()
    rec["stepwise_ms"] = {k: round(v, 2) for k, v in t.items()}
    return rec


def spread(ctx, view, N, K, seeds):
    out = []
    for P in (64, 256):
        ens = common_amd.ChainEnsemble(ctx, SPEC, K, P, alpha=1.0)
        logz = [ens.smc(view, 9000 + 1000 * s).log_evidence for s in range(seeds)]
        ens.close()
        out.append(dict(what="spread", N=N, K=K, particles=P, seeds=seeds, log_evidence_mean=round(float(np.mean(logz)), 4),
                        log_evidence_std=round(float(np.std(logz, ddof=1)), 4),
                        log_evidence=[round(x, 4) for x in logz]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--groups", type=int, default=64)
    ap.add_argument("--particles", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seeds", type=int, default=8)
    ap.add_argument("--only", default="outputs,smc,spread")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = common_amd.Context(device=0)
    cols, _ = make_columns(ctx, SPEC, a.rows, 8, seed=73)          # (eight well separated clusters in the data)
    view = common_amd.DataView.from_tensors(ctx, cols)
    only = a.only.split(",")
    emit(dict(what="setup", device=torch.cuda.get_device_name(0), N=a.rows, K=a.groups, particles=a.particles), a.out)
    if "outputs" in only:
        emit(outputs(ctx, view, a.rows, a.groups, a.particles, a.repeats), a.out)
    if "smc" in only:
        emit(smc_run(ctx, view, a.rows, a.groups, a.particles, a.repeats), a.out)
    if "spread" in only:
        for rec in spread(ctx, view, a.rows, a.groups, a.seeds):
            emit(rec, a.out)


if __name__ == "__main__":
    main()
