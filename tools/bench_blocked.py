"""Time of one blocked Gibbs sweep (msc_sweep_blocked: draw + assign + accumulate) beside one batched synchronous sweep
(msc_sweep_step) on the same data, warm, one sweep a call, device events around every call:
    C2        one nich column, N = 1e6, K = 256
    C3        the mix bb + gp + dd(32) + nich x 16 (D = 64), N = 1e6, K = 256
    C5 shard  one nich column, N = 12.5e6, K = 1024
    C4        one niw column of dim 32, N = 262144, K = 128 (c4d16: dim 16) -- the Dirichlet-process Gaussian mixture;
              beside the niw scoring pass (msc_score_value), the unchanged code the assign pass is measured against
with the blocked sweep's split into draw / assign / accumulate (each timed on its own, the assign against a standing
draw) and, for the pass-by-pass comparison, the collapsed fused assignment pass alone (msc_sweep_assign).  With
--occupied: on N = 2e4 rows of the small C3 mix (bb, gp, dd(9), nich) from eight true clusters with K = 64, the occupied
groups after 50 sweeps of sweep_blocked and of sweep_sequential (recorded, not asserted).  Writes everything to --out.

    python tools/bench_blocked.py [c2] [c3] [c5] [--steps 10] [--occupied] [--out profiles/blocked.txt]
    python tools/bench_blocked.py c4 c4d16 --out profiles/blocked_niw.txt     (the measured lines of that file)
"""
import argparse
import datetime
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import common_amd  # noqa: E402
from common_amd import BB, DD, GP, NICH, NIW  # noqa: E402
from tools.bench_configs import make_columns  # noqa: E402

SHAPES = {
    "c2": ("C2 nich N=1e6 K=256", [(NICH, 0)], 1_000_000, 256),
    "c3": ("C3 mix bb+gp+dd32+nich x16 N=1e6 K=256", [(BB, 0), (GP, 0), (DD, 32), (NICH, 0)] * 16, 1_000_000, 256),
    "c5": ("C5 shard nich N=12.5e6 K=1024", [(NICH, 0)], 12_500_000, 1024),
    "c4": ("C4 niw dim=32 N=262144 K=128", [(NIW, 32)], 262_144, 128),
    "c4d16": ("C4 niw dim=16 N=262144 K=128", [(NIW, 16)], 262_144, 128),
}


def timed(fn, steps, warmup=2):
    """(mean, min) milliseconds of fn(i) over `steps` warm calls, device events around each"""
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    ms = []
    for i in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(warmup + i)
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return sum(ms) / len(ms), min(ms)


def shape(ctx, key, steps):
    name, spec, N, K = SHAPES[key]
    cols, z = make_columns(ctx, spec, N, K, 73)
    view = common_amd.DataView.from_tensors(ctx, cols)
    res = dict(shape=name, N=N, K=K, D=len(spec))
    # the batched synchronous sweep, as it stands
    st = common_amd.State(ctx, spec, K)
    st.set_alpha(1.0)
    zs = z.clone()
    st.accumulate(view, zs)
    avg, mn = timed(lambda i: st.sweep_step(view, zs, 73, i), steps)
    res.update(sweep_step_ms=round(avg, 4), sweep_step_ms_min=round(mn, 4))
    st.accumulate(view, zs)
    avg, mn = timed(lambda i: st.sweep_assign(view, zs, 73, 1000 + i), steps)
    res.update(collapsed_assign_ms=round(avg, 4))
    if any(f == NIW for f, _ in spec):
        st.accumulate(view, zs)
        out = torch.empty((N, K), dtype=torch.float32, device=ctx.torch_device)
        avg, mn = timed(lambda i: st.score_value(view, out=out), steps)
        res.update(score_value_ms=round(avg, 4), score_value_ms_min=round(mn, 4), score_kernel=ctx.lib.msc_last_kernel(0).decode())
        del out
    del st
    # the blocked sweep
    sb = common_amd.State(ctx, spec, K)
    sb.set_alpha(1.0)
    zb = z.clone()
    sb.accumulate(view, zb)
    avg, mn = timed(lambda i: sb.sweep_blocked(view, zb, 73, i), steps)
    res.update(sweep_blocked_ms=round(avg, 4), sweep_blocked_ms_min=round(mn, 4))
    avg, _ = timed(lambda i: sb.blocked_draw(73, 500 + i), steps)
    res.update(draw_ms=round(avg, 4))
    zt = zb.clone()
    avg, _ = timed(lambda i: sb.blocked_assign(view, zt, 73, 500 + steps + 1), steps)
    res.update(assign_ms=round(avg, 4), assign_kernel=ctx.lib.msc_last_kernel(1).decode())
    avg, _ = timed(lambda i: sb.accumulate(view, zb), steps)
    res.update(accumulate_ms=round(avg, 4))
    res.update(blocked_rows_per_s=round(N / (res["sweep_blocked_ms"] * 1e-3)),
               step_rows_per_s=round(N / (res["sweep_step_ms"] * 1e-3)),
               assign_vs_collapsed_assign=round(res["assign_ms"] / res["collapsed_assign_ms"], 3),
               blocked_vs_step=round(res["sweep_blocked_ms"] / res["sweep_step_ms"], 3))
    if "score_value_ms" in res:
        res.update(assign_vs_score_value=round(res["assign_ms"] / res["score_value_ms"], 3))
    return res


def occupied(ctx, N=20000, K=64, true_clusters=8, sweeps=50):
    spec = [(BB, 0), (GP, 0), (DD, 9), (NICH, 0)]
    cols, _ = make_columns(ctx, spec, N, true_clusters, 5)
    view = common_amd.DataView.from_tensors(ctx, cols)
    out = dict(shape="small C3 mix, N=%d, %d true clusters, K=%d, %d sweeps from one group" % (N, true_clusters, K, sweeps))
    for kind in ("blocked", "sequential"):
        st = common_amd.State(ctx, spec, K)
        st.set_alpha(1.0)
        z = torch.zeros(N, dtype=torch.int32, device=ctx.torch_device)
        st.accumulate(view, z)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        if kind == "blocked":
            st.sweep_blocked(view, z, 11, 0, nsweeps=sweeps)
        else:
            st.sweep_sequential(view, z, 11, 0, nsweeps=sweeps)
        b.record()
        torch.cuda.synchronize()
        cnt = st.get_group_counts()
        out[kind] = dict(occupied=int((cnt > 0).sum()), groups_over_1pct=int((cnt > N // 100).sum()),
                         ms=round(a.elapsed_time(b), 2))
    return out


def commit_id():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL,
                                       text=True).strip()
    except Exception:
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", default=[])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--occupied", action="store_true")
    ap.add_argument("--commit", default=None, help="the parent commit the figures are measured beside (default: git's HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blocked.txt"))
    a = ap.parse_args()
    ctx = common_amd.Context(device=0)
    lines = ["# Blocked Gibbs sweep (msc_sweep_blocked) beside the batched synchronous sweep (msc_sweep_step): %s, %s, "
             "parent commit %s" % (torch.cuda.get_device_name(0), datetime.date.today().isoformat(), a.commit or commit_id()),
             "# mean of %d warm calls, one sweep a call, device events around each call; draw / assign / accumulate timed "
             "on their own" % a.steps]
    for key in (a.shapes or ["c2", "c3", "c5"]):
        r = shape(ctx, key, a.steps)
        print(json.dumps(r), flush=True)
        lines.append(json.dumps(r))
        torch.cuda.empty_cache()
    if a.occupied:
        r = occupied(ctx)
        print(json.dumps(r), flush=True)
        lines.append(json.dumps(r))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
