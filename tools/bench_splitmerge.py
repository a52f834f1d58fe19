"""Time of split-merge proposals (msc_split_merge) beside one batched synchronous sweep (msc_sweep_step) of the same
state, warm, device events around every call:
    C2   one nich column, N = 1e6, K = 256
    C3   the mix bb + gp + dd(32) + nich x 16 (D = 64), N = 1e6, K = 256
for launch_iters 0, 2 and 5: the time per proposal (calls of --proposals proposals), what one launch pass adds (the slope
over launch_iters: accumulate + draw + restricted assign of the two pair slots), what is left (anchors, coins, the final
accumulate, score_data, decision, relabel), the state's own accumulate pass and parameter draw for scale, and the
acceptance rates.  With --clusters: section 6j's experiment -- N = 2e4 rows of the small C3 mix (bb, gp, dd(9), nich) from
eight true clusters, K = 64, all rows in one group -- 50 x (sweep_step, 8 proposals) against 50 x sweep_step alone: the
occupied groups and the groups above 1 % of the rows (recorded, not asserted).  Writes everything to --out.

    python tools/bench_splitmerge.py [c2] [c3] [--steps 10] [--proposals 8] [--clusters] [--out profiles/splitmerge.txt]
"""
import argparse
import datetime
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import common_amd  # noqa: E402
from common_amd import BB, DD, GP, NICH  # noqa: E402
from tools.bench_blocked import commit_id, timed  # noqa: E402
from tools.bench_configs import make_columns  # noqa: E402

SHAPES = {
    "c2": ("C2 nich N=1e6 K=256", [(NICH, 0)], 1_000_000, 256),
    "c3": ("C3 mix bb+gp+dd32+nich x16 N=1e6 K=256", [(BB, 0), (GP, 0), (DD, 32), (NICH, 0)] * 16, 1_000_000, 256),
}
LAUNCH_ITERS = (0, 2, 5)


def shape(ctx, key, steps, nprop):
    name, spec, N, K = SHAPES[key]
    cols, z = make_columns(ctx, spec, N, K, 73)
    view = common_amd.DataView.from_tensors(ctx, cols)
    res = dict(shape=name, N=N, K=K, D=len(spec), proposals_per_call=nprop)
    st = common_amd.State(ctx, spec, K)
    st.set_alpha(1.0)
    zs = z.clone()
    st.accumulate(view, zs)
    avg, _ = timed(lambda i: st.sweep_step(view, zs, 73, i), steps)
    res.update(sweep_step_ms=round(avg, 4))
    avg, _ = timed(lambda i: st.accumulate(view, zs), steps)
    res.update(accumulate_ms=round(avg, 4))
    avg, _ = timed(lambda i: st.blocked_draw(73, i), steps)
    res.update(draw_ms=round(avg, 4))
    per = {}
    for li in LAUNCH_ITERS:
        cnt = torch.zeros(5, dtype=torch.int64, device=ctx.torch_device)
        zp = zs.clone()
        st.accumulate(view, zp)
        avg, _ = timed(lambda i: st.split_merge(view, zp, 73, 10000 * (li + 1) + i * nprop, nproposals=nprop, launch_iters=li,
                                                counters=cnt), steps)
        # (a call ends with one accumulate of the whole state: taken out of the per-proposal figure)
        per[li] = (avg - res["accumulate_ms"]) / nprop
        c = cnt.cpu().tolist()
        res["launch_iters_%d" % li] = dict(ms_per_proposal=round(per[li], 4), ms_per_call=round(avg, 4), splits=c[0],
                                           splits_accepted=c[1], merges=c[2], merges_accepted=c[3], void=c[4],
                                           assign_kernel=ctx.lib.msc_last_kernel(1).decode())
    slope = (per[5] - per[0]) / 5.0
    res.update(ms_per_launch_pass=round(slope, 4), ms_fixed_per_proposal=round(per[0] - slope, 4),
               proposal_vs_sweep_step=round(per[2] / res["sweep_step_ms"], 3))
    return res


def clusters(ctx, N=20000, K=64, true_clusters=8, rounds=50, nprop=8):
    spec = [(BB, 0), (GP, 0), (DD, 9), (NICH, 0)]
    cols, _ = make_columns(ctx, spec, N, true_clusters, 5)
    view = common_amd.DataView.from_tensors(ctx, cols)
    out = dict(shape="small C3 mix, N=%d, %d true clusters, K=%d, %d rounds from one group" % (N, true_clusters, K, rounds))
    for kind in ("sweep_step", "sweep_step+split_merge"):
        st = common_amd.State(ctx, spec, K)
        st.set_alpha(1.0)
        z = torch.zeros(N, dtype=torch.int32, device=ctx.torch_device)
        st.accumulate(view, z)
        cnt = torch.zeros(5, dtype=torch.int64, device=ctx.torch_device)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for r in range(rounds):
            st.sweep_step(view, z, 11, r)
            if kind != "sweep_step":
                st.split_merge(view, z, 11, r * nprop, nproposals=nprop, launch_iters=2, counters=cnt)
        b.record()
        torch.cuda.synchronize()
        c = st.get_group_counts()
        out[kind] = dict(occupied=int((c > 0).sum()), groups_over_1pct=int((c > N // 100).sum()),
                         ms=round(a.elapsed_time(b), 2), counters=cnt.cpu().tolist())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", default=[])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--proposals", type=int, default=8)
    ap.add_argument("--clusters", action="store_true")
    ap.add_argument("--commit", default=None, help="the parent commit the figures are measured beside (default: git's HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "splitmerge.txt"))
    a = ap.parse_args()
    ctx = common_amd.Context(device=0)
    lines = ["# Split-merge proposals (msc_split_merge) beside the batched synchronous sweep (msc_sweep_step): %s, %s, parent "
             "commit %s" % (torch.cuda.get_device_name(0), datetime.date.today().isoformat(), a.commit or commit_id()),
             "# mean of %d warm calls of %d proposals, device events around each call; the call's closing accumulate taken "
             "out of the per-proposal figures" % (a.steps, a.proposals)]
    for key in (a.shapes or ["c2", "c3"]):
        r = shape(ctx, key, a.steps, a.proposals)
        print(json.dumps(r), flush=True)
        lines.append(json.dumps(r))
        torch.cuda.empty_cache()
    if a.clusters:
        r = clusters(ctx)
        print(json.dumps(r), flush=True)
        lines.append(json.dumps(r))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
