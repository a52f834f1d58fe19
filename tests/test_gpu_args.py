"""Every tensor and row range the Python binding hands the library is checked first (common_amd/_args.py): a table of
(method, bad argument) pairs over one tiny state, each of which must raise ValueError before anything is launched and
leave the state as it was; then one valid call of each method."""
import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests.gpu_helpers import make_feature, recarray_of

pytestmark = pytest.mark.gpu

N, K = 64, 4


def bad_flat(good):
    """a host copy, a numpy array, another dtype, one element short, every other element of twice as many"""
    wrong = torch.int64 if good.dtype != torch.int64 else torch.int32
    return [("host", good.cpu()), ("numpy", good.cpu().numpy()), ("dtype", good.to(wrong)),
            ("strided", torch.cat([good.reshape(-1)] * 2)[::2]), ("short", good.reshape(-1)[:-1].clone())]


def bad_matrix(good, rows, cols):
    """bad_flat's, and a matrix one column short and a 1-D tensor of `rows` entries"""
    dev, dt = good.device, good.dtype
    return [(k, v) for k, v in bad_flat(good) if k != "short"] + [
        ("rows-1", torch.zeros((rows - 1, cols), dtype=dt, device=dev)),
        ("cols-1", torch.zeros((rows, cols - 1), dtype=dt, device=dev)),
        ("1-D of rows", torch.zeros(rows, dtype=dt, device=dev)),
        ("transposed", torch.zeros((cols, rows), dtype=dt, device=dev).T)]


def test_bad_arguments_raise_before_anything_runs_and_valid_ones_still_work(gpu_ctx):
    import common_amd
    import scipy.sparse as sp
    ctx, dev = gpu_ctx, gpu_ctx.torch_device
    rng = np.random.default_rng(5)
    feats = [make_feature(orc.NICH, N, K, rng), make_feature(orc.BB, N, K, rng)]
    view = common_amd.DataView.from_recarray(ctx, recarray_of(feats))
    st = common_amd.State(ctx, [(orc.NICH, 0), (orc.BB, 0)], K)
    for i, f in enumerate(feats):
        st.set_hp(i, f["hp"])
    st.set_alpha(1.5)
    z0 = rng.integers(0, K - 1, N).astype(np.int32)               # (the last group stays empty)
    z = torch.from_numpy(z0).to(dev)
    st.accumulate(view, z)
    grid = st.hp_grid(1, np.array([[1.0, 1.0], [2.0, 0.5], [0.5, 2.0]], np.float32))
    zm = common_amd.ZMatrix(ctx, N, K)
    zm.add(z)
    shape, Ks = (4, 5), (2, 3)
    rel = common_amd.RelationView(ctx, rng.normal(size=shape).astype(np.float32))
    dense = np.where(rng.random(shape) < 0.5, rng.normal(size=shape), 0.0).astype(np.float32)
    srel = common_amd.SparseRelationView(ctx, sp.csr_matrix(dense))
    ens = common_amd.ChainEnsemble(ctx, [(orc.NICH, 0), (orc.BB, 0)], K, 2, alpha=1.5, hps=[f["hp"] for f in feats])
    ens.assign(view, z)
    ctx.synchronize()

    def snapshot():
        ctx.synchronize()
        return [st.get_ss(0).tobytes(), st.get_ss(1).tobytes(), st.get_group_counts().tobytes(), z.cpu().numpy().tobytes(),
                ens.z.cpu().numpy().tobytes(), zm.nsamples]
    before, steps_before = snapshot(), st.sweep_step_stats()

    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)                      # noqa: E731
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)                   # noqa: E731
    slots = torch.ones(K, dtype=torch.uint8, device=dev)
    zrel = [i32(n) for n in shape]
    col = torch.zeros(N, dtype=torch.float32, device=dev)
    mask = torch.zeros(N, dtype=torch.bool, device=dev)

    # (what the argument is, a good one, the bad ones made of it, the call)
    rows_calls = {                                                # every method that takes (view, ..., row0, nrows)
        "score_value": lambda **kw: st.score_value(view, **kw),
        "score_tune": lambda **kw: st.score_tune(view, f32(N, K), **kw),
        "accumulate": lambda **kw: st.accumulate(view, z, **kw),
        "sweep_assign": lambda **kw: st.sweep_assign(view, z, 1, 0, **kw),
        "sweep_step": lambda **kw: st.sweep_step(view, z, 1, 0, **kw),
        "sweep_step_begin": lambda **kw: st.sweep_step_begin(view, z, 1, 0, **kw),
        "sweep_sequential": lambda **kw: st.sweep_sequential(view, z, 1, 0, **kw),
        "blocked_assign": lambda **kw: st.blocked_assign(view, z, 1, 0, **kw),
        "sweep_blocked": lambda **kw: st.sweep_blocked(view, z, 1, 0, **kw),
        "split_merge": lambda **kw: st.split_merge(view, z, 1, 0, **kw),
        "predictive_logp": lambda **kw: st.predictive_logp(view, **kw),
        "sample_predictive": lambda **kw: st.sample_predictive(view, **kw),
        "chains.sweep": lambda **kw: ens.sweep(view, 1, 1, **kw),
    }
    z_calls = {                                                   # every method that takes z: int32, one entry a row
        "score_value": lambda t: st.score_value(view, z=t),
        "accumulate": lambda t: st.accumulate(view, t),
        "entity_op": lambda t: st.entity_op(view, N - 1, 0, join=False, z=t),
        "sweep_assign": lambda t: st.sweep_assign(view, t, 1, 0),
        "sweep_step": lambda t: st.sweep_step(view, t, 1, 0),
        "sweep_step_begin": lambda t: st.sweep_step_begin(view, t, 1, 0),
        "sweep_sequential": lambda t: st.sweep_sequential(view, t, 1, 0),
        "blocked_assign": lambda t: st.blocked_assign(view, t, 1, 0),
        "sweep_blocked": lambda t: st.sweep_blocked(view, t, 1, 0),
        "split_merge": lambda t: st.split_merge(view, t, 1, 0),
        "predictive_logp": lambda t: st.predictive_logp(view, z=t),
        "sample_predictive": lambda t: st.sample_predictive(view, z=t),
    }
    table = [("z of " + name, bad_flat(z), fn) for name, fn in z_calls.items()]
    table += [
        ("out of score_value", bad_matrix(f32(N, K), N, K), lambda t: st.score_value(view, out=t)),
        ("out of score_tune", bad_matrix(f32(N, K), N, K), lambda t: st.score_tune(view, t)),
        ("out of score_data", bad_matrix(f32(2, K), 2, K) + [("padded", f32(2, K + 1)[:, :K])], lambda t: st.score_data(out=t)),
        ("out of predictive_logp", bad_flat(f32(N)), lambda t: st.predictive_logp(view, out=t)),
        ("out of sample_predictive", bad_flat(f32(N)), lambda t: st.sample_predictive(view, z=z, out={0: t})),
        ("order of sweep_sequential", bad_flat(i32(N)), lambda t: st.sweep_sequential(view, z, 1, 0, order=t)),
        ("trace of sweep_sequential", bad_flat(i32(2 * N)), lambda t: st.sweep_sequential(view, z, 1, 0, nsweeps=2, trace=t)),
        ("trace of sweep_blocked", bad_flat(i32(2 * N)), lambda t: st.sweep_blocked(view, z, 1, 0, nsweeps=2, trace=t)),
        ("top_slot of sweep_blocked", bad_flat(i32(2)), lambda t: st.sweep_blocked(view, z, 1, 0, nsweeps=2, top_slot=t)),
        ("log of split_merge", bad_flat(torch.zeros(16, dtype=torch.float64, device=dev)),
         lambda t: st.split_merge(view, z, 1, 0, nproposals=2, log=t)),
        ("trace of split_merge", bad_flat(i32(2 * N)), lambda t: st.split_merge(view, z, 1, 0, nproposals=2, trace=t)),
        ("proposed of split_merge", bad_flat(i32(2 * N)), lambda t: st.split_merge(view, z, 1, 0, nproposals=2, proposed=t)),
        ("counters of split_merge", bad_flat(torch.zeros(5, dtype=torch.int64, device=dev)),
         lambda t: st.split_merge(view, z, 1, 0, counters=t)),
        ("out of HpGrid.scores", bad_flat(torch.zeros(3, dtype=torch.float64, device=dev)), lambda t: grid.scores(out=t)),
        ("slots of HpGrid.scores", bad_flat(slots), lambda t: grid.scores(slots=t)),
        ("slots of hp_gibbs", bad_flat(slots), lambda t: st.hp_gibbs([grid], 1, 0, slots=t)),
        ("slots of hp_slice", bad_flat(slots), lambda t: st.hp_slice([{"feature": "alpha", "width": 1.0}], 1, 0, slots=t)),
        ("slots of theta_slice", bad_flat(slots), lambda t: st.theta_slice({}, 1, 0, slots=t)),
        ("z of ZMatrix.add", bad_flat(i32(N)), zm.add),
        ("cands of partition_sums", bad_flat(i32(N)), zm.partition_sums),
        ("cands of partition_loss", bad_flat(i32(N)), zm.partition_loss),
        ("starts of partition_refine", bad_flat(i32(N)), zm.partition_refine),
        ("out of ZMatrix.counts", bad_matrix(torch.zeros((N, N), dtype=torch.int32, device=dev), N, N),
         lambda t: zm.counts(out=t)),
        ("out of ZMatrix.result", bad_matrix(f32(N, N), N, N), lambda t: zm.result(out=t)),
        ("z of linkage_single", bad_matrix(f32(8, 8), 8, 8) + [("not square", f32(8, 9))], ctx.linkage_single),
        ("a of partition_distances", [(k, v) for k, v in bad_flat(i32(N)) if k != "short"], ctx.partition_distances),
        ("b of partition_distances", bad_flat(i32(N)), lambda t: ctx.partition_distances(z, t)),
        ("zs of RelationView.blocks", bad_flat(zrel[1]), lambda t: rel.blocks([zrel[0], t], Ks)),
        ("zs of SparseRelationView.blocks", bad_flat(zrel[1]), lambda t: srel.blocks([zrel[0], t], Ks)),
        ("scores of RelationView.slice_scores", bad_matrix(f32(20, 6), 20, 6), lambda t: rel.slice_scores(t, i32(20), 0, Ks)),
        ("off of RelationView.slice_scores", bad_flat(i32(20)), lambda t: rel.slice_scores(f32(20, 6), t, 0, Ks)),
        ("scores of SparseRelationView.slice_scores", bad_matrix(f32(srel.nnz(), 6), srel.nnz(), 6),
         lambda t: srel.slice_scores(t, i32(srel.nnz()), 0, Ks)),
        ("off of SparseRelationView.slice_scores", bad_flat(i32(srel.nnz())),
         lambda t: srel.slice_scores(f32(srel.nnz(), 6), t, 0, Ks)),
        ("columns of from_tensors", [(k, v) for k, v in bad_flat(col) if k in ("host", "numpy", "strided")],
         lambda t: common_amd.DataView.from_tensors(ctx, [col, t])),
        ("masks of from_tensors", bad_flat(mask), lambda t: common_amd.DataView.from_tensors(ctx, [col, col], masks=[None, t])),
        ("order of chains.sweep", bad_flat(i32(N)), lambda t: ens.sweep(view, 1, 1, order=t)),
        ("z of chains.assign", [(k, v) for k, v in bad_flat(i32(N)) if k in ("dtype", "short")], lambda t: ens.assign(view, t)),
    ]
    assert srel.nnz() > 1
    checked = 0
    for what, bads, call in table:
        assert len(bads) >= 2, what
        for kind, bad in bads:
            with pytest.raises(ValueError):
                call(bad)
                pytest.fail("%s: a %s tensor was accepted" % (what, kind), pytrace=False)
            checked += 1
    for name, call in rows_calls.items():
        for kw in (dict(row0=N + 1), dict(nrows=-1), dict(row0=-1, nrows=1)):
            with pytest.raises(ValueError):
                call(**kw)
                pytest.fail("%s: %s was accepted" % (name, kw), pytrace=False)
            checked += 1
    with pytest.raises(ValueError):
        st.entity_op(view, -1, 0)
    with pytest.raises(ValueError):
        common_amd.DataView.from_tensors(ctx, [col, col], masks=[mask])              # one entry a column
    assert checked > 200
    assert snapshot() == before and st.sweep_step_stats() == steps_before            # nothing ran

    # ---- one valid call of each, with the smallest valid arguments ----
    assert st.score_value(view).shape == (N, K)
    padded, line = f32(N, K + 3), f32(N * K)
    want = st.score_value(view, z=z)
    assert torch.equal(st.score_value(view, out=padded[:, :K], z=z), want) and not padded[:, K:].any()
    st.score_value(view, out=line, z=z)
    assert torch.equal(line.view(N, K), want)
    st.score_tune(view, f32(N, K))
    assert st.score_data(out=f32(2, K)).shape == (2, K)
    assert st.predictive_logp(view, z=z, out=f32(N)).shape == (N,)
    st.sample_predictive(view, z=z, out={0: f32(N)})
    z2 = z.clone()
    st.entity_op(view, 0, int(z0[0]), join=False, z=z2)
    st.entity_op(view, 0, int(z0[0]), join=True, z=z2)
    ctx.synchronize()
    assert torch.equal(z2, z) and st.get_group_counts().tobytes() == before[2]
    st.accumulate(view, z2)
    st.sweep_assign(view, z2, 1, 0)
    st.accumulate(view, z2)
    st.sweep_step(view, z2, 1, 1)
    st.sweep_step_begin(view, z2, 1, 2)
    st.commit_reduce()
    st.sweep_sequential(view, z2, 1, 3, nsweeps=2, order=torch.arange(N, dtype=torch.int32, device=dev), trace=i32(2 * N))
    st.blocked_draw(1, 5)
    st.blocked_assign(view, z2, 1, 5)
    st.accumulate(view, z2)
    st.sweep_blocked(view, z2, 1, 6, nsweeps=2, trace=i32(2 * N), top_slot=i32(2))
    st.split_merge(view, z2, 1, 8, nproposals=2, log=torch.zeros(16, dtype=torch.float64, device=dev), trace=i32(2 * N),
                   proposed=i32(2 * N), counters=torch.zeros(5, dtype=torch.int64, device=dev))
    assert grid.scores(slots=slots, out=torch.zeros(3, dtype=torch.float64, device=dev)).shape == (3,)
    assert st.hp_gibbs([grid], 1, 9, slots=slots)[0] < 3
    st.hp_slice([{"feature": "alpha", "width": 1.0, "prior": "exponential", "a": 1.0}], 1, 10, slots=slots)
    zm.add(torch.stack([z, z2]))
    zm.partition_sums(z)
    zm.partition_loss(z)
    zm.partition_refine(z)
    assert zm.counts(out=torch.zeros((N, N + 1), dtype=torch.int32, device=dev)).shape == (N, N)
    res = zm.result(out=f32(N, N))
    assert ctx.linkage_single(res)[0].shape == (N - 1, 4)
    assert ctx.partition_distances(z, torch.stack([z, z2]))[0].shape == (1, 2)
    for r, ncells in ((rel, 20), (srel, srel.nnz())):
        assert r.blocks(zrel, Ks).shape == (ncells,)
        assert r.slice_scores(f32(ncells, 6), r.slice_offsets(zrel, Ks, 0), 0, Ks).shape == (shape[0], Ks[0])
    tv = common_amd.DataView.from_tensors(ctx, [col, mask], masks=[mask, None])
    assert tv.nrows == N
    ens.assign(view, z0)
    assert ens.sweep(view, 1, 1, order=torch.arange(N, dtype=torch.int32, device=dev), trace_every=1).shape == (2, 1, N)
    ctx.synchronize()
    for o in (tv, ens, zm, grid, st, view):
        o.close()
