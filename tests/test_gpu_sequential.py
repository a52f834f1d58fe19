"""GPU: the sequential collapsed Gibbs sweep (msc_sweep_sequential) -- replayed against the double oracle visit by visit,
its tables on return, the exact posterior of a few rows, and its agreement with the other paths."""
import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import seq_helpers as sh
from tests.gpu_helpers import TOL, make_feature, recarray_of, rel_err

pytestmark = pytest.mark.gpu

C3_SMALL = [(orc.BB, 0), (orc.GP, 0), (orc.DD, 9), (orc.NICH, 0)]


def _setup(gpu_ctx, specs, N, K, seed, alpha=1.3, masked=False, gp_large=False, empty=2, z=None):
    """features, a view, a state accumulated from z on the device, and the replay's features"""
    import common_amd
    rng = np.random.default_rng(seed)
    feats = [make_feature(f, N, max(K, 2), rng, d) for f, d in specs]
    if gp_large:        # counts beyond the exact table (kGpMaxTable = 1024)
        for f in feats:
            if f["family"] in (orc.GP, orc.BNB):
                f["values"] = f["values"].copy()
                f["values"][::37] = rng.integers(1024, 3000, len(f["values"][::37])).astype(np.uint32)
    masks = [rng.random(N) < 0.2 for _ in feats] if masked else [None] * len(feats)
    data = recarray_of(feats)
    if masked:
        mask = np.zeros(N, dtype=[(n, np.bool_) for n in data.dtype.names])
        for i, m in enumerate(masks):
            mask["f%d" % i] = m
        data = np.ma.masked_array(data, mask=mask)
    view = common_amd.DataView.from_recarray(gpu_ctx, data)
    st = common_amd.State(gpu_ctx, [(f["family"], f["dim"]) for f in feats], K)
    Fs = [orc.Family(f["family"], f["hp"], f["dim"], "f64") for f in feats]
    for i, F in enumerate(Fs):
        st.set_hp(i, F.hp)
    st.set_alpha(alpha)
    if z is None:
        z = rng.integers(0, max(1, K - empty), N).astype(np.int32)
    st.accumulate(view, torch.from_numpy(z).to(gpu_ctx.torch_device))
    return dict(view=view, st=st, z=z, alpha=alpha, K=K, N=N,
                rfeats=[(F, f["values"], m) for F, f, m in zip(Fs, feats, masks)])


def _run_and_replay(gpu_ctx, s, seed, sweep, nsweeps=1, order=None, row0=0, nrows=None, row_id0=None):
    dev = gpu_ctx.torch_device
    N, K = s["N"], s["K"]
    n = N - row0 if nrows is None else nrows
    rid0 = row0 if row_id0 is None else row_id0
    zt = torch.from_numpy(s["z"][row0:row0 + n].copy()).to(dev)
    trace = torch.full((nsweeps * n,), -7, dtype=torch.int32, device=dev)
    ot = None if order is None else torch.from_numpy(order.astype(np.int32)).to(dev)
    s["st"].sweep_sequential(s["view"], zt, seed, sweep, nsweeps=nsweeps, order=ot, trace=trace, row0=row0, nrows=n,
                             row_id0=row_id0)
    tr = trace.cpu().numpy().reshape(nsweeps, n)
    assert np.array_equal(tr[-1], zt.cpu().numpy())
    rp = sh.Replay(s["rfeats"], K, s["alpha"], s["z"])
    offs = np.arange(n) if order is None else order
    n_off = 0
    for k in range(nsweeps):
        n_off += rp.sweep(row0 + offs, seed, sweep + k, rid0 + offs, got=tr[k][offs])
        assert np.array_equal(rp.z[row0:row0 + n], tr[k]), k
    assert n_off <= max(3, 0.005 * nsweeps * n), n_off
    return zt, rp


FAMILY_CASES = {
    "bb": dict(specs=[(orc.BB, 0)] * 3),
    "gp": dict(specs=[(orc.GP, 0)]),
    "gp_beyond_table": dict(specs=[(orc.GP, 0), (orc.BB, 0)], gp_large=True),
    "bnb": dict(specs=[(orc.BNB, 0)]),
    "dd2": dict(specs=[(orc.DD, 2)]),
    "dd128": dict(specs=[(orc.DD, 128)]),
    "nich": dict(specs=[(orc.NICH, 0)]),
    "c3_mix": dict(specs=C3_SMALL),
    "masked_mix": dict(specs=C3_SMALL + [(orc.BNB, 0)], masked=True),
}


@pytest.mark.parametrize("case", sorted(FAMILY_CASES))
def test_replay_per_family(gpu_ctx, case):
    c = FAMILY_CASES[case]
    s = _setup(gpu_ctx, c["specs"], 2000, 48, seed=sum(map(ord, case)), masked=c.get("masked", False),
               gp_large=c.get("gp_large", False))
    _run_and_replay(gpu_ctx, s, seed=11, sweep=2)


@pytest.mark.parametrize("K", [1, 2, 7, 64, 65, 256, 257, 1000, 1024])
def test_replay_across_group_counts(gpu_ctx, K):
    s = _setup(gpu_ctx, C3_SMALL, 2000 if K < 1000 else 1200, K, seed=100 + K)
    _run_and_replay(gpu_ctx, s, seed=5 + K, sweep=1)


def test_replay_order_offsets_masks_and_trace(gpu_ctx):
    s = _setup(gpu_ctx, C3_SMALL, 1800, 40, seed=9, masked=True)
    order = np.random.default_rng(4).permutation(1200).astype(np.uint32)
    _run_and_replay(gpu_ctx, s, seed=21, sweep=7, nsweeps=3, order=order, row0=300, nrows=1200, row_id0=50000)


def _compare_tables(gpu_ctx, s, zt_range, row0=0):
    """the state after the call against a fresh state accumulated from the final z"""
    import common_amd
    z = s["z"].copy()
    z[row0:row0 + len(zt_range)] = zt_range
    st, view = s["st"], s["view"]
    fresh = common_amd.State(gpu_ctx, st.features, s["K"])
    for i in range(len(st.features)):
        fresh.set_hp(i, st.get_hp(i))
    fresh.set_alpha(s["alpha"])
    fresh.accumulate(view, torch.from_numpy(z).to(gpu_ctx.torch_device), reset=True)
    assert np.array_equal(st.get_group_counts(), fresh.get_group_counts())
    for i in range(len(st.features)):
        a, b = st.get_ss(i), fresh.get_ss(i)
        for name in a.dtype.names:
            x, y = a[name].astype(np.float64), b[name].astype(np.float64)
            if np.issubdtype(a.dtype[name].base, np.integer):
                assert np.array_equal(x, y), name
            else:
                assert np.all(np.abs(x - y) <= 1e-6 * np.maximum(1.0, np.abs(y))), name
    for crp in (False, True):
        got = st.score_value(view, crp_prior=crp).cpu().numpy()
        want = fresh.score_value(view, crp_prior=crp).cpu().numpy()
        assert rel_err(got, want).max() <= TOL
    return fresh, z


def test_tables_current_on_return(gpu_ctx):
    s = _setup(gpu_ctx, C3_SMALL + [(orc.BNB, 0)], 3000, 96, seed=12, masked=True)
    dev = gpu_ctx.torch_device
    zt = torch.from_numpy(s["z"].copy()).to(dev)
    s["st"].sweep_sequential(s["view"], zt, 3, 0, nsweeps=2)
    fresh, z = _compare_tables(gpu_ctx, s, zt.cpu().numpy())
    # one following batched sweep on each agrees (a dart within rounding of a CDF step may differ)
    za, zb = torch.from_numpy(z.copy()).to(dev), torch.from_numpy(z.copy()).to(dev)
    s["st"].sweep_step(s["view"], za, 8, 4)
    fresh.sweep_step(s["view"], zb, 8, 4)
    assert (za.cpu().numpy() == zb.cpu().numpy()).mean() >= 0.995


def test_exact_posterior_of_six_rows(gpu_ctx):
    """N = 6, K = 7: 2e5 sequential sweeps visit the 203 partitions with the exact posterior's frequencies"""
    import common_amd
    rng = np.random.default_rng(2024)
    dev = gpu_ctx.torch_device
    N, K, alpha, per_call, calls = 6, 7, 1.0, 40000, 5
    datasets = {
        "bb3": [make_feature(orc.BB, N, 2, rng) for _ in range(3)],
        "nich_bb": [make_feature(orc.NICH, N, 2, rng), make_feature(orc.BB, N, 2, rng)],
    }
    datasets["nich_bb"][0]["values"] = np.array([0.2, -0.4, 0.1, 2.5, 2.9, 5.0], dtype=np.float32)
    for name, feats in datasets.items():
        Fs = [orc.Family(f["family"], f["hp"], f["dim"], "f64") for f in feats]
        parts, p = sh.exact_posterior([(F, f["values"]) for F, f in zip(Fs, feats)], alpha)
        view = common_amd.DataView.from_recarray(gpu_ctx, recarray_of(feats))
        st = common_amd.State(gpu_ctx, [(f["family"], f["dim"]) for f in feats], K)
        for i, F in enumerate(Fs):
            st.set_hp(i, F.hp)
        st.set_alpha(alpha)
        zt = torch.full((N,), -1, dtype=torch.int32, device=dev)
        st.accumulate(view, zt)
        trace = torch.empty(per_call * N, dtype=torch.int32, device=dev)
        traces = []
        for c in range(calls):
            st.sweep_sequential(view, zt, 77, c * per_call, nsweeps=per_call, trace=trace)
            traces.append(trace.cpu().numpy().reshape(per_call, N))
        freq = sh.partition_frequencies(np.concatenate(traces), parts)
        tv, kl = sh.tv_kl(freq, p)
        print("exact posterior %s: sequential TV %.4f KL %.5f" % (name, tv, kl))
        assert tv <= 0.05 and kl <= 0.01, (name, tv, kl)


def test_power_two_identical_rows(gpu_ctx):
    """two identical rows, K = 2, 16 uniform-hp bb columns, alpha = 1: P(apart) = 1 / (1 + (4/3)^16) ~ 0.010.  The
    sequential sweep matches it; the batched sweep, whose simultaneous moves swap the rows, does not"""
    import common_amd
    dev = gpu_ctx.torch_device
    D, K, sweeps = 16, 2, 4000
    exact = 1.0 / (1.0 + (4.0 / 3.0) ** D)
    data = np.zeros(2, dtype=[("f%d" % i, np.bool_) for i in range(D)])
    for i in range(D):
        data["f%d" % i] = [True, True]
    view = common_amd.DataView.from_recarray(gpu_ctx, data)

    def state():
        st = common_amd.State(gpu_ctx, [(orc.BB, 0)] * D, K)
        for i in range(D):
            st.set_hp(i, dict(alpha=1.0, beta=1.0))
        st.set_alpha(1.0)
        zt = torch.tensor([0, 1], dtype=torch.int32, device=dev)
        st.accumulate(view, zt)
        return st, zt

    st, zt = state()
    trace = torch.empty(sweeps * 2, dtype=torch.int32, device=dev)
    st.sweep_sequential(view, zt, 5, 0, nsweeps=sweeps, trace=trace)
    tr = trace.cpu().numpy().reshape(sweeps, 2)
    apart_seq = float((tr[:, 0] != tr[:, 1]).mean())
    st, zt = state()
    apart = []
    for k in range(1000):
        st.sweep_step(view, zt, 5, k)
        zz = zt.cpu().numpy()
        apart.append(zz[0] != zz[1])
    apart_batched = float(np.mean(apart))
    print("P(apart): exact %.4f sequential %.4f batched %.4f" % (exact, apart_seq, apart_batched))
    assert abs(apart_seq - exact) <= 0.02
    assert abs(apart_batched - exact) >= 0.2


def test_one_row_agrees_with_sweep_step(gpu_ctx):
    s = _setup(gpu_ctx, C3_SMALL, 1500, 30, seed=31)
    dev = gpu_ctx.torch_device
    import common_amd
    other = common_amd.State(gpu_ctx, s["st"].features, s["K"])
    for i in range(len(other.features)):
        other.set_hp(i, s["st"].get_hp(i))
    other.set_alpha(s["alpha"])
    other.accumulate(s["view"], torch.from_numpy(s["z"]).to(dev))
    for row in (0, 733, 1499):
        z1 = torch.from_numpy(s["z"][row:row + 1].copy()).to(dev)
        z2 = torch.from_numpy(s["z"][row:row + 1].copy()).to(dev)
        s["st"].sweep_sequential(s["view"], z1, 9, 3, row0=row, nrows=1)
        other.sweep_step(s["view"], z2, 9, 3, row0=row, nrows=1)
        got, want = int(z1.item()), int(z2.item())
        if got != want:
            rp = sh.Replay(s["rfeats"], s["K"], s["alpha"], s["z"])
            rp.visit(row, orc.uniform01(9, 3, row), got=got)
        # put both states back to the fixed state for the next row
        for st in (s["st"], other):
            st.accumulate(s["view"], torch.from_numpy(s["z"]).to(dev), reset=True)


def test_unassigned_rows_are_seated_and_tables_consistent(gpu_ctx):
    """a sweep from an all-unassigned z is sequential CRP seating: every row seated, the replay's chain, tables current"""
    s = _setup(gpu_ctx, C3_SMALL, 1000, 1000, seed=41, z=np.full(1000, -1, np.int32))
    zt, _ = _run_and_replay(gpu_ctx, s, seed=13, sweep=0)
    got = zt.cpu().numpy()
    assert ((got >= 0) & (got < s["K"])).all()
    _compare_tables(gpu_ctx, s, got)


def test_every_slot_full_opens_no_group(gpu_ctx):
    K, N = 5, 600
    z = np.arange(N, dtype=np.int32) % K
    s = _setup(gpu_ctx, [(orc.NICH, 0), (orc.BB, 0)], N, K, seed=51, z=z)
    zt, rp = _run_and_replay(gpu_ctx, s, seed=3, sweep=0, nsweeps=2)
    got = zt.cpu().numpy()
    # every group keeps members (120 each at the start): a slot with no pseudocount offered would show as a group the
    # replay does not have, or one the device count disagrees with
    assert np.array_equal(s["st"].get_group_counts(), np.bincount(got, minlength=K).astype(np.uint32))
    assert np.array_equal(rp.cnt, np.bincount(got, minlength=K))
    assert (np.bincount(got, minlength=K) > 0).all()


def test_same_arguments_same_bits_and_split_calls(gpu_ctx):
    dev = gpu_ctx.torch_device
    runs = []
    for way in ("one", "one", "two"):
        s = _setup(gpu_ctx, C3_SMALL, 1500, 50, seed=61)
        zt = torch.from_numpy(s["z"].copy()).to(dev)
        if way == "one":
            s["st"].sweep_sequential(s["view"], zt, 17, 4, nsweeps=2)
        else:
            s["st"].sweep_sequential(s["view"], zt, 17, 4)
            s["st"].sweep_sequential(s["view"], zt, 17, 5)
        runs.append((zt.cpu().numpy(), s["st"].score_value(s["view"], crp_prior=True).cpu().numpy()))
    for z, sc in runs[1:]:
        assert np.array_equal(z, runs[0][0])
        assert np.array_equal(sc.view(np.uint32), runs[0][1].view(np.uint32))


def test_batched_counters_and_stats_untouched(gpu_ctx):
    """the call leaves msc_sweep_step's device (seed, sweep) pair alone: a step that follows it continues the
    batched stream exactly as on a state that never ran the sequential sweep (same tables by construction)"""
    dev = gpu_ctx.torch_device
    s = _setup(gpu_ctx, C3_SMALL, 1200, 40, seed=71)
    st = s["st"]
    zt = torch.from_numpy(s["z"].copy()).to(dev)
    st.sweep_step(s["view"], zt, 23, 0)
    stats = st.sweep_step_stats()
    zs = zt[:100].clone()
    st.sweep_sequential(s["view"], zs, 99, 0, nrows=100)
    assert st.sweep_step_stats() == stats
    # rebuild from the batched step's z, then the next batched step; the twin state does the same without the call
    st.accumulate(s["view"], zt, reset=True)
    import common_amd
    twin = common_amd.State(gpu_ctx, st.features, s["K"])
    for i in range(len(st.features)):
        twin.set_hp(i, st.get_hp(i))
    twin.set_alpha(s["alpha"])
    zt2 = zt.clone()
    twin.accumulate(s["view"], zt2, reset=True)
    st.sweep_step(s["view"], zt, 23, 1)
    twin.sweep_step(s["view"], zt2, 23, 1)
    assert np.array_equal(zt.cpu().numpy(), zt2.cpu().numpy())


@pytest.mark.parametrize("spec", [(orc.NIW, 3), (orc.DM, 4), (orc.BBNC, 0)])
def test_unsupported_families(gpu_ctx, spec):
    import common_amd
    s = _setup(gpu_ctx, [spec, (orc.NICH, 0)], 200, 8, seed=81)
    zt = torch.from_numpy(s["z"].copy()).to(gpu_ctx.torch_device)
    with pytest.raises(common_amd.MicroscopesHipError) as e:
        s["st"].sweep_sequential(s["view"], zt, 1, 0)
    assert e.value.code == -4


def test_errors(gpu_ctx):
    import common_amd
    dev = gpu_ctx.torch_device
    s = _setup(gpu_ctx, C3_SMALL, 500, 20, seed=91)
    st, view = s["st"], s["view"]
    zt = torch.from_numpy(s["z"].copy()).to(dev)
    # between sweep_step_begin and commit_reduce
    st.sweep_step_begin(view, zt, 1, 0)
    with pytest.raises(common_amd.MicroscopesHipError) as e:
        st.sweep_sequential(view, zt, 1, 0)
    assert e.value.code == -1
    st.commit_reduce()
    # bad tensors
    with pytest.raises(ValueError):
        st.sweep_sequential(view, zt.to(torch.int64), 1, 0)
    with pytest.raises(ValueError):
        st.sweep_sequential(view, zt[:10], 1, 0)
    with pytest.raises(ValueError):
        st.sweep_sequential(view, zt, 1, 0, order=torch.arange(500, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError):
        st.sweep_sequential(view, zt, 1, 0, order=torch.arange(10, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        st.sweep_sequential(view, zt, 1, 0, nsweeps=2, trace=torch.empty(500, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        st.sweep_sequential(view, zt, 1, 0, trace=torch.empty(500, dtype=torch.int32))
    with pytest.raises(ValueError):
        st.sweep_sequential(view, zt, 1, 0, nsweeps=1 << 32)
    # an order entry >= nrows: that visit is skipped, the next call reports it (once)
    order = torch.arange(500, dtype=torch.int32, device=dev)
    order[17] = 500
    st.sweep_sequential(view, zt, 1, 0, order=order)
    with pytest.raises(common_amd.MicroscopesHipError) as e:
        gpu_ctx.synchronize()
    assert e.value.code == -6 and "msc_sweep_sequential" in str(e.value)
    st.accumulate(view, zt, reset=True)
    st.sweep_sequential(view, zt, 1, 2)
    gpu_ctx.synchronize()


def test_leave_from_an_empty_group_is_reported_and_the_row_joins(gpu_ctx):
    """z says row 0 is in a group the tables hold empty: the visit reports it (MSC_EDEVICE at the next synchronising
    call) and only seats the row; nothing is taken out of any group"""
    import common_amd
    dev = gpu_ctx.torch_device
    K = 12
    s = _setup(gpu_ctx, C3_SMALL, 300, K, seed=93, empty=3)     # groups 9..11 empty
    st, view = s["st"], s["view"]
    z = s["z"].copy()
    z[0] = K - 1
    zt = torch.from_numpy(z).to(dev)
    st.sweep_sequential(view, zt, 4, 0, nrows=1)
    with pytest.raises(common_amd.MicroscopesHipError) as e:
        gpu_ctx.synchronize()
    assert e.value.code == -6 and "msc_sweep_sequential" in str(e.value)
    cnt = st.get_group_counts().astype(np.int64)
    want = np.bincount(s["z"], minlength=K)          # (the tables still hold row 0 in the group it really is in)
    g = int(zt[0].item())
    assert 0 <= g < K
    want[g] += 1
    assert np.array_equal(cnt, want)
