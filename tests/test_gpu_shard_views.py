"""GPU: shards through views of their own draw what the whole draws.

A multi-GPU run gives every rank a view of its own row shard (common_amd.dist.ShardedSweep).  A sweep's kernels are
chosen by what the bound view holds -- its rows, and its columns' maxima: a count feature's exact tables cover 0 .. the
column's maximum, and the maxima size the tables, pack features into groups, decide sentinel columns, the lookup or
generic kind, the tile / role-split / nich-pack / narrow / lane <-> row kernels and (a count >= 1024) the generic sweep.
Those kernels add a row's scores in different orders, so a shard planned from its own maxima may draw other bits than
the whole.  Here R ranks are emulated in one process, each with a view and a state of its own told the rows of the whole
(set_sweep_rows) and the MAX of every shard's column bounds (set_col_bounds, as ShardedSweep installs them), on data
whose shards' maxima differ on purpose.  Every case checks (a) the draws, bit for bit against the whole view and against
the oracle's double sweep; (b) plain, leave-one-out and leave-one-out + prior scores, against the double twin and bit
for bit against the whole; (c) three full steps with the tables summed across the ranks; (d) the kernels every rank and
the whole took."""
import re

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests.gpu_helpers import TOL, audit, crp_prior_matrix, make_feature, recarray_of
from tests.test_gpu_score import _gate_on_sum
from tests.test_gpu_sweep import _check_agreement

pytestmark = pytest.mark.gpu


def _tables(feats, masks, K, z):
    """state_from_assignment with masked (row, feature) pairs left out of their group's tables"""
    out = []
    for i, f in enumerate(feats):
        F = orc.Family(f["family"], f["hp"], f["dim"], "f64")
        init = None
        if f["family"] == orc.BBNC:
            init = np.zeros(K, dtype=orc.ss_dtype(orc.BBNC, 0, "f64"))
            init["p"] = np.random.default_rng(K).uniform(0.05, 0.95, K).astype(np.float32)
        zz = z if i not in masks else np.where(masks[i], -1, z).astype(np.int32)
        ss32 = orc.narrow_ss(f["family"], F.accumulate(K, f["values"], zz, ss_init=init), f["dim"])
        out.append((F, orc.widen_ss(f["family"], ss32, f["dim"]), ss32))
    return out


def _records(feats, masks):
    arr = recarray_of(feats)
    if not masks:
        return arr
    mask = np.zeros(len(arr), dtype=[("f%d" % i, np.bool_, np.dtype(f["np_dtype"]).shape) for i, f in enumerate(feats)])
    for i, m in masks.items():
        mask["f%d" % i] = m
    return np.ma.masked_array(arr, mask=mask)


def _load(st, fs, counts, alpha):
    import common_amd
    for i, (F, _, ss32) in enumerate(fs):
        st.set_hp(i, F.hp)
        rec = np.zeros(ss32.shape[0], dtype=common_amd.ss_dtype(F.family, F.dim))
        for name in rec.dtype.names:
            rec[name] = ss32[name]
        st.set_ss(i, rec)
    st.set_group_counts(counts)
    st.set_alpha(alpha)


def _oracle_sweep(feats, masks, fs, K, alpha, z, seed, sweep):
    """the oracle's synchronous double sweep; with masked entries (which its C loop does not know) the same sweep from the
    twin's leave-one-out scores: a masked (row, feature) adds nothing, the draw is orc_sample_discrete's"""
    if not masks:
        return orc.sweep([(F, ss64, f["values"]) for f, (F, ss64, _) in zip(feats, fs)], K, alpha, z, seed, sweep, "f64",
                         want_scores=True)
    scores = crp_prior_matrix(np.bincount(z, minlength=K), alpha, z)
    for i, (f, (F, ss64, _)) in enumerate(zip(feats, fs)):
        m = masks.get(i)
        t = F.score_matrix(ss64, f["values"], z if m is None else np.where(m, -1, z).astype(np.int32))
        if m is not None:
            t[m] = 0.0
        scores = scores + t
    want = np.array([orc.sample_discrete(orc.scores_to_probs(scores[n]).astype(np.float32), orc.uniform01(seed, sweep, n))
                     for n in range(len(z))], dtype=np.int32)
    return want, scores


def _kernels(ctx):
    """(score, sweep) kernel names of the last call: the sweep slot names the fused kernel, a sweep through the generic
    path names its score kernel in the other.  The rows-per-wave argument of k_score_tile / k_sweep_tile<2 | 4 | 8, 16, ..>
    follows the CALL's rows (a launch shape: row ranges of one view take any of them with the same bits), so it is left
    out; everything else -- kernel, phases, SPLIT, PAIR, tail and dm arguments -- must match."""
    return tuple(re.sub(r"k_(score|sweep)_tile<[248], 16,", r"k_\1_tile<G, 16,", ctx.last_kernel(w)) for w in ("score", "sweep"))


def _install_whole_bounds(whole_state, whole_view, states, views, N):
    """what ShardedSweep does across ranks: rows of the whole, the elementwise MAX of the shards' column bounds"""
    own = [st.col_bounds(v) for st, v in zip(states, views)]
    bounds = np.max(np.stack(own), axis=0).astype(np.uint32)
    assert np.array_equal(bounds, whole_state.col_bounds(whole_view))       # (the MAX over shards is the whole's)
    for st in states:
        st.set_sweep_rows(N)
        st.set_col_bounds(bounds)
    return own


def _shard_case(gpu_ctx, feats, K, R, seed, masks=None, hot=(), alpha=1.1, empty=2, min_agree=0.995):
    """R emulated ranks against the whole, (a) - (d) of the module's docstring.  hot: global rows the gates must see."""
    import common_amd
    masks = masks or {}
    N = len(feats[0]["values"])
    dev = gpu_ctx.torch_device
    rng = np.random.default_rng(seed)
    z = rng.integers(0, max(1, K - empty), N).astype(np.int32)
    fs = _tables(feats, masks, K, z)
    counts = np.bincount(z, minlength=K).astype(np.uint32)
    arr = _records(feats, masks)
    specs = [(f["family"], f["dim"]) for f in feats]
    parts = [common_amd.dist.shard_rows(N, R, r) for r in range(R)]
    whole = common_amd.DataView.from_recarray(gpu_ctx, arr)
    views = [common_amd.DataView.from_recarray(gpu_ctx, arr[lo:lo + n]) for lo, n in parts]
    sw = common_amd.State(gpu_ctx, specs, K)
    sts = [common_amd.State(gpu_ctx, specs, K) for _ in parts]
    try:
        own = _install_whole_bounds(sw, whole, sts, views, N)
        for st in [sw] + sts:
            _load(st, fs, counts, alpha)

        # (a) draws: every shard with row_id0 = its first global row, against the whole, against the oracle
        zw = torch.from_numpy(z).to(dev)
        sw.sweep_assign(whole, zw, seed=seed, sweep=1)
        names = {"whole": _kernels(gpu_ctx)}
        zr = []
        for r, ((lo, n), st, v) in enumerate(zip(parts, sts, views)):
            t = torch.from_numpy(z[lo:lo + n].copy()).to(dev)
            st.sweep_assign(v, t, seed=seed, sweep=1, row_id0=lo)
            names[r] = _kernels(gpu_ctx)
            zr.append(t.cpu().numpy())
        got, cat = zw.cpu().numpy(), np.concatenate(zr)
        why = dict(kernels=names, own_bounds=[b.tolist() for b in own])
        assert np.array_equal(cat, got), (int((cat != got).sum()), why)
        want, scores = _oracle_sweep(feats, masks, fs, K, alpha, z, seed, 1)
        _check_agreement(got, want, scores, seed, 1, min_agree)

        # (b) scores: plain, leave-one-out, leave-one-out + prior; twin gates on a sample of every shard, the whole's bits
        zt = torch.from_numpy(z).to(dev)
        plain_w = sw.score_value(whole)
        loo_w = sw.score_value(whole, z=zt)
        prior_w = sw.score_value(whole, z=zt, crp_prior=True)
        for r, ((lo, n), st, v) in enumerate(zip(parts, sts, views)):
            t = zt[lo:lo + n].contiguous()
            plain, loo, prior = st.score_value(v), st.score_value(v, z=t), st.score_value(v, z=t, crp_prior=True)
            assert torch.equal(plain, plain_w[lo:lo + n]), (r, why)
            assert torch.equal(loo, loo_w[lo:lo + n]), (r, why)
            assert torch.equal(prior, prior_w[lo:lo + n]), (r, why)
            pick = rng.choice(n, min(n, 300), replace=False)
            local = np.unique(np.concatenate([pick, [0, n - 1], [h - lo for h in hot if lo <= h < lo + n]]).astype(np.int64))
            rows = local + lo
            lt = torch.from_numpy(local).to(dev)
            audit("shard_views.plain", _gate_on_sum(plain[lt].cpu().numpy(), feats, fs, rows, masks=masks), TOL)
            audit("shard_views.loo", _gate_on_sum(loo[lt].cpu().numpy(), feats, fs, rows, z=z, masks=masks), TOL)
            audit("shard_views.loo_prior", _gate_on_sum(prior[lt].cpu().numpy(), feats, fs, rows, z=z, masks=masks,
                                                        prior=crp_prior_matrix(counts, alpha, z[rows])), TOL)
        del plain_w, loo_w, prior_w

        # (c) three full steps: shards begin, their packed tables are summed in rank order, unpacked and committed
        for st in [sw] + sts:
            _load(st, fs, counts, alpha)
        zw = torch.from_numpy(z).to(dev)
        zr = [torch.from_numpy(z[lo:lo + n].copy()).to(dev) for lo, n in parts]
        same = []
        for s in range(3):
            sw.sweep_step(whole, zw, seed=seed + 1, sweep=s)
            for (lo, n), st, v, t in zip(parts, sts, views, zr):
                st.sweep_step_begin(v, t, seed=seed + 1, sweep=s, row_id0=lo)
            packs = [st.reduce_pack() for st in sts]
            gpu_ctx.synchronize()
            total = packs[0].clone()
            for p in packs[1:]:
                total += p
            for p in packs:
                p.copy_(total)
            torch.cuda.synchronize()
            for st in sts:
                st.reduce_unpack()
                st.commit_reduce()
            same.append(float((torch.cat(zr).cpu().numpy() == zw.cpu().numpy()).mean()))
        gpu_ctx.synchronize()
        zf = torch.cat(zr).cpu().numpy()
        assert same[0] == 1.0, (same, why)
        assert min(same) >= 0.9999, (same, why)
        c0 = sts[0].get_group_counts()
        assert np.array_equal(c0, np.bincount(zf, minlength=K))
        for st in sts[1:]:                              # every rank holds the same tables
            assert np.array_equal(st.get_group_counts(), c0)
            for f in range(len(feats)):
                a, b = st.get_ss(f), sts[0].get_ss(f)
                for name in a.dtype.names:
                    assert np.array_equal(a[name], b[name]), (f, name)
        if min(same) == 1.0:                            # same partition => same tables: integers bit for bit
            assert np.array_equal(c0, sw.get_group_counts())
            for f in range(len(feats)):
                a, b = sts[0].get_ss(f), sw.get_ss(f)
                for name in a.dtype.names:
                    x, y = a[name].astype(np.float64), b[name].astype(np.float64)
                    if np.issubdtype(a.dtype[name].base, np.integer):
                        assert np.array_equal(x, y), (f, name)
                    elif name != "p":                   # (bbnc's group parameter is the state's own, not a sum over rows)
                        assert (np.abs(x - y) / np.maximum(1.0, np.abs(y))).max() <= 1e-6, (f, name)

        # (d) the kernels: every rank took the whole's (checked last, so that a case whose bits agree on kernels that
        # parted ways still says what it found above; every assertion above names them too)
        assert all(names[r] == names["whole"] for r in range(R)), why
        return names
    finally:
        for st in [sw] + sts:
            st.close()
        for v in [whole] + views:
            v.close()


def _clip(feats, i, hi):
    feats[i] = dict(feats[i], values=np.minimum(feats[i]["values"], hi).astype(feats[i]["values"].dtype))


def _last_shard(N, R):
    import common_amd
    return common_amd.dist.shard_rows(N, R, R - 1)


@pytest.mark.parametrize("R", [2, 3])
@pytest.mark.parametrize("K", [100, 200])
def test_gp_lds_one_shard_with_a_sentinel_column(gpu_ctx, R, K):
    """gp maxima <= 60 on every shard but the last, whose rows reach 100..127: the first shards alone would fold the mask
    of the masked gp column in as a sentinel (vcap + 1 <= 64) and pack their groups otherwise"""
    rng = np.random.default_rng(10 * K + R)
    N = 8000
    specs = [(orc.BB, 0), (orc.GP, 0), (orc.NICH, 0), (orc.GP, 0), (orc.DD, 5)]
    feats = [make_feature(f, N, K, rng, d) for f, d in specs]
    _clip(feats, 1, 60)
    _clip(feats, 3, 60)
    lo, n = _last_shard(N, R)
    hot = [lo + 7, lo + n // 2, lo + n - 3]
    for h, v in zip(hot, (100, 127, 113)):
        feats[1]["values"][h] = v
        feats[3]["values"][h] = v - 20
    m = rng.random(N) < 0.1
    m[hot] = False
    m[[0, lo + 1]] = True                               # (masked rows on every shard)
    _shard_case(gpu_ctx, feats, K, R, seed=50 + K + R, masks={1: m}, hot=hot)


@pytest.mark.parametrize("R", [2, 3])
def test_gp_generic_kind_on_one_shard_in_pair_mode(gpu_ctx, R):
    """40k rows, K = 100 (PAIR mode, nothing forced), bb + three nich + a gp column whose maximum is <= 100 on every
    shard but the last (200..1000 there): LOOKUP_U32 against GENERIC in the first phase, the role-split or nich-pack
    kernels against the plain tile kernel"""
    rng = np.random.default_rng(300 + R)
    N, K = 40_000, 100
    specs = [(orc.BB, 0), (orc.BB, 0), (orc.GP, 0), (orc.NICH, 0), (orc.NICH, 0), (orc.NICH, 0), (orc.BB, 0)]
    feats = [make_feature(f, N, K, rng, d) for f, d in specs]
    _clip(feats, 2, 100)
    lo, n = _last_shard(N, R)
    hot = [lo + 11, lo + n // 3, lo + n - 1]
    for h, v in zip(hot, (200, 640, 1000)):
        feats[2]["values"][h] = v
    _shard_case(gpu_ctx, feats, K, R, seed=77 + R, hot=hot)


@pytest.mark.parametrize("family", [orc.GP, orc.BNB])
@pytest.mark.parametrize("R", [2, 3])
def test_count_beyond_the_table_on_one_shard(gpu_ctx, family, R):
    """a single count >= 1024 on the last shard: the whole (and that shard) sweep through the generic score-then-sample
    path with k_gp_large_fix, every other shard alone would take the fused kernel"""
    rng = np.random.default_rng(400 + R + family)
    N, K = 12_000, 100
    specs = [(orc.BB, 0), (family, 0), (orc.NICH, 0), (orc.DD, 5)]
    feats = [make_feature(f, N, K, rng, d) for f, d in specs]
    _clip(feats, 1, 200)
    lo, n = _last_shard(N, R)
    hot = [lo + n // 2]
    feats[1]["values"][hot[0]] = 1500
    _shard_case(gpu_ctx, feats, K, R, seed=90 + R + family, hot=hot)


def _small_dm_feats(rng, N, K, R):
    specs = [(orc.BB, 0), (orc.DM, 4), (orc.NICH, 0), (orc.GP, 0)]
    feats = [make_feature(f, N, K, rng, d) for f, d in specs]
    feats[1] = dict(feats[1], values=(feats[1]["values"] // 5).astype(np.int32))     # row totals of at most ~10
    lo, n = _last_shard(N, R)
    hot = [lo + n // 2]
    feats[1]["values"][hot[0]] = [60, 50, 50, 50]       # one row totalling 210
    return feats, hot


@pytest.mark.parametrize("K", [5, 50, 64, 100])
def test_dm_staged_on_one_shard_forced_lane_row(gpu_ctx, K, monkeypatch):
    """a dm feature's counts all small but for one row on the last shard -- the first shard alone
    would stage its dm tables (tail_dm: k_score_tail_rows<.., DMF>), the whole takes the tile kernel.  The lane <-> row
    kernels allowed at any size (MSC_TAIL_MIN_ROWS=1)"""
    monkeypatch.setenv("MSC_TAIL_MIN_ROWS", "1")
    rng = np.random.default_rng(500 + K)
    N, R = 6000, 2
    feats, hot = _small_dm_feats(rng, N, K, R)
    _shard_case(gpu_ctx, feats, K, R, seed=120 + K, hot=hot, empty=1 if K < 10 else 2)


@pytest.mark.parametrize("R", [2, 3])
def test_dm_staged_on_one_shard_unforced(gpu_ctx, R):
    rng = np.random.default_rng(600 + R)
    N, K = 40_000, 100
    feats, hot = _small_dm_feats(rng, N, K, R)
    _shard_case(gpu_ctx, feats, K, R, seed=140 + R, hot=hot)


@pytest.mark.parametrize("K", [32, 64])
def test_narrow_tiling_on_one_shard_only(gpu_ctx, K):
    """K <= 64 and fewer than 65 536 rows: the narrow tiling stages every table in 64 KiB of LDS.  A gp maximum of 600 on
    the last shard makes the tables too large for it; the first shard's alone fit"""
    rng = np.random.default_rng(700 + K)
    N, R = 20_000, 2
    specs = [(orc.BB, 0), (orc.GP, 0), (orc.NICH, 0), (orc.DD, 6)]
    feats = [make_feature(f, N, K, rng, d) for f, d in specs]
    _clip(feats, 1, 40)
    lo, n = _last_shard(N, R)
    hot = [lo + 3, lo + n - 2]
    feats[1]["values"][hot[0]] = 600
    feats[1]["values"][hot[1]] = 350
    _shard_case(gpu_ctx, feats, K, R, seed=160 + K, hot=hot)


@pytest.mark.parametrize("R", [2, 3])
def test_single_nich_sweep_kernel_follows_the_whole(gpu_ctx, R):
    """one nich feature, K = 256, 24 000 rows: the whole takes the transposed single-nich sweep (k_sweep_nich1_t, from 64
    rows a CU on); its shards of 12 000 or 8 000 rows alone would take the row-at-a-time kernel, which draws other bits"""
    rng = np.random.default_rng(800 + R)
    N, K = 24_000, 256
    feats = [make_feature(orc.NICH, N, K, rng)]
    names = _shard_case(gpu_ctx, feats, K, R, seed=180 + R)
    assert names["whole"][1].startswith("k_sweep_nich1_t<"), names


@pytest.mark.parametrize("R", [2, 3])
@pytest.mark.parametrize("plan", ["roles", "lookups"])
def test_small_shards_of_a_large_whole_keep_the_plans_sweep_kernel(gpu_ctx, plan, R):
    """K = 200 (no PAIR mode), 24 000 rows: the whole sweeps on its plan's own kernel (role-split or lookups-only); its
    shards of 12 000 or 8 000 rows alone would be few enough rows for k_sweep_tile<2 | 4, 16>"""
    rng = np.random.default_rng(850 + R + (10 if plan == "roles" else 0))
    N, K = 24_000, 200
    specs = {"roles": [(orc.BB, 0), (orc.BB, 0), (orc.DD, 5), (orc.NICH, 0), (orc.NICH, 0)],
             "lookups": [(orc.BB, 0), (orc.BB, 0), (orc.DD, 5), (orc.DD, 3)]}[plan]
    feats = [make_feature(f, N, K, rng, d) for f, d in specs]
    names = _shard_case(gpu_ctx, feats, K, R, seed=190 + R)
    assert not names["whole"][1].startswith("k_sweep_tile<"), names


FUZZ_FAMILIES = [orc.BB, orc.BBNC, orc.GP, orc.BNB, orc.DD, orc.DM, orc.NICH]


@pytest.mark.parametrize("seed", range(24))
def test_fuzz_shards_with_independently_scaled_maxima(gpu_ctx, seed):
    """a seeded random mix of families (masked or not), K from a list across the kernels' borders, 2 or 3 shards whose
    count columns are scaled shard by shard: whatever route each lands on, the shards draw what the whole draws"""
    import common_amd
    rng = np.random.default_rng(9000 + seed)
    K = int(rng.choice([5, 33, 64, 100, 128, 200, 300]))
    R = int(rng.integers(2, 4))
    N = int(rng.integers(3000, 9000))
    nf = int(rng.integers(2, 7))
    specs = []
    for _ in range(nf):
        fam = int(rng.choice(FUZZ_FAMILIES))
        specs.append((fam, int(rng.integers(2, 12)) if fam == orc.DD else 3 if fam == orc.DM else 0))
    feats = [make_feature(f, N, K, rng, d) for f, d in specs]
    hot = []
    for r in range(R):
        lo, n = common_amd.dist.shard_rows(N, R, r)
        for i, (fam, _) in enumerate(specs):
            v = feats[i]["values"]
            if fam in (orc.GP, orc.BNB):
                scale = float(rng.choice([0.25, 1.0, 4.0, 20.0, 60.0]))
                v[lo:lo + n] = np.minimum(np.floor(v[lo:lo + n] * scale), 1400).astype(v.dtype)
                hot.append(lo + int(np.argmax(v[lo:lo + n])))
            elif fam == orc.DM:
                div = int(rng.choice([1, 5, 40]))
                v[lo:lo + n] = v[lo:lo + n] // div
                hot.append(lo + int(np.argmax(v[lo:lo + n].sum(1))))
    masks = {}
    for i, (fam, _) in enumerate(specs):
        if fam != orc.DM and rng.random() < 0.3:
            m = rng.random(N) < 0.15
            m[hot] = False
            masks[i] = m
    _shard_case(gpu_ctx, feats, K, R, seed=200 + seed, masks=masks, hot=hot, empty=min(3, K - 1),
                min_agree=0.99 if K >= 200 else 0.995)


# ---- the state-level contract of the bounds ---------------------------------------------------------------------------

def _small_state(gpu_ctx, N=6000, K=40, seed=3):
    import common_amd
    rng = np.random.default_rng(seed)
    specs = [(orc.BB, 0), (orc.GP, 0), (orc.DM, 3), (orc.NICH, 0), (orc.BNB, 0)]
    feats = [make_feature(f, N, K, rng, d) for f, d in specs]
    z = rng.integers(0, K - 2, N).astype(np.int32)
    fs = _tables(feats, {}, K, z)
    counts = np.bincount(z, minlength=K).astype(np.uint32)
    view = common_amd.DataView.from_recarray(gpu_ctx, recarray_of(feats))
    return feats, specs, fs, z, counts, view


def test_col_bounds_layout_and_a_wrong_size_is_refused(gpu_ctx):
    import common_amd
    feats, specs, fs, z, counts, view = _small_state(gpu_ctx)
    st = common_amd.State(gpu_ctx, specs, 40)
    try:
        assert st.col_bound_count() == 1 + 4 + 1
        b = st.col_bounds(view)
        v = [f["values"] for f in feats]
        want = [v[1].max()] + list(v[2].max(0)) + [v[2].sum(1).max()] + [v[4].max()]
        assert b.dtype == np.uint32 and b.tolist() == [int(x) for x in want]
        lib = gpu_ctx.lib
        for n in (5, 7):
            with pytest.raises(common_amd.MicroscopesHipError) as e:
                st.set_col_bounds(np.zeros(n, np.uint32))
            assert e.value.code == -1 and "6" in str(e.value)
            out = np.zeros(n, np.uint32)
            rc = lib.msc_state_col_bounds(st._h, view._h, None, out.ctypes.data_as(common_amd._lib.C.c_void_p), n)
            assert rc == -1 and b"6" in lib.msc_last_error()
        st.set_col_bounds(None)                         # (the default back; no bounds is not an error)
    finally:
        st.close()
        view.close()


def test_bounds_below_the_views_own_change_nothing(gpu_ctx):
    import common_amd
    feats, specs, fs, z, counts, view = _small_state(gpu_ctx)
    a, b = common_amd.State(gpu_ctx, specs, 40), common_amd.State(gpu_ctx, specs, 40)
    try:
        for st in (a, b):
            _load(st, fs, counts, 1.2)
        zt = torch.from_numpy(z).to(gpu_ctx.torch_device)
        want = [a.score_value(view), a.score_value(view, z=zt, crp_prior=True)]
        b.set_col_bounds(np.zeros(b.col_bound_count(), np.uint32))
        assert torch.equal(b.score_value(view), want[0])
        b.set_col_bounds(b.col_bounds(view) // 2)
        assert torch.equal(b.score_value(view, z=zt, crp_prior=True), want[1])
    finally:
        a.close()
        b.close()
        view.close()


def test_a_captured_step_replays_nothing_stale_after_new_bounds(gpu_ctx, monkeypatch):
    """three steps capture the step graph; bounds that change the plan (a gp maximum past the narrow tiling's LDS, a dm
    total past the staged tables) must drop it: the next step equals an eager state's given the same bounds"""
    import common_amd
    monkeypatch.setenv("MSC_SWEEP_GRAPH", "1")
    feats, specs, fs, z, counts, view = _small_state(gpu_ctx, K=40)
    g, e = common_amd.State(gpu_ctx, specs, 40), common_amd.State(gpu_ctx, specs, 40)
    try:
        dev = gpu_ctx.torch_device
        zg = torch.from_numpy(z).to(dev)
        for st in (g, e):
            _load(st, fs, counts, 1.2)
        for s in range(4):
            g.sweep_step(view, zg, seed=6, sweep=s)
        assert g.sweep_step_stats()[1] >= 1            # (captured and replayed)
        bounds = g.col_bounds(view)
        bounds[0] = 900                                 # gp
        bounds[4] = 400                                 # dm row total
        g.set_col_bounds(bounds)
        g.sweep_step(view, zg, seed=6, sweep=4)
        # the eager twin: the same four steps without a graph, then the step under the new bounds
        monkeypatch.setenv("MSC_SWEEP_GRAPH", "0")
        ze = torch.from_numpy(z).to(dev)
        for s in range(4):
            e.sweep_step(view, ze, seed=6, sweep=s)
        e.set_col_bounds(bounds)
        e.sweep_step(view, ze, seed=6, sweep=4)
        assert e.sweep_step_stats()[1] == 0
        assert torch.equal(zg, ze)
        assert np.array_equal(g.get_group_counts(), e.get_group_counts())
        for f in range(len(specs)):
            a, b = g.get_ss(f), e.get_ss(f)
            for name in a.dtype.names:
                assert np.array_equal(a[name], b[name]), (f, name)
        # and the scores that follow are the eager state's too
        assert torch.equal(g.score_value(view, z=zg, crp_prior=True), e.score_value(view, z=ze, crp_prior=True))
    finally:
        g.close()
        e.close()
        view.close()
