"""The heavy-rung fixture (tests/golden/heavy.json, tests/heavy_cases.py) on the CPU: the generator reproduces the
committed numbers, and the oracle's double twin is measured against them -- held to 1e-7 on every rung whose posterior
parameters stay below 1e6 (where the rest of the suite uses it as the arbiter), reported without a gate beyond (its
differences of lgamma cancel at the size of lgamma's value there: DESIGN.md section 2 carries the table this prints)."""
import importlib.util
import os

import numpy as np
import pytest

from oracle import oracle as orc
from tests import heavy_cases as hc
from tests.gpu_helpers import rel_err

TWIN_GATE = 1e-7
TWIN_LIMIT = 1e6


def test_generator_reproduces_the_committed_fixture():
    pytest.importorskip("mpmath")
    spec = importlib.util.spec_from_file_location(
        "make_heavy_golden", os.path.join(os.path.dirname(hc.FIXTURE), "make_heavy_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    doc = gen.generate()
    fresh, kept = doc["families"], hc.load_fixture()
    assert sorted(fresh) == sorted(kept) == sorted(hc.FAMILIES)
    crp = hc.load_score_assignment()
    assert doc["score_assignment"]["alpha"] == float(hc.ALPHA32) and sorted(crp) == sorted(hc.LAYOUT_KEYS)
    for key in crp:
        assert abs(doc["score_assignment"][key] - crp[key]) <= 1e-15 * abs(crp[key]), key
    for name, d in fresh.items():
        ok = np.array(d["loo_ok"], dtype=bool)
        assert np.array_equal(ok, kept[name]["loo_ok"]), name
        for key in ("score_value", "loo", "score_data"):
            a = np.array([[np.nan if x is None else x for x in row] for row in d[key]] if key != "score_data" else d[key],
                         dtype=np.float64)
            b = kept[name][key]
            assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)), (name, key)
            m = ~np.isnan(a)
            assert np.all(np.abs(a[m] - b[m]) <= 1e-15 * np.abs(b[m])), (name, key)


def test_fixture_covers_every_family_rung_and_value():
    fx = hc.load_fixture()
    for name in hc.FAMILIES:
        R, V = len(hc.rungs(name)), len(hc.values(name))
        assert R == 2 * len(hc.counts_of(name)) and fx[name]["score_value"].shape == (R, V) and fx[name]["score_data"].shape == (R,)
        assert np.all(np.isfinite(fx[name]["score_value"])) and np.all(np.isfinite(fx[name]["score_data"]))
        n = hc.rung_counts(name)
        if name != "dm":                                            # (dm has no count: the zero vector leaves any group)
            assert not fx[name]["loo_ok"][n == 0].any()             # nothing leaves an empty group
        assert fx[name]["loo_ok"][n >= 1000].any(axis=1).all()      # every large rung has rows that can leave it
    assert os.path.getsize(hc.FIXTURE) < 150 * 1024


def _largest_parameter(name, rec):
    """the largest posterior parameter of the rung, up to the hyperparameters' O(1): its largest count or sum (bnb: r count)"""
    big = [float(np.max(rec[f])) for f in rec.dtype.names if np.issubdtype(rec.dtype[f].base, np.integer)]
    if name == "bnb":
        big.append(float(hc.hp_of("bnb")["r"]) * float(rec["count"]))
    return max(big)


def test_double_twin_against_the_fixture(capsys):
    fx = hc.load_fixture()
    lines, bad = [], []
    for name, (fam, dim) in hc.FAMILIES.items():
        F = orc.Family(fam, hc.hp_of(name), dim, "f64")
        ss32 = hc.rungs(name)
        ss64 = orc.widen_ss(fam, ss32, dim)
        vals = hc.values(name)
        R = len(ss32)
        plain = F.score_matrix(ss64, vals).T                         # [R, V]
        loo = np.full_like(plain, np.nan)
        for r in range(R):
            z = np.where(fx[name]["loo_ok"][r], r, -1).astype(np.int32)
            loo[r] = F.score_matrix(ss64, vals, z)[:, r]
        data = F.score_data_all(ss64)
        ok = fx[name]["loo_ok"]
        e = np.maximum(rel_err(plain, fx[name]["score_value"]).max(axis=1),
                       np.where(ok, rel_err(np.where(ok, loo, 0.0), np.where(ok, fx[name]["loo"], 0.0)), 0.0).max(axis=1))
        ed = rel_err(data, fx[name]["score_data"])
        counts = hc.rung_counts(name)
        for n in hc.counts_of(name):
            rows = np.nonzero(counts == n)[0]
            gated = all(_largest_parameter(name, ss32[r]) <= TWIN_LIMIT for r in rows)
            lines.append("%-6s n = %-9d score_value %.1e  score_data %.1e  %s" % (
                name, n, e[rows].max(), ed[rows].max(), "gated" if gated else "beyond 1e6: reported only"))
        for r in range(R):
            if _largest_parameter(name, ss32[r]) <= TWIN_LIMIT and max(e[r], ed[r]) > TWIN_GATE:
                bad.append((name, r, float(e[r]), float(ed[r])))
    with capsys.disabled():
        print("\nworst rel_err of the double twin against the 60-digit fixture, per (family, count):")
        print("\n".join(lines))
    assert not bad, bad
