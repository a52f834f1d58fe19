"""The tempered ensemble's steps between sweeps, without a GPU: the ABI declares and exports msc_chains_exchange and
msc_chains_anneal_weights and the binding carries their argument types; common_amd/csrc/temper_math.hpp built with the
host compiler into tests/cxx/temper_math_host.cpp -- a program of its own -- and run, plain and under the address and
undefined-behaviour sanitizers; the ladders of common_amd.tempering; the numpy restatement the GPU test compares the
exchange against, held to the rule's invariants; and, on the enumerated partitions of six rows, a replica-exchange sampler
and an annealed importance sampler that decide through that restatement, against every rung's exact tempered posterior
and the exact evidence."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from tests import seq_helpers as sh
from tests import smc_helpers as H
from tests import temper_helpers as TH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "common_amd", "csrc")
SIGS = {
    "msc_chains_exchange": "int msc_chains_exchange(msc_chains *ch, const double *joint_dev, uint64_t ld_joint, uint32_t nrungs, "
                           "float *beta_dev, int32_t *rung_dev, uint64_t parity, uint64_t seed, uint64_t sweep, "
                           "uint32_t *proposed_dev, uint32_t *accepted_dev);",
    "msc_chains_anneal_weights": "int msc_chains_anneal_weights(msc_chains *ch, const double *joint_dev, uint64_t ld_joint, "
                                 "const float *beta_from_dev, const float *beta_to_dev, double *logw_dev);",
}


@pytest.mark.parametrize("name", sorted(SIGS))
def test_header_declares_library_exports_and_binding_types(name):
    import common_amd
    from common_amd import _lib as L
    flat = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "microscopes_hip.h")).read())
    assert SIGS[name] in flat
    assert hasattr(C.CDLL(common_amd.LIB_PATH), name)
    assert name in common_amd.EXPORTS
    lib = L.load()          # dlopen only; no device call
    res, args = L._SIGS[name]
    params = re.search(name + r"\((.*?)\);", SIGS[name]).group(1).split(", ")
    assert res is C.c_int and len(args) == len(params)
    for p, a in zip(params, args):
        if "*" in p:
            assert a is C.c_void_p, p
        elif p.startswith("uint64_t"):
            assert a is C.c_uint64, p
        else:
            assert p.startswith("uint32_t") and a is C.c_uint32, p
    assert getattr(lib, name).argtypes == args


@pytest.mark.parametrize("extra", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "sanitized"])
def test_temper_math_host(tmp_path, extra):
    exe = str(tmp_path / "temper_math_host")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC] + extra +
                          [os.path.join(ROOT, "tests", "cxx", "temper_math_host.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert out.returncode == 0, out.stdout
    assert "temper math ok" in out.stdout


def test_temper_math_is_host_only_and_the_kernels_call_it():
    src = open(os.path.join(CSRC, "temper_math.hpp")).read()
    code = "\n".join(ln.split("//")[0] for ln in src.splitlines())
    for word in ("msc_state", "msc_context", "hip/", "msc_internal"):
        assert word not in code, word
    kern = open(os.path.join(CSRC, "kernels_temper.hip")).read()
    assert "temper::exchange_ladder(" in kern and "temper::anneal_step(" in kern and "temper::chain_loglik(" in kern
    # no sum is atomic (the one atomic is the error word's report, the protocol of device_error.hpp)
    assert "atomicAdd" not in kern and kern.count("__hip_atomic_") == 2 and "err_word" in kern
    host = open(os.path.join(CSRC, "chains.cpp")).read()
    assert "temper::check_exchange(" in host and "temper::check_anneal_weights(" in host


def test_python_surface():
    import common_amd
    from common_amd import tempering
    assert common_amd.tempering is tempering
    E = common_amd.ChainEnsemble
    assert list(inspect.signature(E.exchange).parameters) == ["self", "joint", "beta", "rung", "nrungs", "parity", "seed",
                                                               "sweep", "counters"]
    assert list(inspect.signature(E.anneal_weights).parameters) == ["self", "joint", "beta_from", "beta_to", "logw"]


def test_ladders():
    from common_amd import tempering as T
    for kind in ("geometric", "linear"):
        for R in (1, 2, 3, 5, 8):
            for bmin in (0.0, 0.1):
                b = T.ladder(R, kind, bmin)
                assert b.dtype == np.float32 and b.shape == (R,) and b[0] == 1.0
                assert np.all(np.diff(b) < 0) and (R == 1 or b[-1] == np.float32(bmin)), (kind, R, bmin, b)
    assert np.array_equal(T.ladder(4, "linear"), np.array([1, 2 / 3, 1 / 3, 0], dtype=np.float32))
    assert np.array_equal(T.ladder(4), np.array([1, 0.5, 0.25, 0], dtype=np.float32))
    assert np.allclose(T.ladder(3, "geometric", 0.25), [1, 0.5, 0.25])
    for bad in (dict(nrungs=0), dict(nrungs=3, kind="harmonic"), dict(nrungs=3, beta_min=1.0), dict(nrungs=3, beta_min=-0.1)):
        with pytest.raises(ValueError):
            T.ladder(**bad)


def test_restated_exchange_keeps_the_invariants():
    """the numpy restatement the GPU test compares against: rungs stay permutations, beta follows the rung, a NaN chain
    stays put, a broken ladder is left alone"""
    rng = np.random.default_rng(3)
    for R in (4, 5):
        betas = np.linspace(1.0, 0.0, R).astype(np.float32)
        nl, F = 3, 2
        joint = rng.normal(-20, 5, (nl * R, F + 3))
        joint[1, 2] = np.nan
        joint[R + 2, 3] = -np.inf
        rung = np.concatenate([rng.permutation(R) for _ in range(nl)]).astype(np.int32)
        beta = betas[rung]
        prop = acc = np.zeros((nl, R - 1), dtype=np.uint32)
        for parity in (0, 1, 2, 3):
            was = rung.copy()
            beta, rung, prop, acc, bad = TH.exchange_np(joint, F, R, beta, rung, parity, 5, parity, prop, acc)
            assert not bad and rung[1] == was[1]
            for l in range(nl):
                assert sorted(rung[l * R:(l + 1) * R]) == list(range(R))
            assert np.array_equal(beta, betas[rung])
        assert prop.sum() == 2 * nl * (R - 1) and 0 < acc.sum() < prop.sum()
        rung[0] = rung[1]
        b2, r2, p2, a2, bad = TH.exchange_np(joint, F, R, beta, rung, 0, 5, 9, prop, acc)
        assert bad == [0] and np.array_equal(r2[:R], rung[:R]) and np.array_equal(p2[0], prop[0])


@pytest.mark.parametrize("R", [1, 2, 4, 5, 9])
def test_the_walk_the_kernel_makes_is_the_restatement(tmp_path, R):
    """tests/cxx/temper_walk_host.cpp calls temper_math.hpp's exchange_ladder and anneal_step -- the functions the kernels
    call -- on arrays from here, with the Philox uniforms the kernel would draw: beta, rung, the counters and the weights
    equal the numpy restatement's bytes, NaN and infinite likelihoods and a broken ladder among them"""
    from oracle import oracle as orc
    exe = str(tmp_path / "temper_walk_host")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC,
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cxx", "temper_walk_host.cpp"), "-o", exe])
    rng = np.random.default_rng(100 + R)
    nl, F, ld = 7, 3, 8
    nc, npairs = nl * R, nl * (R - 1)
    betas = np.linspace(1.0, 0.0, R).astype(np.float32) if R > 1 else np.ones(1, dtype=np.float32)
    joint = rng.normal(-30.0, 6.0, (nc, ld))
    joint[0, 2] = np.nan
    joint[nc - 1, 3] = -np.inf
    joint[nc // 2, 4] = -np.inf
    rung = np.concatenate([rng.permutation(R) for _ in range(nl)]).astype(np.int32)
    if R > 1:
        rung[3 * R] = rung[3 * R + 1]                          # ladder 3 is broken
    beta = betas[rung]
    prop = rng.integers(0, 50, (nl, R - 1)).astype(np.uint32)
    acc = rng.integers(0, 50, (nl, R - 1)).astype(np.uint32)
    beta_to = np.where(rng.random(nc) < 0.3, beta, rng.random(nc)).astype(np.float32)
    logw = rng.normal(0.0, 1.0, nc)
    for parity, sweep in ((0, 4), (1, 4), (6, 1 << 33), (7, 0)):
        u = np.array([orc.uniform01(91, sweep, c) for c in range(nc)], dtype=np.float32)
        blob = b"".join(a.tobytes() for a in (np.array([nl, R, F, ld, parity], dtype=np.uint64), joint, beta, rung, u, prop, acc,
                                              beta_to, logw))
        out = subprocess.run([exe], input=blob, stdout=subprocess.PIPE, check=True).stdout
        want = TH.exchange_np(joint, F, R, beta, rung, parity, 91, sweep, prop, acc)
        want_w = TH.anneal_np(joint, F, beta, beta_to, logw)
        ok = np.ones(nl, dtype=np.uint32)
        ok[want[4]] = 0
        assert want[4] == ([3] if R > 1 else [])
        assert out == b"".join(a.tobytes() for a in (want[0], want[1], want[2], want[3], ok, want_w)), (R, parity)
        assert len(out) == 8 * nc + 8 * npairs + 4 * nl + 8 * nc
        beta, rung, prop, acc = want[:4]


def test_restated_weights():
    joint = np.array([[0, 0, -3.0, -1.0, 0], [0, 0, -np.inf, 2.0, 0], [0, 0, -np.inf, 2.0, 0]])
    got = TH.anneal_np(joint, 2, [0.0, 0.5, 0.25], [0.5, 0.5, 0.5], [1.0, 7.0, 0.0])
    assert got.tolist() == [-1.0, 7.0, -np.inf]


# ---- the rule leaves every pi_beta invariant: the samplers over the exact table --------------------------------------------
ALPHA = 1.0


@pytest.fixture(scope="module")
def tables():
    return {name: TH.PartitionTable(H.replay_features(feats), ALPHA) for name, feats in H.six_row_datasets().items()}


def test_partition_table_is_the_exact_posterior(tables):
    for name, feats in H.six_row_datasets().items():
        parts, p = sh.exact_posterior([(F, v) for F, v, _ in H.replay_features(feats)], ALPHA)
        assert parts == tables[name].parts and np.allclose(tables[name].posterior(1.0), p, rtol=1e-12, atol=0)
        assert abs(np.log(np.exp(tables[name].log_prior).sum())) < 1e-12       # the CRP prior is normalised


@pytest.mark.parametrize("name", sorted(TH.LADDERS))
def test_replica_exchange_reaches_every_rungs_exact_target(tables, name):
    """per-rung TV <= 0.05 and KL <= 0.01 against the exact pi_beta, on ladders whose rungs' targets are >= 0.10 apart (so a
    sampler that ignored beta, or a swap rule with the wrong sign, could not pass: a wrong sign drives the cold rung
    towards the prior).  16 ladders x 4 000 iterations after 200: 6.4e4 samples a rung, whose independent-draw TV over the
    203 partitions is about 0.02."""
    table, betas = tables[name], TH.LADDERS[name]
    sep = TH.rung_separation(table, betas)
    print("%s: rungs %s, smallest exact TV between two rungs %.3f" % (name, betas, sep))
    assert sep >= TH.MIN_RUNG_TV, (name, sep)
    freq, rate, held = TH.replica_exchange_np(table, betas, 16, 200, 4000, np.random.default_rng(7))
    for j, b in enumerate(betas):
        tv, kl = sh.tv_kl(freq[j], table.posterior(np.float32(b)))
        print("   rung %d beta %.3f: TV %.4f KL %.5f" % (j, b, tv, kl))
        assert tv <= TH.GATE_TV and kl <= TH.GATE_KL, (name, j, tv, kl)
    print("   acceptance", rate)
    assert np.all((rate > 0) & (rate < 1)) and held, (rate, held)


@pytest.mark.parametrize("name", sorted(TH.LADDERS))
def test_annealed_importance_sampling_gives_the_exact_evidence(tables, name):
    """1 024 chains, T = 32 linear temperatures: |log_evidence - exact| <= 5 se + 1e-4"""
    from common_amd import smc as S
    exact = H.exact_log_evidence(H.replay_features(H.six_row_datasets()[name]), ALPHA)
    logw = TH.ais_np(tables[name], np.linspace(0.0, 1.0, 33), 1024, np.random.default_rng(11))
    est, se = S.log_mean_exp(logw), H.evidence_se(S.normalised_weights(logw))
    print("%s: AIS %.5f exact %.5f se %.5f" % (name, est, exact, se))
    assert abs(est - exact) <= 5 * se + 1e-4, (name, est, exact, se)


def test_tempered_replay():
    """beta = 1 is the replay; beta = 0 the CRP terms alone; in between the features' sum is scaled"""
    feats = H.six_row_datasets()["nich"] + H.six_row_datasets()["bb"]
    rfeats = H.replay_features(feats)
    z = np.array([0, 0, 1, 2, -1, 2], dtype=np.int32)
    plain = sh.Replay(rfeats, 5, 1.3, z).scores(4)
    crp = TH.TemperedReplay(rfeats, 5, 1.3, z, 0.0).scores(4)
    assert np.allclose(TH.TemperedReplay(rfeats, 5, 1.3, z, 1.0).scores(4), plain, rtol=0, atol=1e-12)
    assert np.allclose(crp[:3], np.log([2.0, 1.0, 2.0])) and np.allclose(crp[3:], np.log(1.3 / 2))
    assert np.allclose(TH.TemperedReplay(rfeats, 5, 1.3, z, 0.25).scores(4), crp + 0.25 * (plain - crp), rtol=0, atol=1e-12)
    a, b = TH.TemperedReplay(rfeats, 5, 1.3, z, 0.0), TH.TemperedReplay(rfeats, 5, 1.3, z, 1.7)
    assert a.visit(4, 0.3)[0] in range(5) and b.visit(4, 0.3)[0] in range(5) and a.cnt.sum() == b.cnt.sum() == 6
