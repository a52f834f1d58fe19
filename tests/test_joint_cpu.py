"""The log joint, without a GPU: the ABI declares and exports msc_score_joint, msc_chains_score_joint and
msc_chains_keep_best and the binding carries their argument types; common_amd/csrc/joint_math.hpp (the total's order,
the keep-best rule, the shape checks) built with the host compiler into tests/cxx/joint_math_host.cpp -- a program of
its own -- and run, plain and under the address and undefined-behaviour sanitizers; and the argument checks of
State.score_joint's priors and of chains.JointTracker that need no device."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "common_amd", "csrc")
SIGS = {
    "msc_score_joint": "int msc_score_joint(msc_state *st, const msc_slice_coord *coords, uint32_t n, "
                       "const uint8_t *slots_dev, double *out_dev);",
    "msc_chains_score_joint": "int msc_chains_score_joint(msc_chains *ch, const msc_slice_coord *coords, uint32_t n, "
                              "const uint8_t *slots_dev, uint64_t ld_slots, double *out_dev, uint64_t ld_out);",
    "msc_chains_keep_best": "int msc_chains_keep_best(msc_chains *ch, const double *joint_dev, uint64_t ld_joint, "
                            "const int32_t *z_dev, uint64_t ld_z, uint64_t nrows, uint64_t iter, double *best_dev, "
                            "int32_t *best_z_dev, uint64_t ld_best, int64_t *best_iter_dev);",
}


@pytest.mark.parametrize("name", sorted(SIGS))
def test_header_declares_library_exports_and_binding_types(name):
    import common_amd
    from common_amd import _lib as L
    flat = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "microscopes_hip.h")).read())
    assert SIGS[name] in flat
    assert "#define MSC_ABI_VERSION 1" in flat and L.ABI_VERSION == 1
    assert hasattr(C.CDLL(common_amd.LIB_PATH), name)
    assert name in common_amd.EXPORTS
    lib = L.load()          # dlopen only; no device call
    res, args = L._SIGS[name]
    params = re.search(name + r"\((.*?)\);", SIGS[name]).group(1).split(", ")
    assert res is C.c_int and len(args) == len(params)
    for p, a in zip(params, args):
        if "*" in p:
            assert a in (C.c_void_p, C.POINTER(L.SliceCoord)), p
        elif p.startswith("uint64_t"):
            assert a is C.c_uint64, p
        else:
            assert p.startswith("uint32_t") and a is C.c_uint32, p
    assert getattr(lib, name).argtypes == args


def test_header_states_what_is_not_supported():
    flat = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "microscopes_hip.h")).read())
    assert "MSC_EUNSUPPORTED for a state with a niw feature" in flat


@pytest.mark.parametrize("extra", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "sanitized"])
def test_joint_math_host(tmp_path, extra):
    exe = str(tmp_path / "joint_math_host")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC] + extra +
                          [os.path.join(ROOT, "tests", "cxx", "joint_math_host.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert out.returncode == 0, out.stdout
    assert "joint math ok" in out.stdout


def test_joint_math_is_host_only():
    src = open(os.path.join(CSRC, "joint_math.hpp")).read()
    code = "\n".join(ln.split("//")[0] for ln in src.splitlines())
    for word in ("msc_state", "msc_context", "hip/", "msc_internal"):
        assert word not in code, word
    kern = open(os.path.join(CSRC, "kernels_joint.hip")).read()
    assert "joint::keep_best_wins(" in kern and "joint::joint_total(" in kern      # the kernels call the same functions
    assert "atomic" not in "\n".join(ln.split("//")[0] for ln in kern.splitlines())


def test_python_surface():
    import common_amd
    from common_amd import chains, diagnostics
    assert callable(common_amd.State.score_joint) and callable(common_amd.ChainEnsemble.score_joint)
    assert common_amd.JointTracker is chains.JointTracker and common_amd.diagnostics is diagnostics
    assert chains.RunResult._fields == ("trace", "values")
    import inspect
    sig = inspect.signature(common_amd.ChainEnsemble.run)
    assert list(sig.parameters)[-1] == "joint" and sig.parameters["joint"].default is None
    assert list(inspect.signature(chains.JointTracker.__init__).parameters) == ["self", "ens", "every", "keep_best", "priors"]


def test_priors_are_checked_without_a_device():
    import common_amd
    from common_amd import _lib as L
    P = common_amd.State._joint_priors
    assert P(None) == (None, 0) and P([]) == (None, 0)
    arr, n = P([{"feature": "alpha", "prior": "exponential", "a": 2.0},
                {"feature": 3, "coord": 1, "prior": "noninf_beta", "partner": 0, "width": 0.5}])
    assert n == 2 and arr[0].feature == L.HP_CLUSTER and arr[0].prior == L.PRIOR_EXPONENTIAL and arr[0].prior_a == 2.0
    assert arr[0].width == 1.0                       # a prior needs no width: the library's check is given 1
    assert (arr[1].feature, arr[1].coord, arr[1].prior, arr[1].partner, arr[1].width) == (3, 1, L.PRIOR_NONINF_BETA, 0, 0.5)

    class Carrier(object):                           # what hypers.FeatureHpSlice / EnsembleHpSlice look like to it
        coords = [{"feature": 0, "coord": 0, "width": 2.0}]
    assert P(Carrier())[1] == 1
    for bad in ([3], ["alpha"], [{"coord": 0}], 5):
        with pytest.raises((ValueError, TypeError)):
            P(bad)


def test_tracker_arguments_are_checked_without_a_device():
    from common_amd import chains
    assert chains.joint_tracker_args(1, True) == (1, True) and chains.joint_tracker_args(7, False) == (7, False)
    for every in (0, -1, 1.5, "2", None, True):
        with pytest.raises(ValueError):
            chains.joint_tracker_args(every, True)
    for keep in (1, None, "yes"):
        with pytest.raises(ValueError):
            chains.joint_tracker_args(1, keep)
    with pytest.raises(ValueError):
        chains.JointTracker(object())                # not an ensemble
    with pytest.raises(ValueError):
        chains.JointTracker(None, every=0)           # (every is checked first)
