"""The sweep at a temperature and its drivers, without a GPU: the ABI declares and exports msc_chains_sweep_tempered and the
binding carries its argument types; the one line of arithmetic in common_amd/csrc/temper_math.hpp (tempered_add, beta_ok)
built with the host compiler into tests/cxx/temper_sweep_host.cpp -- a program of its own -- and run, plain and under the
address and undefined-behaviour sanitizers; the kernel calls those functions and the header stays host-only; the Python
surface: sweep(beta=), run_tempered, ais, the result types, the exchange's key, the cold samples of a trace and the checks
of an annealing schedule."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "common_amd", "csrc")
NAME = "msc_chains_sweep_tempered"
SIG = ("int msc_chains_sweep_tempered(msc_chains *ch, const msc_dataview *view, const uint32_t *cols, uint64_t row0, "
       "uint64_t nrows, uint64_t row_id0, int32_t *z_dev, uint64_t ld_z, const uint32_t *order_dev, uint64_t ld_order, "
       "uint32_t nsweeps, const uint64_t *host_seeds, uint64_t sweep, const float *beta_dev, uint32_t trace_every, "
       "int32_t *trace_dev, uint32_t *occupied_dev);")


def test_header_declares_library_exports_and_binding_types():
    import common_amd
    from common_amd import _lib as L
    flat = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "microscopes_hip.h")).read())
    assert SIG in flat
    assert hasattr(C.CDLL(common_amd.LIB_PATH), NAME)
    assert NAME in common_amd.EXPORTS
    lib = L.load()          # dlopen only; no device call
    res, args = L._SIGS[NAME]
    params = re.search(NAME + r"\((.*?)\);", SIG).group(1).split(", ")
    assert res is C.c_int and len(args) == len(params) == 17
    for p, a in zip(params, args):
        if p == "const uint64_t *host_seeds":
            assert a is C.POINTER(C.c_uint64), p          # (a host array, as msc_chains_sweep's)
        elif "*" in p:
            assert a is C.c_void_p, p
        elif p.startswith("uint64_t"):
            assert a is C.c_uint64, p
        else:
            assert p.startswith("uint32_t") and a is C.c_uint32, p
    assert getattr(lib, NAME).argtypes == args
    # msc_chains_sweep's list with beta_dev put in after the sweep counter
    base = list(L._SIGS["msc_chains_sweep"][1])
    assert args == base[:13] + [C.c_void_p] + base[13:]


@pytest.mark.parametrize("extra", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "sanitized"])
def test_temper_sweep_host(tmp_path, extra):
    exe = str(tmp_path / "temper_sweep_host")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC] + extra +
                          [os.path.join(ROOT, "tests", "cxx", "temper_sweep_host.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert out.returncode == 0, out.stdout
    assert "temper sweep math ok" in out.stdout


def test_the_kernel_calls_the_host_only_header():
    src = open(os.path.join(CSRC, "temper_math.hpp")).read()
    code = "\n".join(ln.split("//")[0] for ln in src.splitlines())
    for word in ("msc_state", "msc_context", "hip/", "msc_internal"):
        assert word not in code, word
    assert "tempered_add(" in code and "beta_ok(" in code
    kern = open(os.path.join(CSRC, "kernels_seq.hip")).read()
    assert "temper::tempered_add(" in kern and "temper::beta_ok(" in kern
    assert "k_sweep_seq_chains_tempered" in kern and "MSC_DEVERR_TEMPER_BETA" in kern
    # the new kernel lives beside the sweep it instantiates, not with the steps between sweeps
    assert "k_sweep_seq" not in open(os.path.join(CSRC, "kernels_temper.hip")).read()
    err = open(os.path.join(CSRC, "device_error.hpp")).read()
    assert re.search(r"MSC_DEVERR_TEMPER_BETA\s*=\s*512u", err)
    abi = open(os.path.join(CSRC, "abi.cpp")).read()
    assert "code & 512u" in abi and "~1023u" in abi and "~511u" not in abi
    assert re.search(r'code & 512u\) add\("msc_chains_sweep_tempered', abi)
    host = open(os.path.join(CSRC, "chains.cpp")).read()
    assert "launch_sweep_seq_chains_tempered(" in host


def test_python_surface():
    import common_amd
    from common_amd import tempering as T
    E = common_amd.ChainEnsemble
    params = inspect.signature(E.sweep).parameters
    assert list(params)[-1] == "beta" and params["beta"].default is None
    assert list(params)[:-1] == ["self", "view", "nsweeps", "seed", "sweep", "order", "trace_every", "zmatrix", "want_occupied",
                                 "row0", "nrows", "row_id0", "cols"]
    sig = inspect.signature(E.run_tempered)
    assert list(sig.parameters) == ["self", "view", "niters", "seed", "betas", "sweep", "order", "trace_every", "zmatrix",
                                    "state"]
    assert [sig.parameters[k].default for k in ("sweep", "order", "trace_every", "zmatrix", "state")] == [0, None, None, None,
                                                                                                          None]
    sig = inspect.signature(E.ais)
    assert list(sig.parameters) == ["self", "view", "betas", "seed", "sweeps_per_temp", "order", "sweep"]
    assert [sig.parameters[k].default for k in ("sweeps_per_temp", "order", "sweep")] == [1, None, 0]
    assert T.TemperedResult._fields == ("trace", "rungs", "beta", "rung", "proposed", "accepted", "joint")
    assert T.AISResult._fields == ("log_evidence", "log_weights", "weights", "ess", "truncated")
    assert common_amd.TemperedResult is T.TemperedResult and common_amd.AISResult is T.AISResult
    assert "TemperedResult" in common_amd.__all__ and "AISResult" in common_amd.__all__
    for doc in (E.run_tempered.__doc__, E.ais.__doc__):
        assert "share hyper-parameters and alpha" in " ".join(doc.split())
    assert "calls nothing" not in T.__doc__ and "run_tempered" in T.__doc__


def test_exchange_key():
    from common_amd import tempering as T
    from common_amd.chains import chain_seeds
    want = 5 ^ 0x9E3779B97F4A7C15
    assert T.exchange_key(5) == want and T.exchange_key([5, 9]) == want and T.exchange_key(np.uint64(5)) == want
    assert T.exchange_key(7) == chain_seeds(7, 3)[0] ^ 0x9E3779B97F4A7C15
    # no chain's own key, whatever its index below 2^32, and not the slice step's key of any chain either
    for seed in (0, 5, (1 << 64) - 1, 0x9E3779B97F4A7C15, (1 << 32) - 1, 0xFFFFFFFF00000000):
        k = T.exchange_key(seed)
        assert 0 <= k < (1 << 64)
        assert (k - seed) % (1 << 64) >= (1 << 32)
        assert ((k ^ 0x2545F4914F6CDD1D) - seed) % (1 << 64) >= (1 << 32)


def test_cold_samples():
    from common_amd import tempering as T
    nchains, ns, n = 4, 3, 5
    trace = torch.arange(nchains * ns * n, dtype=torch.int32).reshape(nchains, ns, n)
    rungs = torch.tensor([[0, 1, 0], [1, 0, 1], [2, 2, 2], [3, 3, 0]], dtype=torch.int32)
    got = T.cold_samples(trace, rungs)
    want = torch.stack([trace[0, 0], trace[0, 2], trace[1, 1], trace[3, 2]])        # chain-major, then sample order
    assert got.dtype == torch.int32 and tuple(got.shape) == (4, n) and torch.equal(got, want)
    assert torch.equal(T.cold_samples(trace, rungs, rung=2), trace[2])
    assert torch.equal(T.cold_samples(trace, rungs, 3), torch.stack([trace[3, 0], trace[3, 1]]))
    assert tuple(T.cold_samples(trace, rungs, 7).shape) == (0, n)
    with pytest.raises(ValueError):
        T.cold_samples(trace, rungs[:, :2])


def test_ais_refuses_a_bad_schedule_before_any_device_work():
    """ChainEnsemble.ais checks the schedule first, through tempering.ais_betas: an object that was never given a device
    (no context, no handle) gets as far as that check and no further"""
    import common_amd
    from common_amd import tempering as T
    good = T.ais_betas(np.linspace(0.0, 1.0, 33))
    assert good.dtype == np.float32 and good.shape == (33,) and good[0] == 0.0 and good[-1] == 1.0
    assert T.ais_betas([0, 0, 0.5, 0.5, 1, 1]).tolist() == [0.0, 0.0, 0.5, 0.5, 1.0, 1.0]
    ens = object.__new__(common_amd.ChainEnsemble)           # no __init__: it has nothing a device call could use
    for bad in ([0.1, 0.5, 1.0], [0.0, 0.5, 0.9], [0.0, 0.6, 0.5, 1.0], [], [0.0, float("nan"), 1.0], [1.0, 0.0]):
        with pytest.raises(ValueError):
            T.ais_betas(bad)
        with pytest.raises(ValueError, match="betas"):
            ens.ais(None, bad, 1)
    with pytest.raises(ValueError, match="closed"):         # a good schedule passes the check and meets the next one
        ens.ais(None, [0.0, 1.0], 1)
