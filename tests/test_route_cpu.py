"""The kernel routes, host side: common_amd/csrc/route.hpp (with feat_desc.hpp and tile_plan.hpp, which makes the plans
it routes) built with the host compiler into tests/cxx/test_route.cpp -- a program of its own that includes nothing else
of the library -- and run, plain and under the address and undefined-behaviour sanitizers.  No device needed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "common_amd", "csrc")


@pytest.mark.parametrize("extra", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "sanitized"])
def test_route_host(tmp_path, extra):
    exe = str(tmp_path / "test_route")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC] + extra +
                          [os.path.join(ROOT, "tests", "cxx", "test_route.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert out.returncode == 0, out.stdout
    assert "route ok" in out.stdout


def test_routes_read_no_state():
    """the routes are functions of RouteFacts, Switches and the call's rows: route.hpp names neither the state nor the
    context nor the environment, and abi.cpp holds no second copy of a rule"""
    src = open(os.path.join(CSRC, "route.hpp")).read()
    code = "\n".join(ln.split("//")[0] for ln in src.splitlines())
    for word in ("msc_state", "msc_context", "getenv", "hip"):
        assert word not in code, word
    abi = open(os.path.join(CSRC, "abi.cpp")).read()
    for rule in ("narrow_lanes", "sweep_rows_pays", "sweep_pair_mode", "pair_path", "sweep_is_niw1"):
        assert not re.search(r"\b%s\(" % rule, abi), rule
    assert len(re.findall(r"\broute_sweep\(", abi)) == 1 and len(re.findall(r"\broute_score\(", abi)) == 2
    # ... and so are the routes of every other call (route_calls.hpp): the units and the kernel files hold none
    def code_of(name):
        return "\n".join(ln.split("//")[0] for ln in open(os.path.join(CSRC, name)).read().splitlines())
    calls = code_of("route_calls.hpp")
    for word in ("msc_state", "msc_context", "msc_chains", "getenv", "hip"):
        assert word not in calls, word
    for unit in ("blocked.cpp", "predict.cpp", "chains.cpp"):
        assert not re.search(r"static\s+\w[\w:<> ]*\s+route_\w+\(", code_of(unit)), unit
    for name in sorted(os.listdir(CSRC)):
        if name.startswith("kernels_") and name.endswith(".hip"):
            assert not re.search(r"\bplan_chains_marginal\([^;{]*\)\s*\{", code_of(name)), name
            assert not re.search(r"^[\w:<>&\* ]+\bplan_\w+\([^;{]*\)\s*\{", code_of(name), re.M), name
    assert not re.search(r"^[\w:<>&\* ]*\broute_\w+\([^;{]*\)\s*\{", code_of("launchers.hpp"), re.M)
