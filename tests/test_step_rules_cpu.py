"""The sweep step's host bookkeeping: common_amd/csrc/step_rules.hpp (the mirror of the device's (seed, sweep) pair and the
step graph's rules) built with the host compiler into tests/cxx/test_step_rules.cpp -- a program of its own that includes
nothing else of the library -- and run, plain and under the address and undefined-behaviour sanitizers.  No device needed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "common_amd", "csrc")


@pytest.mark.parametrize("extra", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "sanitized"])
def test_step_rules_host(tmp_path, extra):
    exe = str(tmp_path / "test_step_rules")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC] + extra +
                          [os.path.join(ROOT, "tests", "cxx", "test_step_rules.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert out.returncode == 0, out.stdout
    assert "step_rules ok" in out.stdout


def test_header_is_host_only():
    """no HIP header, nothing of the library: standard headers alone"""
    src = open(os.path.join(CSRC, "step_rules.hpp")).read()
    includes = [ln.split()[1] for ln in src.splitlines() if ln.startswith("#include")]
    assert includes == ["<cstdint>", "<vector>"], includes


def test_the_header_owns_the_mirror_and_the_executable_has_one_destroyer():
    """no unit names a field of the mirror, and abi.cpp destroys a captured step in drop_step_graph alone"""
    old = re.compile(r"\brng_(valid|seed|sweep|bump_pending|next_sweep)\b")
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".cpp", ".hpp", ".hip")):
            assert not old.search(open(os.path.join(CSRC, name)).read()), name
    abi = open(os.path.join(CSRC, "abi.cpp")).read()
    assert abi.count("hipGraphExecDestroy") == 1
    assert abi.index("static void drop_step_graph") < abi.index("hipGraphExecDestroy") < abi.index('extern "C" int msc_state_destroy')
