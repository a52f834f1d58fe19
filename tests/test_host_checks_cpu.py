"""The library's checks of host arrays, host side: common_amd/csrc/host_checks.hpp built with the host compiler into
tests/cxx/test_host_checks.cpp -- a program of its own that includes nothing else of the library -- and run, plain and
under the address and undefined-behaviour sanitizers.  No device needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "common_amd", "csrc")


@pytest.mark.parametrize("extra", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "sanitized"])
def test_host_checks_host(tmp_path, extra):
    exe = str(tmp_path / "test_host_checks")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC] + extra +
                          [os.path.join(ROOT, "tests", "cxx", "test_host_checks.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert out.returncode == 0, out.stdout
    assert "host_checks ok" in out.stdout


def test_header_is_host_only():
    """standard headers only: no HIP header, nothing of the library"""
    src = open(os.path.join(CSRC, "host_checks.hpp")).read()
    includes = [ln.split()[1] for ln in src.splitlines() if ln.startswith("#include")]
    assert includes == ["<cstdint>", "<cstdio>", "<vector>"], includes


def test_every_order_check_uses_it():
    """one definition of the loop: the three entry points that take a visiting order call the header's"""
    src = open(os.path.join(CSRC, "summary.cpp")).read()
    assert src.count("require_permutation(host_order, ") == 3
    for name in os.listdir(CSRC):
        if name.endswith((".cpp", ".hip", ".hpp")) and name != "host_checks.hpp":
            assert "is not a permutation" not in open(os.path.join(CSRC, name)).read(), name
