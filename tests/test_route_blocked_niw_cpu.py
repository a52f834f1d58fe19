"""The blocked sweep's niw route, host side: common_amd/csrc/route_calls.hpp built with the host compiler into
tests/cxx/test_route_blocked_niw.cpp -- a program of its own that includes nothing else of the library -- and run, plain
and under the address and undefined-behaviour sanitizers.  No device needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "common_amd", "csrc")


@pytest.mark.parametrize("extra", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "sanitized"])
def test_route_blocked_niw_host(tmp_path, extra):
    exe = str(tmp_path / "test_route_blocked_niw")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC] + extra +
                          [os.path.join(ROOT, "tests", "cxx", "test_route_blocked_niw.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert out.returncode == 0, out.stdout
    assert "route blocked niw ok" in out.stdout
