"""The library's row-range test, host side: common_amd/csrc/row_range.hpp built with the host compiler into
tests/cxx/test_row_range.cpp -- a program of its own that includes nothing else of the library -- and run, plain and
under the address and undefined-behaviour sanitizers.  No device needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "common_amd", "csrc")


@pytest.mark.parametrize("extra", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "sanitized"])
def test_row_range_host(tmp_path, extra):
    exe = str(tmp_path / "test_row_range")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC] + extra +
                          [os.path.join(ROOT, "tests", "cxx", "test_row_range.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert out.returncode == 0, out.stdout
    assert "row_range ok" in out.stdout


def test_header_is_host_only():
    """no HIP header, nothing of the library"""
    src = open(os.path.join(CSRC, "row_range.hpp")).read()
    includes = [ln.split()[1] for ln in src.splitlines() if ln.startswith("#include")]
    assert includes == ["<cstdint>"], includes


def test_bind_view_uses_it():
    src = open(os.path.join(CSRC, "abi.cpp")).read()
    assert "msc::rows_within(row0, nrows, view->nrows)" in src and "row0 + nrows <= view->nrows" not in src
