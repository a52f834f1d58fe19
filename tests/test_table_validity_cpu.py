"""The state's table-validity bookkeeping, host side: common_amd/csrc/table_validity.hpp built with the host compiler
into tests/cxx/test_table_validity.cpp -- a program of its own that includes nothing else of the library -- and run: the
flags after every event from two starts, the snapshot round trip, which events drop a blocked draw.  No device needed."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "common_amd", "csrc")


def test_table_validity_host(tmp_path):
    exe = str(tmp_path / "test_table_validity")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cxx", "test_table_validity.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert out.returncode == 0, out.stdout
    assert "table_validity ok" in out.stdout


def test_header_is_host_only():
    """no HIP header, nothing of the library: the one include of the program above is all it needs"""
    src = open(os.path.join(CSRC, "table_validity.hpp")).read()
    includes = [ln.split()[1] for ln in src.splitlines() if ln.startswith("#include")]
    assert includes == ["<cstddef>", "<vector>"], includes
