"""The chain ensemble's call tables, host side: common_amd/csrc/chains_layout.hpp built with the host compiler into
tests/cxx/test_chains_layout.cpp -- a program of its own that includes nothing else of the library -- and run, plain and
under the address and undefined-behaviour sanitizers; and what the sources of the staging must and must not hold.  No
device needed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "common_amd", "csrc")


def _code(name):
    """a source file of the host library without its // comments"""
    src = open(os.path.join(CSRC, name)).read()
    return "\n".join(ln.split("//")[0] for ln in src.splitlines())


@pytest.mark.parametrize("extra", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "sanitized"])
def test_chains_layout_host(tmp_path, extra):
    exe = str(tmp_path / "test_chains_layout")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC] + extra +
                          [os.path.join(ROOT, "tests", "cxx", "test_chains_layout.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert out.returncode == 0, out.stdout
    assert "chains layout ok" in out.stdout


def test_layout_is_host_only():
    code = _code("chains_layout.hpp")
    for word in ("hip", "msc_state", "#include \""):
        assert word not in code, word


def test_one_refusal_and_one_way_into_a_staging_area():
    """chains.cpp words the mid-step refusal once, and reaches pinned staging memory only through StagedUpload::begin,
    whose result is typed: it holds no pinned buffer, event or copy of its own, and casts nothing it reads off the upload"""
    src = open(os.path.join(CSRC, "chains.cpp")).read()
    assert src.count("is between msc_sweep_step_begin and") == 1
    code = _code("chains.cpp")
    for word in ("PinnedBuf", "hipHostMalloc", "hipEvent", "hipMemcpyAsync(ch->call_tab"):
        assert word not in code, word
    for cast in re.findall(r"reinterpret_cast<[^>]*>\(([^;]*?)\)", code):
        assert "upload" not in cast and "stage" not in cast, cast
    # every table goes up through the one upload into the one device buffer
    assert len(re.findall(r"upload\.begin\(", code)) == len(re.findall(r"upload\.commit\(s, (?:ch->call_tab|dev),", code)) == 6


def test_events_are_recorded_in_one_place():
    """among the host files hipEventRecord stands in dev_buf.hpp (StagedUpload) and in abi.cpp's timing code alone"""
    holders = set()
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".cpp", ".hpp")) and "hipEventRecord" in _code(name):
            holders.add(name)
    assert holders == {"abi.cpp", "dev_buf.hpp"}, holders
    assert _code("dev_buf.hpp").count("hipEventRecord") == 1
