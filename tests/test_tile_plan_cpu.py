"""The tile planner, host side: common_amd/csrc/tile_plan.hpp (with feat_desc.hpp and route.hpp) built with the host
compiler into tests/cxx/test_tile_plan.cpp -- a program of its own that includes nothing else of the library -- and run,
plain and under the address and undefined-behaviour sanitizers.  No device needed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "common_amd", "csrc")
HOST_ONLY = ("feat_desc.hpp", "tile_plan.hpp", "route.hpp")


@pytest.mark.parametrize("extra", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "sanitized"])
def test_tile_plan_host(tmp_path, extra):
    exe = str(tmp_path / "test_tile_plan")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC] + extra +
                          [os.path.join(ROOT, "tests", "cxx", "test_tile_plan.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert out.returncode == 0, out.stdout
    assert "tile_plan ok" in out.stdout


def test_headers_are_host_only():
    """standard headers, the public C header and each other only: no HIP header, nothing else of the library"""
    for name in HOST_ONLY:
        src = open(os.path.join(CSRC, name)).read()
        assert "hip/" not in src and "__global__" not in src, name
        for inc in re.findall(r"^\s*#\s*include\s+(\S+)", src, re.M):
            ok = re.fullmatch(r"<[a-z_]+>", inc) or inc == '"../../include/microscopes_hip.h"' or inc.strip('"') in HOST_ONLY
            assert ok, (name, inc)
    public = open(os.path.join(ROOT, "include", "microscopes_hip.h")).read()
    assert all(re.fullmatch(r"<[a-z_.]+>", inc) for inc in re.findall(r"^\s*#\s*include\s+(\S+)", public, re.M))


def test_the_state_keeps_one_plan():
    """the planner's results are one member, written by one assignment; no unit reads a loose field"""
    fields = ("tile_split|fuse_nfeat|fuse_split|fuse_any|nich_blocks_any|tile_path|plan_cost|tile_narrow_tail_ok|"
              "tail_max_rows|tail_pack_rows|tail_masked_nich|tail_dm|loo_staged")
    for name in os.listdir(CSRC):
        if name.endswith((".cpp", ".hip", ".hpp")):
            src = open(os.path.join(CSRC, name)).read()
            assert not re.search(r"\bst->(%s)\b" % fields, src), name
    assert len(re.findall(r"\bst->plan = ", open(os.path.join(CSRC, "abi.cpp")).read())) == 1
