"""C++ side of the split-merge move: mixture_state::split_merge (tests/cxx/test_split_merge_gpu.cpp), built against
include/ and the library and run on the device: one accepted split and one accepted merge, the host partition in step with
the device's counts, score_data of every group against plugin groups fed the state's own suff-stats."""
import os
import subprocess

import pytest

from tests.test_cxx import LINK, ROOT, _audited, _cxx

SRC = os.path.join(ROOT, "tests", "cxx", "test_split_merge_gpu.cpp")


def test_mixture_state_split_merge_builds():
    _cxx(SRC, "test_split_merge_gpu", LINK)


@pytest.mark.gpu
def test_split_merge_keeps_the_host_partition_in_step(gpu_ctx):
    exe = _cxx(SRC, "test_split_merge_gpu", LINK)
    out = subprocess.check_output([exe], timeout=300).decode()
    assert "test_split_merge_gpu ok" in out and _audited(out) >= 1
