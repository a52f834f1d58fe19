"""C++ side of the blocked Gibbs sweep: mixture_state::gibbs_sweep_blocked (tests/cxx/test_blocked_gpu.cpp), built
against include/ and the library and run on the device: the host partition follows the device's counts, and a bbnc
component throws."""
import os
import subprocess

import pytest

from tests.test_cxx import LINK, ROOT, _cxx

SRC = os.path.join(ROOT, "tests", "cxx", "test_blocked_gpu.cpp")


def test_mixture_state_blocked_extension_builds():
    _cxx(SRC, "test_blocked_gpu", LINK)


@pytest.mark.gpu
def test_gibbs_sweep_blocked_keeps_the_host_partition_in_step(gpu_ctx):
    exe = _cxx(SRC, "test_blocked_gpu", LINK)
    out = subprocess.check_output([exe], timeout=300).decode()
    assert "test_blocked_gpu ok" in out
