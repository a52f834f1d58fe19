"""C++ side of the log joint: mixture_state::score_joint() (tests/cxx/test_score_joint_gpu.cpp), built against include/
and the library, run on the device."""
import os
import subprocess

import pytest

from tests.test_cxx import LINK, ROOT, _audited, _cxx


def test_mixture_state_score_joint_builds():
    _cxx(os.path.join(ROOT, "tests", "cxx", "test_score_joint_gpu.cpp"), "test_score_joint_gpu", LINK)


@pytest.mark.gpu
def test_mixture_state_score_joint_is_the_abi_total():
    exe = _cxx(os.path.join(ROOT, "tests", "cxx", "test_score_joint_gpu.cpp"), "test_score_joint_gpu", LINK)
    out = subprocess.check_output([exe], timeout=300).decode()
    assert "test_score_joint_gpu ok" in out and _audited(out) >= 2
