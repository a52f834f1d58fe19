"""C++ side of slice sampling: mixture_state::slice_component_hp / slice_cluster_hp / slice_theta
(tests/cxx/test_slice_gpu.cpp), built against include/ and the library, run on the device."""
import os
import subprocess

import pytest

from tests.test_cxx import LINK, ROOT, _audited, _cxx


def test_mixture_state_slice_extension_builds():
    _cxx(os.path.join(ROOT, "tests", "cxx", "test_slice_gpu.cpp"), "test_slice_gpu", LINK)


@pytest.mark.gpu
def test_mixture_state_slice_steps_install_their_values():
    exe = _cxx(os.path.join(ROOT, "tests", "cxx", "test_slice_gpu.cpp"), "test_slice_gpu", LINK)
    out = subprocess.check_output([exe], timeout=300).decode()
    assert "test_slice_gpu ok" in out and _audited(out) >= 2
