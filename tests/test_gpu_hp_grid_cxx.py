"""C++ side of grid hyper-parameter inference: mixture_state::score_likelihood_grid / grid_component_hp /
grid_cluster_hp (tests/cxx/test_hp_grid_gpu.cpp), built against include/ and the library, run on the device."""
import os
import subprocess

import pytest

from tests.test_cxx import LINK, ROOT, _audited, _cxx


def test_mixture_state_grid_extension_builds():
    _cxx(os.path.join(ROOT, "tests", "cxx", "test_hp_grid_gpu.cpp"), "test_hp_grid_gpu", LINK)


@pytest.mark.gpu
def test_mixture_state_grid_steps_install_the_chosen_point():
    exe = _cxx(os.path.join(ROOT, "tests", "cxx", "test_hp_grid_gpu.cpp"), "test_hp_grid_gpu", LINK)
    out = subprocess.check_output([exe], timeout=300).decode()
    assert "test_hp_grid_gpu ok" in out and _audited(out) >= 1
