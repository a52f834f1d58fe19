"""C++ side of the row predictive log-density: mixture_state::log_post_pred (tests/cxx/test_log_post_pred_gpu.cpp), built
against include/ and the library and run on the device; logp, the MAP slot and its log responsibility of new, partly
masked rows against the host plugin groups fed the state's own suff-stats, through tests/cxx/audit.hpp."""
import os
import subprocess

import pytest

from tests.test_cxx import LINK, ROOT, _audited, _cxx

SRC = os.path.join(ROOT, "tests", "cxx", "test_log_post_pred_gpu.cpp")


def test_mixture_state_log_post_pred_builds():
    _cxx(SRC, "test_log_post_pred_gpu", LINK)


@pytest.mark.gpu
def test_log_post_pred_matches_the_host_twin(gpu_ctx):
    exe = _cxx(SRC, "test_log_post_pred_gpu", LINK)
    out = subprocess.check_output([exe], timeout=300).decode()
    assert "test_log_post_pred_gpu ok" in out
    assert _audited(out) == 2
