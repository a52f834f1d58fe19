"""C++ side of posterior predictive sampling: mixture_state::sample_post_pred (tests/cxx/test_predictive_gpu.cpp), built
against include/ and the library and run on the device; its masked entries and groups are then compared with the Python
call (State.impute, z = None) on the same tables, rows, seed and sweep."""
import os
import subprocess

import numpy as np
import pytest
import torch

import common_amd
from tests.test_cxx import LINK, ROOT, _cxx

SRC = os.path.join(ROOT, "tests", "cxx", "test_predictive_gpu.cpp")
ROW = np.dtype([("f0", np.bool_), ("f1", np.uint32), ("f2", np.float32), ("f3", np.int32)])
FEATS = [(common_amd.BB, 0), (common_amd.GP, 0), (common_amd.NICH, 0), (common_amd.DD, 4)]
K = 16


def test_mixture_state_predictive_extension_builds():
    _cxx(SRC, "test_predictive_gpu", LINK)


@pytest.mark.gpu
def test_sample_post_pred_keeps_observed_bytes_and_matches_the_python_call(gpu_ctx, tmp_path):
    exe = _cxx(SRC, "test_predictive_gpu", LINK)
    out = subprocess.check_output([exe, str(tmp_path)], timeout=300).decode()
    assert "test_predictive_gpu ok" in out

    def load(name, dt):
        return np.fromfile(str(tmp_path / name), dtype=dt)
    rows, got = load("rows.bin", ROW), load("out.bin", ROW)
    mask = load("mask.bin", np.uint8).reshape(-1, 4).astype(bool)
    groups = load("groups.bin", np.int32)
    st = common_amd.State(gpu_ctx, FEATS, K)
    for f, (fam, dim) in enumerate(FEATS):
        st.set_hp(f, load("hp%d.bin" % f, np.float32))
        st.set_ss(f, load("ss%d.bin" % f, common_amd.ss_dtype(fam, dim)))
    st.set_group_counts(load("counts.bin", np.uint32))
    st.set_alpha(1.0)
    mrec = np.zeros(rows.shape[0], dtype=[(n, np.bool_) for n in ROW.names])
    for f, n in enumerate(ROW.names):
        mrec[n] = mask[:, f]
    view = common_amd.DataView.from_recarray(gpu_ctx, np.ma.masked_array(rows, mask=mrec))
    cols, g = st.impute(view, seed=77, sweep=4)
    torch.cuda.synchronize()
    assert np.array_equal(g.cpu().numpy(), groups)
    for f, n in enumerate(ROW.names):
        py = cols[f].cpu().numpy()
        m = mask[:, f]
        assert np.array_equal(np.asarray(got[n][m]).astype(py.dtype), py[m]), n
        assert np.array_equal(got[n][~m], rows[n][~m]), n
