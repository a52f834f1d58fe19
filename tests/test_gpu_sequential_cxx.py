"""C++ side of the sequential Gibbs sweep: mixture_state::gibbs_sweep_sequential (tests/cxx/test_sequential_gpu.cpp),
built against include/ and the library and run on the device; its assignment after two sweeps is then compared with the
Python call (State.sweep_sequential) from the same start, tables, seed and sweep."""
import os
import subprocess

import numpy as np
import pytest
import torch

import common_amd
from tests.test_cxx import LINK, ROOT, _cxx

SRC = os.path.join(ROOT, "tests", "cxx", "test_sequential_gpu.cpp")
ROW = np.dtype([("f0", np.bool_), ("f1", np.uint32), ("f2", np.float32), ("f3", np.int32)])
FEATS = [(common_amd.BB, 0), (common_amd.GP, 0), (common_amd.NICH, 0), (common_amd.DD, 4)]
K = 24


def test_mixture_state_sequential_extension_builds():
    _cxx(SRC, "test_sequential_gpu", LINK)


@pytest.mark.gpu
def test_gibbs_sweep_sequential_matches_the_python_call(gpu_ctx, tmp_path):
    exe = _cxx(SRC, "test_sequential_gpu", LINK)
    out = subprocess.check_output([exe, str(tmp_path)], timeout=300).decode()
    assert "test_sequential_gpu ok" in out

    def load(name, dt):
        return np.fromfile(str(tmp_path / name), dtype=dt)
    rows = load("rows.bin", ROW)
    z0, z_in, z_out = load("z0.bin", np.int32), load("z_in.bin", np.int32), load("z_out.bin", np.int32)
    assert (z_in == -1).sum() == 1 and (z_out >= 0).all()
    e = int(np.nonzero(z_in == -1)[0][0])
    view = common_amd.DataView.from_recarray(gpu_ctx, rows)
    st = common_amd.State(gpu_ctx, FEATS, K)
    for f in range(len(FEATS)):
        st.set_hp(f, load("hp%d.bin" % f, np.float32))
    st.set_alpha(1.0)
    zt = torch.from_numpy(z0.copy()).to(gpu_ctx.torch_device)
    st.accumulate(view, zt)
    st.entity_op(view, e, int(z0[e]), join=False, z=zt)       # (the C++ side's remove_value: the same tables, bit for bit)
    assert np.array_equal(zt.cpu().numpy(), z_in)
    st.sweep_sequential(view, zt, 31, 5, nsweeps=2)
    assert np.array_equal(zt.cpu().numpy(), z_out)
