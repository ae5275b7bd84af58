"""CPU: ``dv_reg_metrics`` -- the C-ABI declaration, its argument checks without a GPU, and the float64 restatement of its
two-pass arithmetic (``reg_metrics64`` of tests/kernel_ref.py) against the reference's own numbers (the kernel itself:
tests/test_gpu_reg_metrics.py)."""
import os
import re

import numpy as np
import pytest

from tests import kernel_ref
from tests.golden import cases as C

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def test_entry_point_is_declared_and_the_abi_is_additive():
    from drvae_amd import _lib
    assert 'dv_reg_metrics' in _lib.SIGNATURES and len(_lib.SIGNATURES['dv_reg_metrics']) == 9
    with open(os.path.join(os.path.dirname(os.path.dirname(GOLDEN)), 'include', 'drvae_hip.h')) as f:
        src = f.read()
    assert _lib.ABI_VERSION == int(re.search(r'#define DV_ABI_VERSION (\d+)', src).group(1))


def test_entry_point_rejects_bad_arguments_without_gpu():
    import ctypes as Ct
    from drvae_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    assert lib.dv_reg_metrics(None, 1, None, 1, None, 4, 1, None, None) == -1
    buf = (Ct.c_double * 8)()           # (never dereferenced: the arguments are refused before anything is launched)
    ptr = Ct.cast(buf, Ct.c_void_p)
    assert lib.dv_reg_metrics(ptr, 1, ptr, 1, None, 4, 0, ptr, None) == -1          # Y = 0
    assert lib.dv_reg_metrics(ptr, 1, ptr, 1, None, -1, 1, ptr, None) == -1         # n < 0
    assert lib.dv_reg_metrics(ptr, 1, None, 1, None, 4, 1, ptr, None) == -1         # no targets
    assert lib.dv_reg_metrics(ptr, 1, ptr, 1, None, 4, 1, None, None) == -1         # no output


def test_two_pass_reference_reproduces_the_reference_generated_metrics():
    c = C.y_metric_cases()['Ycont']
    G = np.load(os.path.join(GOLDEN, 'fit.npz'))
    got = kernel_ref.reg_metrics64(c['pred'], c['ylab'])
    for i, k in enumerate(('rmse', 'r2', 'pearr')):
        assert got[i] == pytest.approx(float(G['Ycont/' + k]), rel=1e-6)


def test_two_pass_reference_edge_cases_and_selection():
    rs = np.random.RandomState(0)
    y, p = rs.rand(20, 3).astype(np.float32), rs.rand(20, 3).astype(np.float32)
    sel = np.array([3, 1, 17, 4])
    np.testing.assert_array_equal(kernel_ref.reg_metrics64(p, y, sel=sel), kernel_ref.reg_metrics64(p[sel], y[sel]))
    np.testing.assert_array_equal(kernel_ref.reg_metrics64(p, y, n=5), kernel_ref.reg_metrics64(p[:5], y[:5]))
    assert np.isnan(kernel_ref.reg_metrics64(p, y, n=0)).all()
    const = np.full_like(y, 0.3)
    v = kernel_ref.reg_metrics64(p, const)
    assert np.isfinite(v[0]) and np.isnan(v[1]) and np.isnan(v[2])
    v = kernel_ref.reg_metrics64(const, y)
    assert np.isfinite(v[0]) and np.isfinite(v[1]) and np.isnan(v[2])
    # against the host function the step-by-step evaluation uses
    import torch
    from drvae_amd import metrics as MET
    h = MET.eval_y_regression(torch.from_numpy(p), torch.from_numpy(y))
    np.testing.assert_allclose(kernel_ref.reg_metrics64(p, y), [h['rmse'], h['r2'], h['pearr']], rtol=1e-12)
