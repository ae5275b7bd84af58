"""-m gpu: ``dv_reg_metrics`` against the float64 restatement of its two-pass arithmetic (``reg_metrics64`` of tests/kernel_ref.py).

Tolerance 1e-9 * max(1, |v|): the inputs are fp32, exact in float64, and only the ORDER of at most 2^17 float64 additions
differs between the kernel and numpy (n u ~ 1e-11); two orders of margin keep the test independent of the reduction tree."""
import numpy as np
import pytest
import torch

from tests import kernel_ref
from tests.golden import cases as C

pytestmark = pytest.mark.gpu


def _close(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    for g, w in zip(got, want):
        print('dv_reg_metrics %.17g   reference %.17g   |diff| %.3g' % (g, w, abs(g - w)))
        assert (np.isnan(g) and np.isnan(w)) or abs(g - w) <= 1e-9 * max(1.0, abs(w)), (got, want)


def _run(K, pred, y, sel=None, n=None, dev='cuda'):
    out = torch.full((3,), 7.0, dtype=torch.float64, device=dev)
    K.reg_metrics(out, pred, y, sel=sel, n=n)
    return out.cpu().numpy()


@pytest.fixture(scope='module')
def K():
    from drvae_amd import kernels
    return kernels


def test_reference_generated_case(K, dev):
    c = C.y_metric_cases()['Ycont']
    got = _run(K, torch.from_numpy(c['pred']).cuda(), torch.from_numpy(np.asarray(c['ylab'], np.float32)).cuda())
    _close(got, kernel_ref.reg_metrics64(c['pred'], np.asarray(c['ylab'], np.float32)))
    G = np.load(C.__file__.replace('cases.py', 'fit.npz'))
    for i, k in enumerate(('rmse', 'r2', 'pearr')):
        assert got[i] == pytest.approx(float(G['Ycont/' + k]), rel=1e-6)


@pytest.mark.parametrize('with_sel', [False, True])
@pytest.mark.parametrize('Y', [1, 3])
@pytest.mark.parametrize('n', [1, 7, 4097, 32768])
def test_random_against_fp64(K, dev, n, Y, with_sel):
    rs = np.random.RandomState(100 * n % 9973 + 10 * Y + int(with_sel))
    M = n + 5 if with_sel else n
    y = rs.rand(M, Y).astype(np.float32)
    p = (0.6 * y + 0.2 + 0.15 * rs.standard_normal((M, Y))).astype(np.float32)
    sel = rs.permutation(M)[:n].astype(np.int32) if with_sel else None
    got = _run(K, torch.from_numpy(p).cuda(), torch.from_numpy(y).cuda(),
               sel=torch.from_numpy(sel).cuda() if with_sel else None)
    _close(got, kernel_ref.reg_metrics64(p, y, sel=sel))


@pytest.mark.parametrize('Y', [1, 3])
def test_row_strides(K, dev, Y):
    """``pred`` / ``y`` as column ranges of wider buffers (the heads of one product; a row-padded target array)"""
    rs = np.random.RandomState(5)
    n = 1000
    wide_p = rs.standard_normal((n, 2 * Y + 3)).astype(np.float32)
    wide_y = rs.rand(n, Y + 1).astype(np.float32)
    tp, ty = torch.from_numpy(wide_p).cuda(), torch.from_numpy(wide_y).cuda()
    pv, yv = tp[:, 2:2 + Y], ty[:, :Y]
    assert not pv.is_contiguous() and not yv.is_contiguous()
    sel = rs.permutation(n)[:333].astype(np.int32)
    _close(_run(K, pv, yv), kernel_ref.reg_metrics64(wide_p[:, 2:2 + Y], wide_y[:, :Y]))
    _close(_run(K, pv, yv, sel=torch.from_numpy(sel).cuda()), kernel_ref.reg_metrics64(wide_p[:, 2:2 + Y], wide_y[:, :Y], sel=sel))
    _close(_run(K, pv, yv, n=17), kernel_ref.reg_metrics64(wide_p[:, 2:2 + Y], wide_y[:, :Y], n=17))


@pytest.mark.parametrize('n', [4097, 32768])
def test_targets_in_a_narrow_band(K, dev, n):
    """0.5 +- 1e-3: sum(y^2) - sum(y)^2 / n loses what the centred sums keep -- the reason for the two passes"""
    rs = np.random.RandomState(8)
    y = (0.5 + 1e-3 * (2 * rs.rand(n, 1) - 1)).astype(np.float32)
    p = (y + 3e-4 * rs.standard_normal((n, 1))).astype(np.float32)
    want = kernel_ref.reg_metrics64(p, y)
    assert 0.5 < want[2] < 1.0 and np.isfinite(want[1])
    _close(_run(K, torch.from_numpy(p).cuda(), torch.from_numpy(y).cuda()), want)


def test_edge_cases(K, dev):
    rs = np.random.RandomState(9)
    n, Y = 300, 3
    y = torch.from_numpy(rs.rand(n, Y).astype(np.float32)).cuda()
    p = torch.from_numpy(rs.rand(n, Y).astype(np.float32)).cuda()
    const = torch.full((n, Y), 0.3, device='cuda')
    v = _run(K, p, const)                       # constant target: no variance to explain, no correlation
    assert np.isfinite(v[0]) and np.isnan(v[1]) and np.isnan(v[2])
    _close(v, kernel_ref.reg_metrics64(p.cpu().numpy(), const.cpu().numpy()))
    v = _run(K, const, y)                       # constant prediction: r2 finite (<= 0), no correlation
    assert np.isfinite(v[0]) and np.isfinite(v[1]) and np.isnan(v[2])
    _close(v, kernel_ref.reg_metrics64(const.cpu().numpy(), y.cpu().numpy()))
    assert np.isnan(_run(K, p, y, n=0)).all()
    assert np.isnan(_run(K, p, y, sel=torch.zeros(0, dtype=torch.int32, device='cuda'))).all()


def test_two_calls_give_the_same_bits(K, dev):
    rs = np.random.RandomState(10)
    y = torch.from_numpy(rs.rand(32768, 3).astype(np.float32)).cuda()
    p = torch.from_numpy(rs.rand(32768, 3).astype(np.float32)).cuda()
    a, b = _run(K, p, y), _run(K, p, y)
    assert a.tobytes() == b.tobytes() and np.isfinite(a).all()


def test_capturable(K, dev):
    """no allocation, no synchronisation: the launch records into a graph, the replay reads the arrays as they are then"""
    rs = np.random.RandomState(11)
    y = torch.from_numpy(rs.rand(500, 1).astype(np.float32)).cuda()
    p = torch.from_numpy(rs.rand(500, 1).astype(np.float32)).cuda()
    out = torch.zeros(3, dtype=torch.float64, device='cuda')
    K.reg_metrics(out, p, y)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        K.reg_metrics(out, p, y)
    y.mul_(0.5)
    g.replay()
    _close(out.cpu().numpy(), kernel_ref.reg_metrics64(p.cpu().numpy(), y.cpu().numpy()))
