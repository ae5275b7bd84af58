"""GPU: ``dv_rank_metrics`` against the exact rank reference of ``tests/eval_gauss_ref.py``: ROC-AUC bit-equal to the exact
rational, average precision within 1e-12 (n float64 additions of values <= 1 with n <= 2^15: n 2^-53 ~ 4e-12 at the very
worst, the tolerance ``test_rank_metrics_without_a_sort`` has held), accuracy = hits / n in fp32 -- at the tile edges of
``pair_counts_kernel`` (256 rows per workgroup, 512-row j-tiles) up to the documented maximum, over tie-heavy, saturated,
signed-zero and subnormal scores, with ``proba`` as a column range of a wider buffer, an unsorted ``sel`` into a larger set,
and guard bands around ``counts`` and ``out``."""
import numpy as np
import pytest
import torch

from tests import eval_gauss_ref as G
from tests.test_eval_gauss_cpu import RANK_MODES, RANK_NS
from tests.test_gpu_gene_disp import GUARD, SENTINEL, host

pytestmark = pytest.mark.gpu

AP_TOL = 1e-12
f = np.float32


@pytest.fixture(scope='module')
def K(dev):
    import drvae_amd.kernels as K
    from drvae_amd import _lib
    _lib.load()
    return K


def _banded_out(n_out, dev):
    big = torch.full((n_out + 2 * GUARD,), SENTINEL, dtype=torch.float64, device=dev)
    return big[GUARD:GUARD + n_out], big


def _banded_counts(n_cls, n, dev):
    """zeroed counts between two bands of a nonzero sentinel"""
    big = torch.full((n_cls * n * 4 + 2 * GUARD,), 7, dtype=torch.int32, device=dev)
    big[GUARD:GUARD + n_cls * n * 4] = 0
    return big[GUARD:GUARD + n_cls * n * 4], big


def _counts_ok(big, m):
    b = host(big)
    return bool((b[:GUARD] == 7).all() and (b[GUARD + m:] == 7).all() and (b[GUARD:GUARD + m] == 0).all())


def _out_ok(big, m):
    b = host(big)
    return bool((b[:GUARD] == SENTINEL).all() and (b[GUARD + m:] == SENTINEL).all())


def run(K, dev, proba, y, pred, sel, c0, n_cls, binary, wide=True):
    """two calls on the same buffers (the counts come back zeroed): identical bytes -> out (2 n_cls + 1) float64"""
    n_all, Y = proba.shape
    n = len(sel) if sel is not None else n_all
    if wide:          # proba as a column range of a wider buffer: ldp > Y
        buf = torch.full((n_all, Y + 3), SENTINEL, device=dev)
        buf[:, 2:2 + Y] = torch.from_numpy(proba).to(dev)
        pd = buf[:, 2:2 + Y]
        assert host(pd).numpy().tobytes() == proba.tobytes()          # (signed zeros and subnormals arrive as they are)
    else:
        buf = pd = torch.from_numpy(proba).to(dev)
    buf0 = buf.clone()
    yd = torch.from_numpy(y).to(dev)
    prd = torch.from_numpy(pred).to(dev) if pred is not None else None
    sd = torch.from_numpy(sel).to(dev) if sel is not None else None
    rows = max(n, 1)          # (never an empty buffer: the launch is given a pointer)
    counts, cbig = _banded_counts(n_cls, rows, dev)
    outs = []
    for rep in range(2):
        out, obig = _banded_out(2 * n_cls + 1, dev)
        K.rank_metrics(out, counts, pd, yd, pred32=prd, sel=sd, c0=c0, n_cls=n_cls, binary=binary)
        outs.append(host(out).numpy().copy())
        assert _counts_ok(cbig, n_cls * rows * 4) and _out_ok(obig, 2 * n_cls + 1)
    assert outs[0].tobytes() == outs[1].tobytes()
    assert torch.equal(buf, buf0) and np.array_equal(host(yd).numpy(), y)
    return outs[0]


def compare(got, want, n_cls, where):
    worst_ap = 0.0
    for c in range(n_cls):
        a, b = got[2 * c], want[2 * c]
        assert (np.isnan(a) and np.isnan(b)) or a == b, ('ROC-AUC is not the exact rational', where, c, a, b)
        assert abs(got[2 * c + 1] - want[2 * c + 1]) <= AP_TOL, ('AP', where, c, got[2 * c + 1], want[2 * c + 1])
        worst_ap = max(worst_ap, abs(got[2 * c + 1] - want[2 * c + 1]))
    a, b = got[2 * n_cls], want[2 * n_cls]
    assert (np.isnan(a) and np.isnan(b)) or a == b, ('accuracy', where, a, b)          # hits / n, one fp32 division: the same bits
    return worst_ap


@pytest.mark.parametrize('mode', RANK_MODES, ids=['binary', 'three_classes', 'class_subset'])
@pytest.mark.parametrize('n', RANK_NS)
def test_rank_metrics_against_the_exact_reference(K, dev, n, mode):
    Y, c0, n_cls, binary = mode
    worst = 0.0
    for pattern in G.RANK_PATTERNS:
        proba, y, pred, sel = G.rank_case(n, pattern, Y)
        want = G.rank_expected(proba, y, pred, sel, c0, n_cls, binary)
        got = run(K, dev, proba, y, pred, sel, c0, n_cls, binary)
        worst = max(worst, compare(got, want, n_cls, (n, mode, pattern)))
        if pattern == 'equal':
            for c in range(n_cls):
                assert np.isnan(want[2 * c]) or got[2 * c] == 0.5
    print('dv_rank_metrics n = %d %s: worst |AP - reference| %.3g (tolerance %g); AUC and accuracy bit-equal' % (n, mode, worst, AP_TOL))


def test_signed_zeros_tie_and_subnormals_rank(K, dev):
    y = np.asarray([1, 0], np.int32)
    for scores, auc, ap in (([-0.0, 0.0], 0.5, 0.5), ([0.0, -0.0], 0.5, 0.5), ([2e-40, 1e-40], 1.0, 1.0), ([1e-40, 2e-40], 0.0, 0.5),
                            ([1e-45, 0.0], 1.0, 1.0), ([-1e-45, -0.0], 0.0, 0.5)):
        proba = np.stack([np.zeros(2, f), np.asarray(scores, f)], 1)
        got = run(K, dev, proba, y, y, None, 1, 1, True, wide=False)
        assert got[0] == auc and got[1] == ap, (scores, got)
        assert (got[0], got[1]) == G.rank_reference(proba[:, 1], y > 0)


def test_no_sel_and_contiguous_proba(K, dev):
    for n in (257, 513):
        proba, y, pred, _ = G.rank_case(n, 'grid3', 3, extra=0)
        want = G.rank_expected(proba, y, pred, None, 0, 3, False)
        compare(run(K, dev, proba, y, pred, None, 0, 3, False, wide=False), want, 3, (n, 'no sel'))


def test_degenerate_cases_and_the_accuracy_without_a_prediction(K, dev):
    """one class only: AUC nan (AP 1 with positives only, 0 with none); no rows: nan, 0, nan; ``pred`` None: the accuracy slot is nan
    -- no prediction given is not 0 % correct -- and nothing else changes"""
    proba, y, pred, sel = G.rank_case(300, 'continuous', 2)
    ones, zeros = np.ones_like(y), np.zeros_like(y)
    got = run(K, dev, proba, ones, pred, sel, 1, 1, True)
    assert np.isnan(got[0]) and got[1] == 1.0
    got = run(K, dev, proba, zeros, pred, sel, 1, 1, True)
    assert np.isnan(got[0]) and got[1] == 0.0
    got = run(K, dev, proba, y, pred, sel[:0], 1, 1, True)
    assert np.isnan(got[0]) and got[1] == 0.0 and np.isnan(got[2])
    with_pred = run(K, dev, proba, y, pred, sel, 1, 1, True)
    without = run(K, dev, proba, y, None, sel, 1, 1, True)
    assert np.isnan(G.ACC_WITHOUT_PRED) and np.isnan(without[2]) and not np.isnan(with_pred[2])
    assert without[:2].tobytes() == with_pred[:2].tobytes()
    compare(without, G.rank_expected(proba, y, None, sel, 1, 1, True), 1, 'pred=None')
    proba, y, pred, sel = G.rank_case(300, 'grid3', 3)
    without = run(K, dev, proba, y, None, sel, 0, 3, False)
    compare(without, G.rank_expected(proba, y, None, sel, 0, 3, False), 3, 'pred=None, three classes')


def test_more_rows_than_the_maximum_are_refused(K, dev):
    """n = DV_RANK_MAX_ROWS + 1: DV_ERR_UNSUPPORTED (a RuntimeError of the launcher), ``out`` and ``counts`` untouched"""
    from drvae_amd import _lib
    n = K.RANK_MAX_ROWS + 1
    assert n == G.RANK_MAX_ROWS + 1 == 32769
    proba, y, pred, _ = G.rank_case(n, 'continuous', 2, extra=0)
    counts, cbig = _banded_counts(1, n, dev)
    out, obig = _banded_out(3, dev)
    pd, yd, prd = torch.from_numpy(proba).to(dev), torch.from_numpy(y).to(dev), torch.from_numpy(pred).to(dev)
    with pytest.raises(RuntimeError):
        K.rank_metrics(out, counts, pd, yd, pred32=prd)
    rc = _lib.load().dv_rank_metrics(pd.data_ptr(), 2, yd.data_ptr(), prd.data_ptr(), None, n, 1, 1, 1, counts.data_ptr(), out.data_ptr(), None)
    assert rc == -3          # DV_ERR_UNSUPPORTED
    assert _counts_ok(cbig, n * 4) and bool((host(obig) == SENTINEL).all())
