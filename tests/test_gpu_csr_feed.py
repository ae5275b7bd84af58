"""GPU: the sparse (CSR) batch feed on the real kernels -- ``dv_batch_feed`` with ``csr1_*`` / ``csr2_*`` against the dense launch
on the densified matrix, bit for bit on integer counts (every width at which the kernel changes path, every row layout, both
access paths, x1 / x2 / both sparse, plain and split forms, transforms 0 / 1 / 3, the label outputs, guard bands, run to run);
non-integer values; an out-of-range column; ``gather_rows``; the fused step on a ``CsrRows`` dataset against the densified one
(eager, captured, ``feed()``); ``fit`` and evaluation.  Helpers and what is held to what: ``tests/csr_feed_ref.py``."""
import itertools
import types
import warnings

import numpy as np
import pytest
import torch

from tests import csr_feed_ref as CF
from tests import ref64
from tests.test_gpu_counts import SENTINEL

pytestmark = pytest.mark.gpu

SIGMA = 0.01
SIZES = [(B, Np) for B in range(1, 10) for Np in sorted({0, 1, B})]       # B in 1 .. 9 with Np in {0, 1, B}
FORMS = {'plain': None, 'split-t0': 0, 'split-log1p': 'log1p', 'split-norm': 'log1p_norm'}
WHICH = ('x1', 'x2', 'both')
N_BATCHES, Y, YC, L = 3, 3, 2, 2
CTRS = (-2, 1, 7)                 # ctr - base: clamped below, inside, clamped above


@pytest.fixture(scope='module')
def K(dev):
    import drvae_amd.kernels as K
    from drvae_amd import _lib
    _lib.load()
    assert _lib.BatchFeed._fields_[-1][0] == 'csr2_val'
    return K


def _i32(a, dev):
    return torch.from_numpy(np.asarray(a, np.int32)).to(dev)


def _buffer(rows, X, off, dev, fill=None):
    """a (rows, X) view inside a sentinel-filled buffer, one guard row above and below and padding behind every row; ``off`` = 1:
    the view starts one float behind a 16-byte boundary (the scalar path).  Returns (view, whole buffer)"""
    ld = (X + 3) // 4 * 4 + 4
    big = torch.full(((rows + 2) * ld + 8,), SENTINEL, device=dev)
    view = big[off:off + (rows + 2) * ld].view(rows + 2, ld)[1:rows + 1, :X]
    assert (view.data_ptr() % 16 == 0) == (off == 0)
    if fill is not None:
        view.copy_(fill)
    return view, big


def _guards_intact(view, big):
    inner = view.clone()
    view.fill_(SENTINEL)
    ok = bool((big == SENTINEL).all())
    view.copy_(inner)
    return ok


class _Launch:
    """one geometry of the launch: table, pair rows, label inputs -- and fresh sentinel-filled outputs for every call"""

    def __init__(self, K, dev, X, B, Np, off, noisy, ctr, transform, split):
        self.K, self.dev, self.X, self.B, self.Np, self.off = K, dev, X, B, Np, off
        rs = np.random.RandomState(X * 100 + B * 10 + Np)
        tab = rs.randint(0, CF.N_SRC, (N_BATCHES, B))
        if B > 1:
            tab[:, 1] = tab[:, 0]                    # (a table that repeats a row)
        self.table = _i32(tab, dev)
        self.tab = tab[min(max(ctr, 0), N_BATCHES - 1)]
        self.pr = np.arange(B)[::-1][:Np].copy()
        self.pair_rows = _i32(self.pr, dev) if Np else None
        self.ctr, self.base = _i32([ctr + 5], dev), _i32([5], dev)
        self.noise = _buffer(B + Np, X, off, dev, torch.randn(B + Np, X, device=dev))[0] if noisy else None
        self.transform, self.split = transform, split
        Mf = 2 * B
        self.lab = dict(has_y=_i32(rs.randint(0, 2, B), dev), L=L, fp_i=_i32(np.arange(Mf) % B, dev),
                        fp_lab=_i32(np.arange(Mf) % 2, dev), fp_slot=_i32(np.arange(Mf) % Y, dev), n_classes=Y,
                        yf=torch.from_numpy(rs.randn(CF.N_SRC, YC).astype(np.float32)).to(dev))
        self.y32 = _i32(rs.randint(0, Y, CF.N_SRC), dev)
        self.Mf = Mf

    def __call__(self, x1, x2):
        """returns every output of the launch: (xin, xt or None, label_r, fp_cls, onehot, onehot2, ylab) and the buffers"""
        dev, B, Np, X = self.dev, self.B, self.Np, self.X
        xin, xin_big = _buffer(B + Np, X, self.off, dev)
        xt, xt_big = _buffer(B + Np, X, 0, dev) if self.split else (None, None)      # (xt must be 16-byte aligned)
        out = dict(label_r=torch.full((L * B,), -7, dtype=torch.int32, device=dev),
                   fp_cls=torch.full((self.Mf,), -7, dtype=torch.int32, device=dev),
                   onehot=torch.full((self.Mf, Y + 1), SENTINEL, device=dev)[:, :Y],
                   onehot2=torch.full((self.Mf, Y + 2), SENTINEL, device=dev)[:, :Y],
                   ylab=torch.full((B, YC), SENTINEL, device=dev))
        kw = dict(xt=xt, transform=self.transform) if self.split else {}
        self.K.batch_feed(xin, x1, x2 if Np else None, self.y32, self.table, N_BATCHES, self.ctr, self.base,
                          pair_rows=self.pair_rows, noise=self.noise, sigma=SIGMA if self.noise is not None else 0.0,
                          **self.lab, **out, **kw)
        return dict(out, xin=xin, xt=xt), (xin_big, xt_big)

    def rows(self, x1, x2):
        """the source rows of the batch, host (numpy)"""
        return np.concatenate([x1[self.tab], x2[self.tab[self.pr]]]) if self.Np else x1[self.tab]


def _bits_equal(a, b):
    if a is None or b is None:
        return a is b
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return torch.equal(a, b)


def _dense_source(x, off, dev):
    return _buffer(x.shape[0], x.shape[1], off, dev, torch.from_numpy(x).to(dev))[0]


def _sources(x1, x2, which, off, dev):
    """(dense x1, dense x2), (x1, x2 with the named matrices sparse)"""
    from drvae_amd.sparse_rows import CsrRows
    d1, d2 = _dense_source(x1, off, dev), _dense_source(x2, off, dev)
    c1 = CsrRows.from_dense(torch.from_numpy(x1)).to(dev).check() if which in ('x1', 'both') else d1
    c2 = CsrRows.from_dense(torch.from_numpy(x2)).to(dev).check() if which in ('x2', 'both') else d2
    return (d1, d2), (c1, c2)


# --------------------------------------------------------------------------------------- 1. the launch, integer counts
@pytest.mark.parametrize('form', sorted(FORMS))
@pytest.mark.parametrize('X', CF.XS)
def test_sparse_launch_equals_the_dense_launch_bit_for_bit(K, dev, X, form):
    """integer counts: every output of the launch with sparse operands is the dense launch's on the densified matrix, bit for
    bit; guard bands and row padding untouched; two launches give equal bits.  Inside: every row layout x (x1 | x2 | both
    sparse) x both access paths, the batch sizes B in 1 .. 9 with Np in {0, 1, B}, noise on / off and the three positions of
    the batch counter cycling underneath (each size meets each width and form; each layout meets every operand choice and path)"""
    split, transform = form != 'plain', FORMS[form] or None
    sizes, n = itertools.cycle(SIZES), 0
    for lay, which, off in itertools.product(CF.LAYOUTS, WHICH, (0, 1)):
        x1, x2 = CF.layout(lay, X, seed=1), CF.layout(lay, X, seed=2)[::-1].copy()
        dense, sparse = _sources(x1, x2, which, off, dev)
        for _ in range(2):
            B, Np = next(sizes)
            if which == 'x2' and Np == 0:          # (no sparse matrix is read: that IS the dense launch)
                Np = 1
            n += 1
            run = _Launch(K, dev, X, B, Np, off, noisy=n % 2 == 0, ctr=CTRS[n % 3], transform=transform, split=split)
            want, _ = run(*dense)
            got, bufs = run(*sparse)
            again, _ = run(*sparse)
            site = 'X=%d %s %s %s off=%d B=%d Np=%d' % (X, form, lay, which, off, B, Np)
            for k in want:
                assert _bits_equal(got[k], want[k]), '%s: %s differs from the dense launch' % (site, k)
                assert _bits_equal(again[k], got[k]), '%s: %s differs run to run' % (site, k)
            assert _guards_intact(got['xin'], bufs[0]) and (not split or _guards_intact(got['xt'], bufs[1])), site
            rows = torch.from_numpy(run.rows(x1, x2)).to(dev)
            assert _bits_equal(got['xt'] if split else got['xin'], rows) or (not split and run.noise is not None), site
    assert n == 2 * len(CF.LAYOUTS) * len(WHICH) * 2


# --------------------------------------------------------------------------------------- 2. non-integer values
@pytest.mark.parametrize('X', CF.XS)
def test_non_integer_values(K, dev, X):
    """any fp32 values: ``xt`` and the transforms 0 / 1 are the dense launch's bits, and transform 3 too up to 1024 columns (the
    sum runs in the dense launch's order).  Values on a grid of 1/4 (the premise of the bound: a total fp32 sums exactly):
    transform 3 inside the bound of ``tests/depth_ref.py`` at every width"""
    worst = 0.0
    for lay, which, off, noisy in (('full', 'both', 0, True), ('p07', 'x1', 0, False), ('p07', 'both', 1, True), ('gap', 'x2', 0, True)):
        B, Np = (5, 5) if which != 'x1' else (6, 1)
        x1, x2 = CF.layout(lay, X, seed=3, integer=False), CF.layout(lay, X, seed=4, integer=False)[::-1].copy()
        dense, sparse = _sources(x1, x2, which, off, dev)
        for form in ('split-t0', 'split-log1p') + (('split-norm',) if X <= 1024 else ()):
            run = _Launch(K, dev, X, B, Np, off, noisy, 1, FORMS[form] or None, True)
            want, got = run(*dense)[0], run(*sparse)[0]
            assert _bits_equal(got['xt'], want['xt']) and _bits_equal(got['xin'], want['xin']), (lay, which, off, form)
        g1, g2 = CF.layout(lay, X, seed=3, integer=False, grid=4), CF.layout(lay, X, seed=4, integer=False, grid=4)[::-1].copy()
        dense, sparse = _sources(g1, g2, which, off, dev)
        run = _Launch(K, dev, X, B, Np, off, noisy, 1, 'log1p_norm', True)
        got = run(*sparse)[0]
        rows = torch.from_numpy(run.rows(g1, g2))
        assert torch.equal(got['xt'].cpu(), rows)
        want64, bnd = CF.norm_reference(rows, run.noise.cpu() if noisy else None, SIGMA if noisy else 0.0)
        worst = max(worst, ref64.check('sparse dv_batch_feed (log1p_norm) X=%d %s %s' % (X, lay, which), got['xin'].cpu(), want64, bnd))
    print('sparse normalised feed, non-integer values, X=%d: worst |err| / bound %.3g' % (X, worst))


# --------------------------------------------------------------------------------------- 3. other launch-level checks
@pytest.mark.parametrize('X', [978, 2052])
def test_out_of_range_column_is_skipped(K, dev, X):
    """a row holding a column >= X (behind its last entry) and one holding a negative column (in front of its first), built
    without ``check()``: nothing is written for those entries -- every output, guard bands included, is as without them"""
    from drvae_amd.sparse_rows import CsrRows
    x = CF.layout('p07', X, seed=5)
    good = CsrRows.from_dense(torch.from_numpy(x))
    ptr, idx, val = good.ptr.clone(), good.idx.tolist(), good.val.tolist()
    for row, col in ((4, -1), (2, X + 5)):                 # (later rows first: the offsets in front stay valid)
        at = int(ptr[row]) if col < 0 else int(ptr[row + 1])
        idx.insert(at, col)
        val.insert(at, 1000.0)
        ptr[row + 1:] += 1
    bad = CsrRows(ptr, torch.tensor(idx, dtype=torch.int32), torch.tensor(val), (CF.N_SRC, X))
    with pytest.raises(ValueError, match='idx'):
        CsrRows(ptr, torch.tensor(idx, dtype=torch.int32), torch.tensor(val), (CF.N_SRC, X)).check()
    good, bad = good.to(dev), bad.to(dev)
    for form, off in (('plain', 0), ('split-norm', 0), ('split-log1p', 1)):
        run = _Launch(K, dev, X, CF.N_SRC, CF.N_SRC, off, True, 1, FORMS[form] or None, form != 'plain')
        run.table[:] = torch.arange(CF.N_SRC, dtype=torch.int32, device=dev)       # (every row, its neighbours included)
        want, wbufs = run(good, good)
        got, bufs = run(bad, bad)
        assert _bits_equal(got['xin'], want['xin']) and _bits_equal(got['xt'], want['xt']), (form, off)
        assert all(_bits_equal(a, b) for a, b in zip(bufs, wbufs)), 'the whole buffers, guard bands and padding included'


def test_gather_rows_equals_to_dense(K, dev):
    from drvae_amd.sparse_rows import CsrRows
    for X in (3, 978, 2052):
        c = CsrRows.from_dense(torch.from_numpy(CF.layout('p07', X, seed=6))).to(dev)
        idx = _i32([6, 0, 0, 3, 1, 5, 2, 4, 6], dev)
        out, big = _buffer(idx.numel(), X, 0, dev)
        c.gather_rows(out, idx)
        assert torch.equal(out, c.to_dense()[idx.long()]) and _guards_intact(out, big)
        assert torch.equal(c.to_dense().cpu(), torch.from_numpy(CF.layout('p07', X, seed=6)))


# --------------------------------------------------------------------------------------- 4. the step
@pytest.mark.parametrize('dim_x', [20, 1028])
@pytest.mark.parametrize('name', ['drvae-nb', 'pvae-zinb-norm', 'vfae-use_s-gene-batch'])
def test_step_on_a_sparse_dataset_equals_the_dense_one(name, dim_x, dev):
    """tiny models, batch 8, 3 steps, the same epoch table: losses, parameters and both Adam moments of the model fed from a
    ``CsrRows`` dataset are the bits of the model fed from the densified one; eager == captured; ``feed()`` == the epoch feed"""
    kind = CF.STEP_MODELS[name][0]
    ds = CF.counts_dataset(kind, 32, dim_x, 3, dev, n_s=2 if 'use_s' in name else 1)
    sp = CF.to_csr_dataset(ds)
    dense = CF.trajectory(name, ds, 'eager', dev)
    eager = CF.trajectory(name, sp, 'eager', dev, table=dense[2])
    assert CF.same_trajectory(dense, eager), 'sparse against dense'
    assert CF.same_trajectory(eager, CF.trajectory(name, sp, 'captured', dev, table=dense[2])), 'eager against captured'
    assert CF.same_trajectory(eager, CF.trajectory(name, sp, 'feed', dev, table=dense[2])), 'feed() against the epoch feed'
    if kind != 'vfae':          # (one matrix sparse, the other dense)
        assert CF.same_trajectory(dense, CF.trajectory(name, CF.to_csr_dataset(ds, ('x2',)), 'captured', dev, table=dense[2]))


# --------------------------------------------------------------------------------------- 5. fit and evaluation
def _same(a, b):
    if isinstance(a, dict):
        return set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, str):
        return a == b
    a, b = (t.detach().cpu().numpy() if torch.is_tensor(t) else t for t in (a, b))
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


@pytest.mark.parametrize('mode', ['stratified', 'sampler'])
def test_fit_and_evaluation_on_a_sparse_dataset(mode, dev, tmp_path):
    """one epoch of ``fit`` on a ``CsrRows`` dataset in both batcher modes: the parameters are the dense run's bits, the captured
    evaluation is declined, and the evaluation's numbers equal the dense model's step-by-step evaluation"""
    from drvae_amd import data as D
    from drvae_amd import fit as F
    from tests.test_dropout_cpu import tiny_model
    tr, va = CF.counts_dataset('drvae', 32, 20, 1, dev), CF.counts_dataset('drvae', 16, 20, 2, dev)
    models = {}
    for tag, conv in (('dense', lambda d: d), ('csr', CF.to_csr_dataset)):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            model = tiny_model('drvae', device=dev, dim_x=20, type_rec='nb', x_transform='log1p', library_size=True, epochs=1)
        model.w2log = lambda *a: None
        model.fit(D.DeviceBatcher(conv(tr), torch.ones(32), 8, seed=3, mode=mode), types.SimpleNamespace(dataset=conv(va)),
                  add_noise=True, verbose=False, early_stop=False, model_filename=str(tmp_path / (tag + '.pth')))
        assert model.finished_training_iters == 4
        models[tag] = model
    pd, pc = models['dense'].engine().arena.param, models['csr'].engine().arena.param
    assert torch.equal(pd, pc) and bool(torch.isfinite(pc).all())
    sva = CF.to_csr_dataset(va)
    assert F._EvalGraph.get(models['csr'], sva) is None and F._EvalGraph.get(models['csr'], CF.to_csr_dataset(va, ('x2',))) is None
    for m in models.values():             # (the evaluation's loss pass draws its samples: the same Philox position for both)
        m.engine().rng_ctr.fill_(1000)
    got, txt = models['csr'].evaluate_performance_on_dataset(sva)
    want, txt_ref = models['dense']._evaluate(va.x1, va.x2, va.s, va.y, va.has_x2, va.has_y)
    assert txt == txt_ref and _same(got, want) and np.isfinite(float(got['x1_ll']))


def test_gaussian_model_on_sparse_input(dev):
    """a Gaussian model (the plain feed, stratified batches) trains on a ``CsrRows`` dataset to the dense run's bits"""
    ds = CF.counts_dataset('drvae', 32, 20, 3, dev)
    dense = CF.trajectory('drvae-gauss', ds, 'eager', dev)
    assert CF.same_trajectory(dense, CF.trajectory('drvae-gauss', CF.to_csr_dataset(ds), 'captured', dev, table=dense[2]))
