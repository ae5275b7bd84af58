"""CPU: sparse rows in the device batch feed -- ``CsrRows`` (construction from scipy / torch / dense, round trips, ``check()``'s
refusals), the C entry point's refusals without a launch and the descriptor's new tail, the datasets (``__getitem__``, ``.to()``,
``require_counts``), the evaluation (the captured one declines; the step-by-step path on a transient dense copy) and the fused
step on the CPU stand-ins: a model fed from a ``CsrRows`` dataset against the same model fed from the densified one, bit for
bit, through the epoch feed and through ``feed()``.  The kernel itself: ``tests/test_gpu_csr_feed.py``."""
import ctypes as C
import types
import warnings

import numpy as np
import pytest
import torch

from tests import csr_feed_ref as CF
from tests import kernel_ref
from tests.test_dropout_cpu import tiny_model


def _dense(seed=0, n=9, X=11):
    rs = np.random.RandomState(seed)
    x = (rs.poisson(3.0, (n, X)) * (rs.uniform(size=(n, X)) < 0.3)).astype(np.float32)
    x[2] = 0
    x[5] = np.arange(1, X + 1)
    return torch.from_numpy(x)


# ------------------------------------------------------------------------------------------ 1. CsrRows
def test_construction_and_round_trips():
    import scipy.sparse as sp
    from drvae_amd.sparse_rows import CsrRows
    x = _dense()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')          # (torch: sparse CSR support is in beta)
        made = dict(dense=CsrRows.from_dense(x), numpy=CsrRows.from_dense(x.numpy()), scipy=CsrRows.from_scipy(sp.csr_matrix(x.numpy())),
                    coo=CsrRows.from_scipy(sp.coo_matrix(x.numpy())), torch=CsrRows.from_torch(x.to_sparse_csr()))
    for tag, c in made.items():
        assert c.shape == (9, 11) and c.size(0) == 9 and c.size(1) == 11 and len(c) == 9 and c.dim() == 2, tag
        assert c.nnz == int((x != 0).sum()) and c.device.type == 'cpu' and not c.is_cuda
        assert c.ptr.dtype == torch.int64 and c.idx.dtype == torch.int32 and c.val.dtype == torch.float32
        assert c.check() is c and torch.equal(c.to_dense(), x), tag
        assert torch.equal(c.row_sums(), x.sum(1))
        rows = torch.tensor([5, 2, 5, 0, 8])
        assert torch.equal(c.to_dense(rows), x[rows]) and torch.equal(c[rows], x[rows]) and torch.equal(c[3], x[3])
        assert torch.equal(c[-1], x[-1]) and torch.equal(c[2:7:2], x[2:7:2]) and torch.equal(c[x[:, 0] > 0], x[x[:, 0] > 0])
        assert c.to('cpu') is c
        out = torch.full((5, 11), 7.0)
        assert c.gather_rows(out, rows.to(torch.int32)) is out and torch.equal(out, x[rows])
    # unsorted input with duplicates: the scipy constructor sorts and sums on a copy
    m = sp.csr_matrix((np.array([1.0, 2.0, 3.0, 4.0], np.float32), np.array([3, 1, 1, 0]), np.array([0, 3, 4])), shape=(2, 5))
    c = CsrRows.from_scipy(m).check()
    assert c.idx.tolist() == [1, 3, 0] and c.val.tolist() == [5.0, 1.0, 4.0] and m.indices.tolist() == [3, 1, 1, 0]
    empty = CsrRows.from_dense(torch.zeros(4, 6)).check()
    assert empty.nnz == 0 and torch.equal(empty.to_dense(), torch.zeros(4, 6)) and torch.equal(empty.row_sums(), torch.zeros(4))
    with pytest.raises(ValueError, match='N \\+ 1'):
        CsrRows(torch.zeros(3, dtype=torch.int64), torch.zeros(0), torch.zeros(0), (4, 6))


BAD = {     # name: (ptr, idx, val, the rule's words)
    'unsorted row': ([0, 3, 4], [0, 4, 2, 1], [1, 1, 1, 1], 'unsorted row'),
    'duplicate column': ([0, 3, 4], [0, 2, 2, 1], [1, 1, 1, 1], 'duplicate column'),
    'column == X': ([0, 3, 4], [0, 2, 5, 1], [1, 1, 1, 1], 'idx < X'),
    'negative column': ([0, 3, 4], [-1, 2, 4, 1], [1, 1, 1, 1], 'negative column'),
    'decreasing ptr': ([0, 3, 2, 4], [0, 2, 4, 1], [1, 1, 1, 1], 'non-decreasing'),
    'wrong ptr[N]': ([0, 3, 3], [0, 2, 4, 1], [1, 1, 1, 1], 'ptr\\[N\\] == nnz'),
    'NaN value': ([0, 3, 4], [0, 2, 4, 1], [1, float('nan'), 1, 1], 'finite'),
    'ptr[0] != 0': ([1, 3, 4], [0, 2, 4, 1], [1, 1, 1, 1], 'ptr\\[0\\] == 0'),
}


@pytest.mark.parametrize('name', sorted(BAD))
def test_check_refuses_each_malformed_structure_with_its_own_message(name):
    from drvae_amd.sparse_rows import CsrRows
    ptr, idx, val, words = BAD[name]
    c = CsrRows(torch.tensor(ptr), torch.tensor(idx), torch.tensor(val, dtype=torch.float32), (len(ptr) - 1, 5))
    with pytest.raises(ValueError, match=words) as e:
        c.check()
    others = [w.replace('\\', '') for k, (_, _, _, w) in BAD.items() if k != name]
    assert not any(w in str(e.value) for w in others), str(e.value)       # (its own message, nobody else's)
    with pytest.raises(ValueError):           # (a refusal is not remembered as a pass)
        c.check()
    good = CsrRows(torch.tensor([0, 3, 4]), torch.tensor([0, 2, 4, 1]), torch.ones(4), (2, 5))
    assert good.check() is good and good._checked
    # the row boundary: a column may drop from one row to the next
    assert CsrRows(torch.tensor([0, 2, 4]), torch.tensor([3, 4, 0, 3]), torch.ones(4), (2, 5)).check()._checked


# ------------------------------------------------------------------------------------------ 2. the C surface
def test_descriptor_ends_in_the_six_new_fields():
    from drvae_amd import _lib
    names = [f[0] for f in _lib.BatchFeed._fields_]
    assert names[-6:] == ['csr1_ptr', 'csr1_idx', 'csr1_val', 'csr2_ptr', 'csr2_idx', 'csr2_val']
    assert names[-9:-6] == ['xt', 'ldt', 'transform'] and all(f[1] is C.c_void_p for f in _lib.BatchFeed._fields_[-6:])
    assert _lib.ABI_VERSION == 13


def test_entry_point_refusals_without_a_launch():
    """``B == 0``, or a refusal in front of the launch: no address is ever dereferenced"""
    from drvae_amd import _lib
    lib = _lib.load()
    call = lambda **kw: lib.dv_batch_feed(C.byref(_lib.BatchFeed(L=1, n_batches=1, X=8, **kw)), None, None, None)
    A = 4096                                                            # (an address that is only looked at)
    full1, full2 = dict(csr1_ptr=A, csr1_idx=A, csr1_val=A), dict(csr2_ptr=A, csr2_idx=A, csr2_val=A)
    # the new fields zero: what it returned
    assert call(B=0) == 0 and call(B=0, Np=3) == 0 and call(B=4) == -1 and call(B=0, x1=A, x2=A) == 0
    # whole triples at B == 0: nothing to do
    assert call(B=0, **full1) == 0 and call(B=0, **full2) == 0 and call(B=0, **full1, **full2) == 0 and call(B=0, x1=A, **full2) == 0
    # an incomplete triple, at B == 0 too
    for m in (full1, full2):
        for drop in m:
            part = {k: v for k, v in m.items() if k != drop}
            assert call(B=0, **part) == -1 and call(B=4, **part) == -1, drop
        for only in m:
            assert call(B=0, **{only: A}) == -1
    # a dense pointer AND a triple
    assert call(B=0, x1=A, **full1) == -1 and call(B=0, x2=A, **full2) == -1 and call(B=0, x1=A, x2=A, **full1, **full2) == -1
    # a matrix that is read has neither (every other operand given: these are refused for that alone)
    rest = dict(B=4, table=A, ctr=A, base=A, xin=A)
    assert call(**rest) == -1 and call(x1=A, Np=2, pair_rows=A, **rest) == -1 and call(Np=2, pair_rows=A, **full2, **rest) == -1
    assert call(Np=2, pair_rows=A, **full1, **rest) == -1
    # ... and the checks behind it still hold with a sparse matrix (refused before the launch)
    assert call(B=4, **full1) == -1                                      # no table / counters / output
    assert call(transform=2, xt=A, **full1, **rest) == -1 and call(transform=1, **full1, **rest) == -1


# ------------------------------------------------------------------------------------------ 3. the datasets
def test_datasets_take_sparse_rows():
    from drvae_amd import data as D
    from drvae_amd.sparse_rows import CsrRows
    ds = CF.counts_dataset('drvae', 12, 9, 1)
    for which in (('x1', 'x2'), ('x1',), ('x2',)):
        sp = CF.to_csr_dataset(ds, which)
        assert len(sp) == 12 and all(isinstance(getattr(sp, k), CsrRows) == (k in which) for k in ('x1', 'x2'))
        for i in (0, 1, 11):
            assert all(torch.equal(a, b) for a, b in zip(sp[i], ds[i]))
        got = torch.utils.data.DataLoader(sp, batch_size=5)
        for a, b in zip(got, torch.utils.data.DataLoader(ds, batch_size=5)):
            assert all(torch.equal(u, v) for u, v in zip(a, b))
        moved = sp.to('cpu')
        assert isinstance(moved, D.DrVAEDataset) and all(isinstance(getattr(moved, k), CsrRows) == (k in which) for k in ('x1', 'x2'))
        assert torch.equal(torch.as_tensor(moved.x1[torch.arange(12)]), ds.x1)
        D.require_counts(sp, 'test')
        assert sp._counts_checked
    v = CF.to_csr_dataset(CF.counts_dataset('vfae', 12, 9, 1))
    assert isinstance(v.to('cpu').x1, CsrRows) and torch.equal(v[3][0], CF.counts_dataset('vfae', 12, 9, 1).x1[3])
    with pytest.raises(AssertionError):            # shapes are checked as for dense matrices
        D.DrVAEDataset(CsrRows.from_dense(torch.zeros(12, 9)), CsrRows.from_dense(torch.zeros(12, 8)), ds.s, ds.y, ds.has_x2, ds.has_y)
    # require_counts reduces over the stored values
    neg = ds.x1.clone()
    neg[4, 2] = -1.0
    bad = D.DrVAEDataset(CsrRows.from_dense(neg), CsrRows.from_dense(ds.x2), ds.s, ds.y, ds.has_x2, ds.has_y)
    with pytest.raises(ValueError, match='x >= 0'):
        D.require_counts(bad, 'test')
    D.require_counts(D.VFAEDataset(CsrRows.from_dense(torch.zeros(4, 9)), ds.s[:4], ds.y[:4], ds.has_y[:4]), 'test')


def test_bind_checks_the_structure_once_and_the_feed_rows_pass_through(monkeypatch):
    from drvae_amd import data as D
    from drvae_amd.sparse_rows import CsrRows
    CF.install(monkeypatch)
    ds = CF.to_csr_dataset(CF.counts_dataset('drvae', 32, 13, 3))
    model = tiny_model('drvae', type_rec='nb', x_transform='log1p')
    bat = D.DeviceBatcher(ds, torch.ones(32), 8, seed=5, mode='sampler')
    assert not ds.x1._checked and not ds.x2._checked
    bat.bind(model.engine())
    assert ds.x1._checked and ds.x2._checked
    bat.begin_epoch()
    fd = model.engine().plan.live_feed
    assert fd.x1 is ds.x1 and fd.x2 is ds.x2, 'no copy: the feed reads the arrays themselves'
    bat.begin_epoch()
    assert model.engine().plan.live_feed.x1 is ds.x1
    bad = CsrRows(torch.tensor([0, 2] + [2] * 31), torch.tensor([4, 1]), torch.ones(2), (32, 13))
    ds2 = D.DrVAEDataset(bad, ds.x2, ds.s, ds.y, ds.has_x2, ds.has_y)
    with pytest.raises(ValueError, match='unsorted row'):
        D.DeviceBatcher(ds2, torch.ones(32), 8, seed=5, mode='sampler').bind(tiny_model('drvae', type_rec='nb').engine())


# ------------------------------------------------------------------------------------------ 4. evaluation
def test_captured_evaluation_declines_and_the_step_by_step_path_densifies(monkeypatch):
    from drvae_amd import fit as F
    CF.install(monkeypatch)
    ds = CF.counts_dataset('drvae', 16, 13, 2)
    for which in (('x1', 'x2'), ('x1',), ('x2',)):
        # (declined on the operands' type alone: the model is not even looked at)
        assert F._EvalGraph.get(None, CF.to_csr_dataset(ds, which)) is None
    model = tiny_model('drvae', type_rec='nb', x_transform='log1p', library_size=True)
    model.engine().rng_ctr.fill_(1000)    # (the evaluation's loss pass draws its samples: the same Philox position every time)
    want, txt_ref = model.evaluate_performance_on_dataset(ds)
    for which in (('x1', 'x2'), ('x2',)):
        model.engine().rng_ctr.fill_(1000)
        got, txt = model.evaluate_performance_on_dataset(CF.to_csr_dataset(ds, which))
        assert txt == txt_ref and set(got) == set(want)
        for k in want:
            if isinstance(want[k], dict):
                assert got[k] == want[k], k
            else:
                np.testing.assert_array_equal(np.asarray(got[k]), np.asarray(want[k]), err_msg=k)


# ------------------------------------------------------------------------------------------ 5. the step on the stand-ins
@pytest.mark.parametrize('name', ['drvae-nb', 'vfae-use_s-gene-batch', 'drvae-gauss'])
def test_step_on_a_sparse_dataset_equals_the_dense_one(name, monkeypatch):
    """the epoch feed and ``feed()`` of a ``CsrRows`` dataset against the epoch feed of the densified one: losses, parameters and
    both Adam moments bit for bit over three steps"""
    CF.install(monkeypatch)
    kind = CF.STEP_MODELS[name][0]
    ds = CF.counts_dataset(kind, 32, 13, 3, n_s=2 if 'use_s' in name else 1)
    sp = CF.to_csr_dataset(ds)
    dense = CF.trajectory(name, ds, 'eager')
    assert kernel_ref.CALLS['csr_feed'] == 0 and kernel_ref.CALLS['batch_feed'] >= 3
    epoch = CF.trajectory(name, sp, 'eager', table=dense[2])
    assert kernel_ref.CALLS['csr_feed'] == 3
    assert CF.same_trajectory(dense, epoch), 'the epoch feed, sparse against dense'
    if name != 'drvae-gauss':       # (stratified batches: ``feed()`` draws its own rows group by group)
        assert CF.same_trajectory(epoch, CF.trajectory(name, sp, 'feed', table=dense[2])), 'feed() against the epoch feed'
    if kind != 'vfae':
        assert CF.same_trajectory(dense, CF.trajectory(name, CF.to_csr_dataset(ds, ('x2',)), 'eager', table=dense[2]))


def test_fit_through_host_loaders_on_a_sparse_dataset(monkeypatch, tmp_path):
    """host loaders keep working (the slow path): ``__getitem__`` hands them dense rows"""
    from tests.test_fit import _loader
    CF.install(monkeypatch)
    tr, va = CF.counts_dataset('drvae', 24, 13, 1), CF.counts_dataset('drvae', 16, 13, 2)
    out = []
    for conv in (lambda d: d, CF.to_csr_dataset):
        torch.manual_seed(0)
        model = tiny_model('drvae', type_rec='nb', x_transform='log1p', library_size=True, epochs=1)
        model.w2log = lambda *a: None
        model.fit(_loader(conv(tr), 8), types.SimpleNamespace(dataset=conv(va)), add_noise=False, verbose=False, early_stop=False,
                  model_filename=str(tmp_path / 'm.pth'))
        out.append(model.engine().arena.param.clone())
    assert model.finished_training_iters == 3 and torch.equal(out[0], out[1])
