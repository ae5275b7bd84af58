"""Row-chunked whole-set evaluation (``model.eval_chunk_rows`` / ``evaluate_performance_on_dataset(chunk_rows=...)``), the parts
that need no GPU: the chunk partition and the column-moment fold as pure functions, the re-targetable GLOBAL row column of
the plan's draw descriptors, every refusal, and that ``None`` stays on the existing route."""
import itertools
import types
import warnings

import numpy as np
import pytest
import torch

from tests import kernel_ref
from tests.test_dropout_cpu import tiny_model


def _quiet(kind, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return tiny_model(kind, **kw)


# --------------------------------------------------------------------------------------- the partition
def _flags(n, seed):
    rs = np.random.RandomState(seed)
    return rs.randint(0, 2, n), rs.randint(0, 2, n)


PARTITION_CASES = {
    'mixed': _flags(37, 1),
    'one row': (np.array([1]), np.array([0])),
    'an empty group': (np.array([1, 1, 0, 1, 0]), np.array([1, 1, 1, 1, 1])),
    'a group of one row': (np.array([1, 0, 0, 0, 0, 0, 0]), np.array([0, 1, 1, 0, 1, 1, 0])),
    'one group only': (np.zeros(9, np.int64), np.zeros(9, np.int64)),
}


@pytest.mark.parametrize('kind', ['drvae', 'pvae', 'vfae'])
@pytest.mark.parametrize('case', sorted(PARTITION_CASES))
def test_partition_covers_every_row_once_in_homogeneous_chunks(case, kind):
    from drvae_amd.fit import chunk_partition
    hx, hy = PARTITION_CASES[case]
    n = len(hx)
    ex = hx.astype(bool) & (kind != 'vfae')           # (what the model kind reads of the flags)
    ey = hy.astype(bool) & (kind != 'pvae')
    for C in sorted({1, 2, 5, n - 1, n, n + 1, 64} - {0}):
        chunks = chunk_partition(None if kind == 'vfae' else hx, None if kind == 'pvae' else hy, C, kind)
        rows = np.concatenate([r for _, r in chunks])
        assert sorted(rows.tolist()) == list(range(n)), 'every row exactly once'
        for (gx, gy), r in chunks:
            assert 1 <= len(r) <= C
            assert (ex[r] == gx).all() and (ey[r] == gy).all(), 'homogeneous in its group'
            assert (np.diff(r) > 0).all(), 'data-set order inside a chunk'
        groups = [g for g, _ in chunks]
        assert [k for k, _ in itertools.groupby(groups)] == sorted(set(groups), key=groups.index), 'a group is contiguous'
        # at most one full-size and one tail shape per group: the captures are bounded whatever N is
        shapes = {(g, len(r)) for g, r in chunks}
        assert all(sum(1 for s in shapes if s[0] == g) <= 2 for g in set(groups)) and len(shapes) <= 8
        for g in set(groups):
            sizes = [len(r) for gg, r in chunks if gg == g]
            assert all(s == C for s in sizes[:-1]), 'only the last chunk of a group is short'
        if C >= n:
            assert len(chunks) == len(set(groups)), 'C >= N: one chunk per group that has rows'
    # the flags given as they are stored (the unread one included) partition the same way
    a = chunk_partition(hx, hy, 3, kind)
    b = chunk_partition(None if kind == 'vfae' else hx, None if kind == 'pvae' else hy, 3, kind)
    assert [(g, r.tolist()) for g, r in a] == [(g, r.tolist()) for g, r in b]


def test_partition_is_stable_and_refuses_bad_input():
    from drvae_amd.fit import chunk_partition
    hx, hy = np.array([0, 1, 1, 0, 1, 0]), np.array([1, 1, 0, 0, 1, 1])
    got = [(g, r.tolist()) for g, r in chunk_partition(hx, hy, 2, 'drvae')]
    assert got == [((True, True), [1, 4]), ((True, False), [2]), ((False, True), [0, 5]), ((False, False), [3])]
    assert [(g, r.tolist()) for g, r in chunk_partition(torch.from_numpy(hx), torch.from_numpy(hy).reshape(-1, 1), 2, 'drvae')] == got
    for bad in (0, -3, 2.0, '4', None, True):
        with pytest.raises(ValueError):
            chunk_partition(hx, hy, bad, 'drvae')
    with pytest.raises(ValueError):
        chunk_partition(hx, hy[:-1], 2, 'drvae')


# --------------------------------------------------------------------------------------- the column-sum fold
def test_column_moment_fold_against_numpy_float64():
    from drvae_amd.fit import fold_col_blocks
    rs = np.random.RandomState(3)
    X = 11
    acc = torch.zeros(1, 3, X, dtype=torch.float64)
    want = np.zeros((1, 3, X))
    for blocks in (1, 4, 2, 16):           # chunks of different shapes leave different numbers of blocks
        part = rs.gamma(2.0, 1e3, (blocks, 3, X)) * rs.choice([1e-6, 1.0, 1e6], (blocks, 3, X))
        out = fold_col_blocks(acc, torch.from_numpy(part))
        assert out is acc
        s = np.zeros((3, X))
        for b in range(blocks):            # (block order, then added to the running sum: the one fixed order)
            s = s + part[b]
        want = want + s[None]
        np.testing.assert_allclose(acc.numpy(), want, rtol=4 * np.finfo(np.float64).eps, atol=0)
    with pytest.raises(AssertionError):
        fold_col_blocks(torch.zeros(1, 3, X), torch.zeros(2, 3, X, dtype=torch.float64))


# --------------------------------------------------------------------------------------- the plan's row column
def test_global_row_column_is_retargetable_as_device_data(monkeypatch):
    """``_Plan.retarget_rows``: column 3 of every draw descriptor becomes the given row of its input row, again and again (no
    compounding), the other columns stay -- and equals the column of a plan BUILT at that ``row0`` for a contiguous range"""
    kernel_ref.install(monkeypatch)
    model = _quiet('drvae', dim_x=6)
    eng = model.engine()
    hx, hy = np.array([1, 0, 1, 0, 0]), np.array([1, 1, 0, 0, 1])
    p, _ = eng.set_structure(hx, hy, counts=(40, 9, 21))
    before, trailer = p.noise_desc.clone(), p.noise_table[-1].clone()
    local = before[:, 3].clone()
    assert set(local.tolist()) == set(range(5))
    for grow in ([31, 4, 17, 0, 22], [7, 8, 9, 10, 11]):
        p.retarget_rows(torch.tensor(grow, dtype=torch.int32))
        assert torch.equal(p.noise_desc[:, :3], before[:, :3])
        assert p.noise_desc[:, 3].tolist() == [grow[j] for j in local.tolist()]
    assert torch.equal(p.noise_table[-1], trailer), 'the trailer row is untouched'
    eng.row0 = 7
    q, _ = eng.set_structure(hx, hy, counts=(40, 9, 21))
    assert q is not p and torch.equal(q.noise_desc, p.noise_desc)


# --------------------------------------------------------------------------------------- refusals
def _host_dataset(kind, n=12, X=13):
    from drvae_amd import data as D
    rs = np.random.RandomState(0)
    t = torch.from_numpy
    x1, x2 = t(rs.randn(n, X).astype(np.float32)), t(rs.randn(n, X).astype(np.float32))
    s, y = t(np.zeros(n, np.int64)), t(rs.randint(0, 2, n))
    hx, hy = t((np.arange(n) % 3 == 0).astype(np.int64)), t((np.arange(n) % 4 != 1).astype(np.int64))
    if kind == 'vfae':
        return D.VFAEDataset(x1, s, y, hy)
    return D.DrVAEDataset(x1, x2, s, y, hx, hy)


@pytest.mark.parametrize('kind', ['drvae', 'pvae', 'vfae'])
def test_attribute_and_constructor_keyword(kind):
    assert _quiet(kind).eval_chunk_rows is None
    assert _quiet(kind, eval_chunk_rows=8).eval_chunk_rows == 8
    for bad in (0, -1, 2.5, '8', True):
        with pytest.raises(ValueError, match='eval_chunk_rows'):
            _quiet(kind, eval_chunk_rows=bad)


def test_use_mmd_is_refused_at_construction_and_at_the_call():
    with pytest.raises(NotImplementedError, match='use_MMD'):
        _quiet('vfae', dim_s=2, use_s=True, use_MMD=True, eval_chunk_rows=4)
    model = _quiet('vfae', dim_s=2, use_s=True, use_MMD=True)              # (allowed: the chunk size is not set)
    with pytest.raises(NotImplementedError, match='use_MMD'):
        model.evaluate_performance_on_dataset(_host_dataset('vfae'), chunk_rows=4)
    model.eval_chunk_rows = 4                                              # (the plain attribute, set late: refused at the call)
    with pytest.raises(NotImplementedError, match='use_MMD'):
        model.evaluate_performance_on_dataset(_host_dataset('vfae'))
    # ``use_MMD`` without ``use_s`` has no penalty (the models' default): nothing to refuse
    assert _quiet('vfae', use_MMD=True, eval_chunk_rows=4).eval_chunk_rows == 4


@pytest.mark.parametrize('kind', ['drvae', 'pvae', 'vfae'])
def test_refusals_at_the_call(kind):
    model, ds = _quiet(kind), _host_dataset(kind)
    spy = []
    model._evaluate = lambda *a, **k: spy.append(a) or ('perf', 'text')
    for bad in (0, -2, 1.5, 'all', False):
        with pytest.raises(ValueError, match='chunk'):
            model.evaluate_performance_on_dataset(ds, chunk_rows=bad)
    with pytest.raises(ValueError, match='return_full_data'):
        model.evaluate_performance_on_dataset(ds, return_full_data=True, chunk_rows=4)
    with pytest.raises(ValueError, match='host-resident'):          # a host-resident set: no silent other path
        model.evaluate_performance_on_dataset(ds, chunk_rows=4)
    model.eval_chunk_rows = 4
    with pytest.raises(ValueError, match='host-resident'):
        model.evaluate_performance_on_dataset(ds)
    with pytest.raises(ValueError, match='return_full_data'):
        model.evaluate_performance_on_dataset(ds, return_full_data=True)
    model._dp = (0, 2)                                               # data parallelism: every rank raises alike
    with pytest.raises(NotImplementedError, match='data parallelism'):
        model.evaluate_performance_on_dataset(ds)
    model._dp = None
    assert spy == [], 'a refused chunked evaluation never falls back to the densifying path'
    assert '_eval_chunked' not in model.__dict__ or model.__dict__['_eval_chunked'] == {}


@pytest.mark.parametrize('kind', ['drvae', 'pvae', 'vfae'])
def test_none_stays_on_the_existing_route(kind):
    """``eval_chunk_rows=None`` (the default) and ``chunk_rows=None``: ``_EvalGraph.get`` is asked, then ``_evaluate`` gets the
    set's tensors as before; the argument wins over the attribute in both directions"""
    from drvae_amd import fit as F
    model, ds = _quiet(kind), _host_dataset(kind)
    calls = []

    def spy(x1, x2, s, y, has_x2, has_y, return_full_data=False):
        calls.append((x1, x2, s, y, has_x2, has_y, return_full_data))
        return 'perf', 'text'
    model._evaluate = spy
    asked = []
    keep = F._EvalGraph.get
    F._EvalGraph.get = staticmethod(lambda m, d: asked.append((m, d)) or keep(m, d))
    try:
        assert model.evaluate_performance_on_dataset(ds) == ('perf', 'text')
        assert model.evaluate_performance_on_dataset(ds, chunk_rows=None) == ('perf', 'text')
        assert model.evaluate_performance_on_dataset(ds, return_full_data=True) == ('perf', 'text')
    finally:
        F._EvalGraph.get = keep
    assert len(calls) == 3 and len(asked) == 2 and all(a == (model, ds) for a in asked)
    g = lambda k: getattr(ds, k, None)
    for c, full in zip(calls, (False, False, True)):
        assert all(a is b for a, b in zip(c[:6], (g('x1'), g('x2'), g('s'), g('y'), g('has_x2'), g('has_y')))) and c[6] is full
    assert '_eval_chunked' not in model.__dict__


def test_the_chunked_cache_is_dropped_with_the_captured_evaluations():
    model = _quiet('drvae')
    model.__dict__['_eval_chunked'] = {'stale': object()}
    model.load_state_dict(model.state_dict())
    assert '_eval_chunked' not in model.__dict__
    model.__dict__['_eval_chunked'] = {'stale': object()}
    model._create_optimizer()
    assert '_eval_chunked' not in model.__dict__
