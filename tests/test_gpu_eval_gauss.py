"""GPU: the Gaussian evaluation launches -- ``dv_recon_row_stats``, ``dv_recon_rows`` (finished and raw heads, ``ll`` given and
None), ``dv_col_moments``, ``dv_recon_finalize`` -- each against the float64 reference and bounds of ``tests/eval_gauss_ref.py``
(never against another launch), through the strided and misaligned views the evaluation feeds them, with every output
between guard bands of a sentinel-filled buffer (``_flat`` of ``tests/test_gpu_gene_disp.py``: the launchers want contiguous
outputs, so the bands sit before and behind) and every input bit-unchanged afterwards.  Run with -s for the worst observed
fraction of each bound and the route every ``dv_recon_rows`` layout took."""
import functools

import numpy as np
import pytest
import torch

from tests import eval_gauss_ref as G
from tests import ref64
from tests.test_eval_gauss_cpu import (COL_MS, COL_XS, FIN_BLOCKS, FIN_NS, FIN_XS, MS, PROFILE_XS, XS, XS_STATS_ONLY, _sel_variants,
                                       profile_finalize_case)
from tests.test_gpu_gene_disp import GUARD, SENTINEL, _flat, _flat_intact, host

pytestmark = pytest.mark.gpu

LAYOUTS = ('contig', 'heads0', 'heads3', 'x_odd', 'bias_odd')
f = np.float32


@pytest.fixture(scope='module')
def K(dev):
    import drvae_amd.kernels as K
    from drvae_amd import _lib
    _lib.load()
    return K


def _flat64(n, dev):
    big = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float64, device=dev)
    return big[GUARD:GUARD + n], big


def _note(seen, site, worst):
    """``seen``: the test's own record site -> worst |got - ref| / bound"""
    seen[site] = max(seen.get(site, 0.0), float(worst))


def _report(seen):
    for k in sorted(seen):
        print('worst |got - ref| / bound  %-44s %.3g' % (k, seen[k]))


@functools.lru_cache(maxsize=None)
def _case(name, M, X):
    return G.profile(name, M, X)


@functools.lru_cache(maxsize=None)
def _refs(name, M, X, raw):
    """(r fp32, rows ref, rows bound, ll ref, ll bound): computed once per case, shared by every layout"""
    c = _case(name, M, X)
    r, sd, pre = G.finished(c, raw)
    return (r,) + G.rows_reference(c['x'], r) + G.ll_reference(c['x'], r, sd=sd, pre=pre)


def _aligned8(t):
    return t.data_ptr() % 8 == 0


def route_v2(K, x, mu, sd, bias):
    """the header's words: rows of even width are read with 8-B loads -- X, both row strides even and every pointer (x, mu, sd and,
    with raw heads, both biases) 8-byte aligned; the dword path otherwise (odd X or unaligned rows)"""
    X = x.shape[1]
    ok = X % 2 == 0 and K._ld(x) % 2 == 0 and K._ld(mu) % 2 == 0 and _aligned8(x) and _aligned8(mu) and _aligned8(sd)
    if bias is not None:
        ok = ok and _aligned8(bias[0]) and _aligned8(bias[1])
    return ok


def lay_out(layout, c, raw, dev):
    """device tensors (x, mu, sd, bias | None, backing buffers) of a case in one layout: contiguous; mu / sd as the halves of one
    (M, 2X + pad) heads buffer, pad 0 / 3 (an odd row stride); x as a column range from column 1 of a wider buffer of EVEN row
    stride (only the pointer, 4-byte aligned, forces the dword path); the biases as views one float into their buffers"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    M, X = c['x'].shape
    mu_h, sd_h = (c['mu_raw'], c['sd_raw']) if raw else (c['r'], c['sd'])
    backing = []
    x = t(c['x'])
    if layout in ('heads0', 'heads3'):
        pad = 3 if layout == 'heads3' else 0
        heads = torch.full((M, 2 * X + pad), SENTINEL, device=dev)
        heads[:, :X], heads[:, X:2 * X] = t(mu_h), t(sd_h)
        mu, sd = heads[:, :X], heads[:, X:2 * X]
        backing.append(heads)
    else:
        mu, sd = t(mu_h), t(sd_h)
    if layout == 'x_odd':
        wide = torch.full((M, X + 2 + X % 2), SENTINEL, device=dev)
        wide[:, 1:1 + X] = x
        x = wide[:, 1:1 + X]
        assert x.data_ptr() % 8 == 4 and wide.shape[1] % 2 == 0
        backing.append(wide)
    bias = None
    if raw:
        if layout == 'bias_odd':
            bb = torch.full((2, X + 3), SENTINEL, device=dev)
            bb[0, 1:1 + X], bb[1, 1:1 + X] = t(c['bm']), t(c['bs'])
            bias = (bb[0, 1:1 + X], bb[1, 1:1 + X])
            assert bias[0].data_ptr() % 8 == 4
            backing.append(bb)
        else:
            bias = (t(c['bm']), t(c['bs']))
    backing += [x, mu, sd] + (list(bias) if bias else [])
    return x, mu, sd, bias, backing


def run_rows_case(K, dev, name, M, X, layout, raw, seen, routes=None):
    """``dv_recon_rows`` with and without ``ll`` and ``dv_recon_row_stats`` on one case and layout, each against float64"""
    c = _case(name, M, X)
    r32, rows_ref, rows_b, ll_ref, ll_b = _refs(name, M, X, raw)
    x, mu, sd, bias, backing = lay_out(layout, c, raw, dev)
    before = [b.clone() for b in backing]
    v2 = route_v2(K, x, mu, sd, bias)
    if routes is not None:
        routes.add((raw, v2))
    tag = '%s %s' % ('raw' if raw else 'finished', 'pair' if v2 else 'dword')
    rows, rows_big = _flat(M * 6, dev)
    ll, ll_big = _flat(M, dev)
    K.recon_rows(rows.view(M, 6), ll, x, mu, sd, bias=bias, sd_shift=G.SHIFT)
    got_rows, got_ll = host(rows).view(M, 6).clone(), host(ll).clone()
    where = dict(case=(name, M, X, layout, tag))
    try:
        ref64.check('dv_recon_rows rows', got_rows, rows_ref, rows_b)
        ex = ref64.excess(got_rows, rows_ref, rows_b).max(0)[0]
        for k, nm in enumerate(('sse', 'mx', 'mr', 'cxx', 'crr', 'cxr')):
            _note(seen, 'dv_recon_rows (%s) %s' % (tag, nm), ex[k])
        _note(seen, 'dv_recon_rows (%s) ll' % tag, ref64.check('dv_recon_rows ll', got_ll, ll_ref, ll_b))
    except AssertionError as e:
        raise AssertionError('%s: %s' % (where, e))
    assert _flat_intact(rows_big, M * 6) and _flat_intact(ll_big, M), where
    # no log-likelihood rows wanted: the same statistics, nothing else written
    rows2, rows2_big = _flat(M * 6, dev)
    K.recon_rows(rows2.view(M, 6), None, x, mu, sd, bias=bias, sd_shift=G.SHIFT)
    assert torch.equal(host(rows2).view(M, 6), got_rows) and _flat_intact(rows2_big, M * 6), where
    # dv_recon_row_stats on the finished mean (fl32(mu + bias_mu): the exact rounded sum, formed on the host), same layout of x
    rfin = torch.from_numpy(r32).to(dev) if raw else mu
    rows3, rows3_big = _flat(M * 6, dev)
    K.recon_row_stats(rows3.view(M, 6), x, rfin)
    got3 = host(rows3).view(M, 6)
    ex = ref64.excess(got3, rows_ref, rows_b)
    assert float(ex.max()) <= 1.0, ('dv_recon_row_stats', where, float(ex.max()))
    for k, nm in enumerate(('sse', 'mx', 'mr', 'cxx', 'crr', 'cxr')):
        _note(seen, 'dv_recon_row_stats %s' % nm, ex[:, k].max())
    assert _flat_intact(rows3_big, M * 6)
    if not v2:          # the dword path: dv_recon_row_stats' summation order, bit for bit
        assert torch.equal(got3, got_rows), where
    for b, b0 in zip(backing, before):
        assert torch.equal(b, b0), where
    return v2


# ------------------------------------------------------------------------------------------- the row launches
@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('X', XS)
def test_row_launches_against_float64(K, dev, X, layout):
    seen = {}
    for M in MS:
        for raw in (False, True):
            v2 = run_rows_case(K, dev, 'normal', M, X, layout, raw, seen)
            want = X % 2 == 0 and layout not in ('heads3', 'x_odd') and not (raw and layout == 'bias_odd')
            assert v2 == want, (X, layout, raw)
    _report(seen)


def test_routes_cover_the_four_instantiations(K, dev):
    """RAW x V2 of ``recon_rows_kernel``: which route the entry point's rule selects for every layout of the grid"""
    routes, table = set(), {}
    for X in (13, 978):
        for layout in LAYOUTS:
            for raw in (False, True):
                table[(X, layout, raw)] = run_rows_case(K, dev, 'normal', 3, X, layout, raw, {}, routes)
    for (X, layout, raw), v2 in sorted(table.items()):
        print('dv_recon_rows X = %4d %-8s %-8s -> %s' % (X, layout, 'raw' if raw else 'finished', 'pair (8-B loads)' if v2 else 'dword'))
    assert routes == {(False, False), (False, True), (True, False), (True, True)}


def test_a_workgroup_takes_a_second_trip(K, dev):
    """the grid is capped at 8192 workgroups of 4 rows: M = 32773 is the smallest M with a second trip"""
    seen = {}
    for layout, raw in (('contig', False), ('heads0', True)):
        run_rows_case(K, dev, 'normal', 32773, 13, layout, raw, seen)
    _report(seen)


@pytest.mark.parametrize('X', XS_STATS_ONLY)
def test_row_stats_beyond_the_register_width(K, dev, X):
    """``recon_row_stats_kernel`` alone, as ``fit.py`` runs it for X > 1024: a lane adds up to 65 terms"""
    seen = {}
    for name in ('normal', 'offset', 'expression'):
        c = _case(name, 5, X)
        ref, bnd = G.rows_reference(c['x'], c['r'])
        for strided in (False, True):
            x, r = torch.from_numpy(c['x']).to(dev), torch.from_numpy(c['r']).to(dev)
            if strided:
                wide = torch.full((5, 2 * X + 3), SENTINEL, device=dev)
                wide[:, 1:1 + X], wide[:, 1 + X:1 + 2 * X] = x, r
                x, r = wide[:, 1:1 + X], wide[:, 1 + X:1 + 2 * X]
                w0 = wide.clone()
            rows, big = _flat(30, dev)
            K.recon_row_stats(rows.view(5, 6), x, r)
            _note(seen, 'dv_recon_row_stats X = %d' % X, ref64.check('dv_recon_row_stats %s X=%d' % (name, X), host(rows).view(5, 6), ref, bnd))
            assert _flat_intact(big, 30) and (not strided or torch.equal(wide, w0))
    _report(seen)


def test_recon_rows_is_refused_beyond_the_register_width(K, dev):
    c = _case('normal', 4, 1025)
    rows, big = _flat(24, dev)
    ll, ll_big = _flat(4, dev)
    t = lambda a: torch.from_numpy(a).to(dev)
    with pytest.raises(RuntimeError):
        K.recon_rows(rows.view(4, 6), ll, t(c['x']), t(c['r']), t(c['sd']))
    with pytest.raises(RuntimeError):
        K.recon_rows(rows.view(4, 6), ll, t(c['x']), t(c['mu_raw']), t(c['sd_raw']), bias=(t(c['bm']), t(c['bs'])))
    assert bool((host(big) == SENTINEL).all()) and bool((host(ll_big) == SENTINEL).all())      # nothing written


@pytest.mark.parametrize('X', PROFILE_XS)
@pytest.mark.parametrize('name', G.PROFILES)
def test_row_launches_on_every_profile(K, dev, name, X):
    seen = {}
    for layout in ('contig', 'heads0', 'heads3'):
        for raw in (False, True):
            run_rows_case(K, dev, name, 5, X, layout, raw, seen)
    if name == 'zero_rows':         # exact zeros out of exact zeros (the finished heads: row 0 of x, row 1 of r)
        c = _case(name, 5, X)
        rows = torch.full((5, 6), SENTINEL, device=dev)
        K.recon_rows(rows, None, *(torch.from_numpy(c[k]).to(dev) for k in ('x', 'r', 'sd')))
        got = host(rows)
        assert (got[0, [1, 3, 5]] == 0).all() and (got[1, [2, 4, 5]] == 0).all()
    _report(seen)


# ------------------------------------------------------------------------------------------- dv_col_moments
def _col_run(K, dev, x, r, sel, nb, r_bias=None, strided=False):
    """launch into a banded (nb, 3, X) float64 buffer -> host part; bands intact, inputs unchanged"""
    X = x.shape[1]
    xd, rd = torch.from_numpy(x).to(dev), torch.from_numpy(r).to(dev)
    if strided:
        wide = torch.full((x.shape[0], 2 * X + 3), SENTINEL, device=dev)
        wide[:, 1:1 + X], wide[:, 1 + X:1 + 2 * X] = xd, rd
        xd, rd = wide[:, 1:1 + X], wide[:, 1 + X:1 + 2 * X]
        keep = (wide, wide.clone())
    else:
        keep = (torch.cat([xd, rd]), torch.cat([xd, rd]).clone())
    seld = torch.from_numpy(sel).to(dev) if sel is not None else None
    bd = torch.from_numpy(r_bias).to(dev) if r_bias is not None else None
    part, big = _flat64(nb * 3 * X, dev)
    K.col_moments(None, xd, rd, sel=seld, part=part.view(nb, 3, X), r_bias=bd)
    got = host(part).view(nb, 3, X).clone()
    assert _flat_intact(big, nb * 3 * X)
    assert torch.equal(keep[0], keep[1]) if strided else torch.equal(torch.cat([xd, rd]), keep[1])
    assert sel is None or np.array_equal(host(seld).numpy(), sel)
    return got


@pytest.mark.parametrize('X', COL_XS)
@pytest.mark.parametrize('M', COL_MS)
def test_col_moments_against_float64(K, dev, M, X):
    seen = {}
    for name in ('normal', 'offset'):
        rs = np.random.RandomState(M + X)
        for vn, (sel, rows_all) in _sel_variants(rs, M).items():
            c = G.profile(name, rows_all, X)
            nb = K.col_moment_blocks(M)
            raw = vn in ('permutation', 'from_larger')          # r as the raw product with its bias
            strided = vn in ('sorted_subset', 'from_larger')
            r = c['mu_raw'] if raw else c['r']
            ref, bnd = G.col_reference(c['x'], r, sel=sel, r_bias=c['bm'] if raw else None)
            got = _col_run(K, dev, c['x'], r, sel, nb, r_bias=c['bm'] if raw else None, strided=strided)
            assert torch.isfinite(got).all()
            w = ref64.check('dv_col_moments %s M=%d X=%d sel %s' % (name, M, X, vn), got.sum(0), torch.from_numpy(ref), torch.from_numpy(bnd))
            _note(seen, 'dv_col_moments (margin %g included)' % G.COL_MARGIN, w)
            if raw:         # the finished reconstruction, rounded to fp32 on the host: the same bits
                fin = (c['mu_raw'] + c['bm']).astype(f)
                assert torch.equal(_col_run(K, dev, c['x'], fin, sel, nb, strided=strided), got)
    _report(seen)


def test_col_moments_leaves_empty_blocks_zero(K, dev):
    """a caller-chosen block count: M = 9 over 4 blocks is ceil = 3 rows per block, the fourth is empty -- zeros, not what
    the buffer held: the sharded evaluation adds every block up"""
    c = _case('normal', 9, 13)
    got = _col_run(K, dev, c['x'], c['r'], None, 4)
    assert (got[3] == 0).all() and (got[:3, 1] > 0).all()
    ref, bnd = G.col_reference(c['x'], c['r'])
    ref64.check('dv_col_moments 4 blocks of 9 rows', got.sum(0), torch.from_numpy(ref), torch.from_numpy(bnd))
    for b in range(3):
        refb, bndb = G.col_reference(c['x'][3 * b:3 * b + 3], c['r'][3 * b:3 * b + 3])
        ref64.check('dv_col_moments block %d' % b, got[b], torch.from_numpy(refb), torch.from_numpy(bndb))
    sel = np.asarray([8, 0, 3, 3, 5], np.int32)          # ceil(5 / 64) = 1 row per block: 59 empty blocks
    got = _col_run(K, dev, c['x'], c['r'], sel, 64)
    assert (got[5:] == 0).all()
    ref, bnd = G.col_reference(c['x'], c['r'], sel=sel)
    ref64.check('dv_col_moments 64 blocks of 5 rows', got.sum(0), torch.from_numpy(ref), torch.from_numpy(bnd))


# ----------------------------------------------------------------------------------------- dv_recon_finalize
def _fin_run(K, dev, rows, part, ll, sel, n, X):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ins = [t(rows), t(part), t(ll), t(sel)]
    keep = [None if a is None else a.clone() for a in ins]
    outs = []
    for rep in range(2):
        out, big = _flat64(4, dev)
        K.recon_finalize(out, ins[0], ins[1], X, sel=ins[3], n=n, ll=ins[2])
        outs.append(host(out).numpy().copy())
        assert _flat_intact(big, 4)
    assert outs[0].tobytes() == outs[1].tobytes()           # two calls: identical bytes
    for a, b in zip(ins, keep):
        assert a is None or torch.equal(a, b)
    return outs[0]


@pytest.mark.parametrize('X', FIN_XS)
@pytest.mark.parametrize('n', FIN_NS)
def test_finalize_against_extended_precision(K, dev, n, X):
    names = ('rmse', 'r2', 'pearr', 'll')
    seen = {}
    for B in FIN_BLOCKS:
        for with_sel in (False, True):
            rows, part, ll, sel = G.finalize_case(n, X, B, with_sel)
            assert B < 3 or (part[-1] == 0).all()           # (unused blocks, zero as the sharded path leaves them)
            for use_ll in ((True, False) if B == 3 else (True,)):
                lv = ll if use_ll else None
                ref, bnd = G.finalize_reference(rows, part, lv, sel, n, X)
                got = _fin_run(K, dev, rows, part, lv, sel, n, X)
                w = G.fin_excess(got, ref, bnd)
                assert (w <= 1.0).all(), (n, X, B, with_sel, use_ll, got, ref, w)
                for k in range(4):
                    _note(seen, 'dv_recon_finalize %s' % names[k], w[k])
                assert np.isnan(got[3]) == (not use_ll or n == 0)
                if n == 0:
                    assert np.isnan(got).all()
    _report(seen)


@pytest.mark.parametrize('name', ['expression', 'offset', 'zero_rows'])
def test_finalize_on_the_references_rows(K, dev, name):
    """inputs produced by the reference from profiles (b)-(d), ``sel`` unsorted into a larger ``rows``"""
    rows, part, ll, sel = profile_finalize_case(name)
    ref, bnd = G.finalize_reference(rows, part, ll, sel, 130, 13)
    got = _fin_run(K, dev, rows, part, ll, sel, 130, 13)
    w = G.fin_excess(got, ref, bnd)
    print(name, 'dv_recon_finalize', got, 'reference', ref, 'fraction of the bound', w)
    assert (w <= 1.0).all(), (got, ref, w)
    assert np.isnan(got[2]) == (name == 'zero_rows') and np.isfinite(got[[0, 1, 3]]).all()


def test_finalize_is_capturable(K, dev):
    """no allocation, no synchronisation: the launch records into a graph, the replay reads the arrays as they are then"""
    n, X = 1025, 13
    rows, part, ll, sel = G.finalize_case(n, X, 3, True)
    t = lambda a: torch.from_numpy(a).to(dev)
    rows_d, part_d, ll_d, sel_d = t(rows), t(part), t(ll), t(sel)
    out = torch.zeros(4, dtype=torch.float64, device=dev)
    K.recon_finalize(out, rows_d, part_d, X, sel=sel_d, n=n, ll=ll_d)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        K.recon_finalize(out, rows_d, part_d, X, sel=sel_d, n=n, ll=ll_d)
    rows_d[:, 0].mul_(0.5)
    ll_d.add_(1.0)
    part_d[:, 2].mul_(0.25)
    g.replay()
    ref, bnd = G.finalize_reference(host(rows_d).numpy(), host(part_d).numpy(), host(ll_d).numpy(), sel, n, X)
    w = G.fin_excess(host(out).numpy(), ref, bnd)
    assert (w <= 1.0).all(), w
