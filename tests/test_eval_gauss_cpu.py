"""CPU checks of the Gaussian evaluation metric launches' references (``tests/eval_gauss_ref.py``): the float64 references
are the plain formulas; a careful emulation of every launch in its own arithmetic and the CPU stand-ins of
``tests/kernel_ref.py`` stay inside the bounds over the shape and profile grid of the GPU tests (the worst fraction of the
bound is printed: run with -s); every faulty emulation lands outside on a named case where the careful one is inside; the
rank reference equals scikit-learn and ``drvae_amd.metrics``; the ``pred=None`` accuracy contract."""
import math

import numpy as np
import pytest
import torch

from tests import eval_gauss_ref as G
from tests import kernel_ref
from tests import ref64

XS = (1, 2, 13, 63, 64, 65, 127, 128, 130, 978, 1022, 1023, 1024)
MS = (1, 3, 4, 5, 130)
XS_STATS_ONLY = (1025, 2052, 4100)
PROFILE_XS = (13, 978, 1024)
COL_MS = (1, 15, 16, 17, 255, 256, 257, 4097, 8193)
COL_XS = (1, 63, 64, 65, 130)
RANK_NS = (1, 2, 255, 256, 257, 511, 512, 513, 1025, 32768)
RANK_MODES = ((2, 1, 1, True), (3, 0, 3, False), (4, 1, 2, False))      # (Y, c0, n_cls, binary)
f = np.float32


def _ex(got, ref, bnd):
    return ref64.excess(torch.from_numpy(np.asarray(got, np.float64)), ref, bnd)


def _row_cases():
    for X in XS:
        for M in MS:
            yield 'normal', M, X
    for X in PROFILE_XS:
        for name in G.PROFILES:
            yield name, 5, X


# ------------------------------------------------------------------------------------ 1. references and profiles
def test_references_are_the_plain_float64_formulas():
    c = G.profile('normal', 5, 13)
    rows, _ = G.rows_reference(c['x'], c['r'])
    x, r = c['x'].astype(np.float64), c['r'].astype(np.float64)
    rows = rows.numpy()
    assert np.allclose(rows[:, 0], ((x - r) ** 2).sum(1), rtol=1e-13)
    assert np.allclose(rows[:, 1], x.mean(1), rtol=1e-13) and np.allclose(rows[:, 2], r.mean(1), rtol=1e-13)
    assert np.allclose(rows[:, 3], x.var(1) * 13, rtol=1e-12) and np.allclose(rows[:, 4], r.var(1) * 13, rtol=1e-12)
    assert np.allclose(rows[:, 5], np.asarray([np.cov(x[i], r[i], bias=True)[0, 1] * 13 for i in range(5)]), rtol=1e-11)
    import scipy.stats as st
    ll, _ = G.ll_reference(c['x'], c['r'], sd=c['sd'])
    assert np.allclose(ll.numpy(), st.norm.logpdf(x, r, c['sd'].astype(np.float64)).sum(1), rtol=1e-12)
    rr, _, pre = G.finished(c, raw=True)
    ll, _ = G.ll_reference(c['x'], rr, pre=pre)
    sd = np.log1p(np.exp(pre.astype(np.float64))) + ref64.f32(G.SHIFT)
    assert np.allclose(ll.numpy(), st.norm.logpdf(x, rr.astype(np.float64), sd).sum(1), rtol=1e-12)
    cols, _ = G.col_reference(c['x'], c['r'])
    assert np.allclose(cols, [x.sum(0), (x * x).sum(0), ((x - r) ** 2).sum(0)], rtol=1e-13)
    # the finalizer's formulas on exact inputs == the metrics of the data they came from (sklearn's variance-weighted R^2)
    from sklearn.metrics import r2_score
    out, _ = G.finalize_reference(rows.astype(f), cols[None], ll.numpy().astype(f), None, 5, 13)
    assert out[0] == pytest.approx(np.sqrt(((x - r) ** 2).mean()), rel=1e-6)
    assert out[1] == pytest.approx(r2_score(x, r, multioutput='variance_weighted'), rel=1e-9)
    assert out[2] == pytest.approx(np.mean([np.corrcoef(x[i], r[i])[0, 1] for i in range(5)]), rel=1e-5)
    assert G.C_STAT <= ref64.C_MAX and G.C_NLL <= ref64.C_MAX


def test_the_summation_rule_describes_a_wave_per_row():
    """a lane of ``recon_row_stats_kernel`` makes 65 additions at X = 4100: ``ref64.row_sum_bound`` (33 U) is too small there"""
    one = torch.ones(1, 4100, dtype=torch.float64)
    assert float(G.wave_sum_bound(one, 4100)) == (65 + 6) * ref64.U * 4100
    assert float(ref64.row_sum_bound(one, 4100)) < 65 * ref64.U * 4100
    assert float(G.wave_sum_bound(one[:, :1024], 1024)) == 22 * ref64.U * 1024


def test_profiles_are_what_they_claim():
    for X in PROFILE_XS:
        c = G.profile('expression', 5, X)
        rows, _ = G.rows_reference(c['x'], c['r'])
        mx = rows[:, 1].numpy()
        assert (mx > 0.5).all() and (mx < 3.5).all(), mx
        pear = (rows[:, 5] / torch.sqrt(rows[:, 3] * rows[:, 4])).numpy()
        assert (pear > 0.99).all(), pear
        c = G.profile('zero_rows', 5, X)
        for raw in (False, True):
            r = G.finished(c, raw)[0]
            assert (c['x'][0] == 0).all() and (r[1] == 0).all()
            rows, bnd = G.rows_reference(c['x'], r)
            assert (rows[0, [1, 3, 5]] == 0).all() and (bnd[0, [1, 3, 5]] == 0).all()
            assert (rows[1, [2, 4, 5]] == 0).all() and (bnd[1, [2, 4, 5]] == 0).all()
        c = G.profile('const_rows', 5, X)
        assert (c['x'][0] == f(2.5)).all() and (c['r'][1] == f(-0.75)).all()
        c = G.profile('offset', 5, X)
        assert abs(float(c['x'].mean()) - 1000.0) < 1.0


# ------------------------------------------------------------------------------- 2. the row launches' emulation
@pytest.mark.parametrize('raw', [False, True])
def test_careful_row_emulation_is_inside_the_bounds(raw):
    worst = np.zeros(7)
    for name, M, X in _row_cases():
        c = G.profile(name, M, X)
        r, sd, pre = G.finished(c, raw)
        rows_ref, rows_b = G.rows_reference(c['x'], r)
        ll_ref, ll_b = G.ll_reference(c['x'], r, sd=sd, pre=pre)
        for v2 in ((False, True) if X % 2 == 0 else (False,)):
            if raw:
                em = G.emulate_rows(c['x'], c['mu_raw'], c['sd_raw'], bias=(c['bm'], c['bs']), v2=v2)
            else:
                em = G.emulate_rows(c['x'], r, sd, v2=v2)
            w = np.append(_ex(em['rows'], rows_ref, rows_b).max(0)[0].numpy(), float(_ex(em['ll'], ll_ref, ll_b).max()))
            assert (w <= 1.0).all(), (name, M, X, raw, v2, w)
            worst = np.maximum(worst, w)
    print('dv_recon_rows emulation (%s heads): worst fraction of the bound [sse mx mr cxx crr cxr | ll] %s'
          % ('raw' if raw else 'finished', np.array2string(worst, precision=3)))
    assert (worst > 1e-3).all(), 'a bound nothing comes near is vacuous'


def test_careful_row_stats_emulation_beyond_the_register_width():
    worst = np.zeros(6)
    for X in XS_STATS_ONLY:
        for name in ('normal', 'offset'):
            c = G.profile(name, 5, X)
            ref, bnd = G.rows_reference(c['x'], c['r'])
            w = _ex(G.emulate_rows(c['x'], c['r'])['rows'], ref, bnd).max(0)[0].numpy()
            assert (w <= 1.0).all(), (name, X, w)
            worst = np.maximum(worst, w)
    print('dv_recon_row_stats emulation, X in %s: worst fraction of the bound %s' % (XS_STATS_ONLY, np.array2string(worst, precision=3)))


def test_offset_rows_raw_moments_lose_everything():
    """profile (c): the careful emulation inside, centred sums from raw moments far outside, in all three of them"""
    for X in PROFILE_XS:
        c = G.profile('offset', 5, X)
        ref, bnd = G.rows_reference(c['x'], c['r'])
        for v2 in ((False, True) if X % 2 == 0 else (False,)):
            assert float(_ex(G.emulate_rows(c['x'], c['r'], v2=v2)['rows'], ref, bnd).max()) <= 1.0
            ex = _ex(G.emulate_rows(c['x'], c['r'], v2=v2, fault='raw_moments')['rows'], ref, bnd)
            for col in (3, 4, 5):
                print('raw_moments, offset rows, X = %d, column %d: worst %.3g x bound' % (X, col, float(ex[:, col].max())))
                assert float(ex[:, col].max()) >= 100.0, (X, col)


@pytest.mark.parametrize('fault,name,X,raw,cols,ll_too', [
    ('mean_over_ld', 'expression', 13, False, (1, 2, 3, 4, 5), False),
    ('drop_last_odd', 'normal', 13, False, (0, 1, 2, 3, 4, 5), True),
    ('drop_last_odd', 'normal', 1023, True, (0, 1, 2, 3, 4, 5), True),
    ('pair_bias', 'normal', 130, True, (0, 2, 4, 5), True),
    ('pair_bias', 'normal', 1024, True, (0, 2, 4, 5), True)])
def test_faulty_row_emulations_are_outside(fault, name, X, raw, cols, ll_too):
    c = G.profile(name, 5, X)
    r, sd, pre = G.finished(c, raw)
    rows_ref, rows_b = G.rows_reference(c['x'], r)
    ll_ref, ll_b = G.ll_reference(c['x'], r, sd=sd, pre=pre)
    v2 = fault == 'pair_bias'
    args = (c['x'], c['mu_raw'], c['sd_raw']) if raw else (c['x'], r, sd)
    kw = dict(bias=(c['bm'], c['bs'])) if raw else {}
    good = G.emulate_rows(*args, v2=v2, **kw)
    bad = G.emulate_rows(*args, v2=v2, fault=fault, ld=X + 3, **kw)
    assert float(_ex(good['rows'], rows_ref, rows_b).max()) <= 1.0 and float(_ex(good['ll'], ll_ref, ll_b).max()) <= 1.0
    ex = _ex(bad['rows'], rows_ref, rows_b)
    for col in cols:
        print('%s, %s, X = %d, column %d: worst %.3g x bound' % (fault, name, X, col, float(ex[:, col].max())))
        assert float(ex[:, col].max()) >= 10.0, (fault, col)
    if ll_too:
        w = float(_ex(bad['ll'], ll_ref, ll_b).max())
        print('%s, %s, X = %d, ll: worst %.3g x bound' % (fault, name, X, w))
        assert w >= 10.0


# ------------------------------------------------------------------------------------------ 3. dv_col_moments
def _sel_variants(rs, M):
    """name -> (sel | None, rows of the matrix)"""
    return {'absent': (None, M),
            'sorted_subset': (np.sort(rs.permutation(M + 5)[:M]).astype(np.int32), M + 5),
            'permutation': (rs.permutation(M).astype(np.int32), M),
            'repeats': (rs.randint(0, max(M // 2, 1), M).astype(np.int32), M),
            'from_larger': (rs.permutation(2 * M + 3)[:M].astype(np.int32), 2 * M + 3)}


def test_careful_col_emulation_is_inside_the_bounds():
    worst = 0.0
    for M in COL_MS:
        for X in COL_XS:
            for name in ('normal', 'offset'):
                rs = np.random.RandomState(M + X)
                variants = _sel_variants(rs, M)
                kind = list(variants)[(M + X) % 5] if M > 257 else None         # (the large M: one variant each, all of them over the grid)
                for vn, (sel, rows_all) in variants.items():
                    if kind is not None and vn != kind:
                        continue
                    c = G.profile(name, rows_all, X)
                    ref, bnd = G.col_reference(c['x'], c['r'], sel=sel)
                    nb = kernel_ref.col_moment_blocks(M)
                    part = G.emulate_col(c['x'], c['r'], sel=sel, row_blocks=nb)
                    w = float(_ex(part.sum(0), torch.from_numpy(ref), torch.from_numpy(bnd)).max())
                    assert w <= 1.0, (M, X, name, vn, w)
                    worst = max(worst, w)
    print('dv_col_moments emulation: worst fraction of the bound (margin %g included) %.3g' % (G.COL_MARGIN, worst))
    # trailing blocks a caller-chosen count leaves empty stay zero: M = 9 over 4 blocks is 3 rows per block
    c = G.profile('normal', 9, 13)
    part = G.emulate_col(c['x'], c['r'], row_blocks=4)
    assert (part[3] == 0).all() and (part[:3] != 0).any()
    # r_bias: the reference rounds r + r_bias to fp32 first, so the raw product and the finished one give the same sums
    c = G.profile('normal', 40, 65)
    fin = (c['mu_raw'] + c['bm']).astype(f)
    a, _ = G.col_reference(c['x'], c['mu_raw'], r_bias=c['bm'])
    b, bnd = G.col_reference(c['x'], fin)
    assert np.array_equal(a, b)
    assert float(_ex(G.emulate_col(c['x'], c['mu_raw'], r_bias=c['bm'], row_blocks=2).sum(0), torch.from_numpy(b), torch.from_numpy(bnd)).max()) <= 1.0


@pytest.mark.parametrize('fault,name,M,X', [('sel_ignored', 'normal', 257, 65), ('fp32', 'normal', 257, 65), ('fp32', 'offset', 8193, 13),
                                            ('fp32', 'normal', 17, 1)])
def test_faulty_col_emulations_are_outside(fault, name, M, X):
    rs = np.random.RandomState(3)
    sel = rs.permutation(2 * M + 3)[:M].astype(np.int32)
    c = G.profile(name, 2 * M + 3, X)
    ref, bnd = G.col_reference(c['x'], c['r'], sel=sel)
    ref, bnd = torch.from_numpy(ref), torch.from_numpy(bnd)
    nb = kernel_ref.col_moment_blocks(M)
    assert float(_ex(G.emulate_col(c['x'], c['r'], sel=sel, row_blocks=nb).sum(0), ref, bnd).max()) <= 1.0
    ex = _ex(G.emulate_col(c['x'], c['r'], sel=sel, row_blocks=nb, fault=fault).sum(0), ref, bnd)
    for k in range(3):
        print('col_moments %s, %s, M = %d, X = %d, statistic %d: worst %.3g x bound' % (fault, name, M, X, k, float(ex[k].max())))
        assert float(ex[k].max()) >= 10.0, (fault, k)


# ---------------------------------------------------------------------------------------- 4. dv_recon_finalize
FIN_NS = (0, 1, 1023, 1024, 1025, 5000)
FIN_XS = (1, 13, 1025, 2052)
FIN_BLOCKS = (1, 3, 64, 128)


def profile_finalize_case(name, n=130, X=13, n_all=200, blocks=3):
    """finalizer inputs produced by the reference from a profile: fp32 rows / ll of all rows, the float64 column sums of the
    selected ones in the first block (the others zero), an unsorted ``sel``"""
    c = G.profile(name, n_all, X)
    rs = np.random.RandomState(n + X)
    sel = rs.permutation(n_all)[:n].astype(np.int32)
    rows = G.rows_reference(c['x'], c['r'])[0].numpy().astype(f)
    ll = G.ll_reference(c['x'], c['r'], sd=c['sd'])[0].numpy().astype(f)
    part = np.zeros((blocks, 3, X))
    part[0] = G.col_reference(c['x'], c['r'], sel=sel)[0]
    return rows, part, ll, sel


def test_careful_finalize_emulation_is_inside_the_bounds():
    worst = np.zeros(4)
    for n in FIN_NS:
        for X in FIN_XS:
            for B in FIN_BLOCKS:
                for with_sel in (False, True):
                    rows, part, ll, sel = G.finalize_case(n, X, B, with_sel)
                    for use_ll in ((True, False) if (B == 3 and X == 13) else (True,)):
                        lv = ll if use_ll else None
                        ref, bnd = G.finalize_reference(rows, part, lv, sel, n, X)
                        w = G.fin_excess(G.emulate_finalize(rows, part, lv, sel, n, X), ref, bnd)
                        assert (w <= 1.0).all(), (n, X, B, with_sel, use_ll, w, ref)
                        worst = np.maximum(worst, w)
                        if n == 0:
                            assert np.isnan(ref).all()
                        elif n == 1:
                            assert np.isfinite(ref[[0, 2]]).all() and ref[1] == -math.inf          # (one row: no variance to explain)
                        else:
                            assert np.isfinite(ref[:3]).all() and np.isnan(ref[3]) == (not use_ll)
    for name in ('expression', 'offset', 'zero_rows'):
        rows, part, ll, sel = profile_finalize_case(name)
        ref, bnd = G.finalize_reference(rows, part, ll, sel, 130, 13)
        w = G.fin_excess(G.emulate_finalize(rows, part, ll, sel, 130, 13), ref, bnd)
        assert (w <= 1.0).all(), (name, w)
        worst = np.maximum(worst, w)
        # (d): the zero rows make the mean Pearson r NaN -- in the reference too -- and leave the rest finite
        assert np.isnan(ref[2]) == (name == 'zero_rows') and np.isfinite(ref[[0, 1, 3]]).all()
    print('dv_recon_finalize emulation: worst fraction of the bound [rmse r2 pearr ll] %s' % np.array2string(worst, precision=3))


@pytest.mark.parametrize('source', ['random', 'expression', 'offset'])
def test_faulty_finalize_emulations_are_outside(source):
    if source == 'random':
        n, X = 5000, 13
        rows, part, ll, sel = G.finalize_case(n, X, 3, True)
    else:
        n, X = 130, 13
        rows, part, ll, sel = profile_finalize_case(source)
    ref, bnd = G.finalize_reference(rows, part, ll, sel, n, X)
    assert (G.fin_excess(G.emulate_finalize(rows, part, ll, sel, n, X), ref, bnd) <= 1.0).all()
    w = G.fin_excess(G.emulate_finalize(rows, part, ll, sel, n, X, fault='fp32'), ref, bnd)
    print('finalize fp32 accumulation, %s: %s x bound' % (source, np.array2string(w, precision=3)))
    assert (w >= 10.0).all(), w
    w = G.fin_excess(G.emulate_finalize(rows, part, ll, sel, n, X, fault='ll_position'), ref, bnd)
    print('finalize ll[e] for ll[sel[e]], %s: %s x bound' % (source, np.array2string(w, precision=3)))
    assert w[3] >= 10.0 and (w[:3] <= 1.0).all(), w


# ------------------------------------------------------------------------------------------ 5. the stand-ins
def test_stand_ins_are_inside_the_bounds():
    t = torch.from_numpy
    for name, M, X in list(_row_cases()) + [('normal', 5, X) for X in XS_STATS_ONLY] + [('offset', 5, 4100)]:
        c = G.profile(name, M, X)
        rows = torch.full((M, 6), 7.0)
        kernel_ref.recon_row_stats(rows, t(c['x']), t(c['r']))
        ref, bnd = G.rows_reference(c['x'], c['r'])
        assert float(ref64.excess(rows, ref, bnd).max()) <= 1.0, ('recon_row_stats', name, M, X)
        if X > kernel_ref.RECON_ROWS_MAX_X:
            continue
        for raw in (False, True):
            r, sd, pre = G.finished(c, raw)
            rows, ll = torch.full((M, 6), 7.0), torch.full((M,), 7.0)
            if raw:
                kernel_ref.recon_rows(rows, ll, t(c['x']), t(c['mu_raw']), t(c['sd_raw']), bias=(t(c['bm']), t(c['bs'])), sd_shift=G.SHIFT)
            else:
                kernel_ref.recon_rows(rows, ll, t(c['x']), t(r), t(sd))
            ref, bnd = G.rows_reference(c['x'], r)
            assert float(ref64.excess(rows, ref, bnd).max()) <= 1.0, ('recon_rows rows', name, M, X, raw)
            ref, bnd = G.ll_reference(c['x'], r, sd=sd, pre=pre)
            assert float(ref64.excess(ll, ref, bnd).max()) <= 1.0, ('recon_rows ll', name, M, X, raw)
    for M in COL_MS:
        for X in (1, 65):
            rs = np.random.RandomState(M)
            for vn, (sel, rows_all) in _sel_variants(rs, M).items():
                c = G.profile('offset' if M % 2 else 'normal', rows_all, X)
                nb = 4 if M == 17 else kernel_ref.col_moment_blocks(M)
                part = torch.full((nb, 3, X), 7.0, dtype=torch.float64)
                kernel_ref.col_moments(None, t(c['x']), t(c['mu_raw']), sel=None if sel is None else t(sel), part=part, r_bias=t(c['bm']))
                ref, bnd = G.col_reference(c['x'], c['mu_raw'], sel=sel, r_bias=c['bm'])
                assert float(_ex(part.sum(0).numpy(), t(ref), t(bnd)).max()) <= 1.0, ('col_moments', M, X, vn)
    for n in FIN_NS:
        for X in (1, 1025):
            for with_sel in (False, True):
                rows, part, ll, sel = G.finalize_case(n, X, 3, with_sel)
                rows_all = np.concatenate([rows, rows[:5] + 1]) if not with_sel else rows      # (sel NULL: the first n rows count)
                ll_all = np.concatenate([ll, ll[:5] + 1]) if not with_sel else ll
                out = torch.full((4,), 7.0, dtype=torch.float64)
                kernel_ref.recon_finalize(out, t(rows_all), t(part), X, sel=None if sel is None else t(sel), n=n, ll=t(ll_all))
                ref, bnd = G.finalize_reference(rows_all, part, ll_all, sel, n, X)
                bnd = np.maximum(bnd, 64 * G.U64 * np.abs(np.nan_to_num(ref, posinf=0, neginf=0)))       # (torch's own sums: not the kernel's order)
                assert (G.fin_excess(out.numpy(), ref, bnd) <= 1.0).all(), ('recon_finalize', n, X, with_sel, out, ref)


# ----------------------------------------------------------------------------------------- 6. rank metrics
@pytest.mark.parametrize('n', RANK_NS)
def test_rank_reference_is_scikit_learn_and_the_package_metrics(n):
    from sklearn.metrics import average_precision_score, roc_auc_score, roc_curve
    from drvae_amd import metrics as MET
    seen = 0
    for Y, c0, n_cls, binary in RANK_MODES:
        for pattern in G.RANK_PATTERNS:
            proba, y, pred, sel = G.rank_case(n, pattern, Y)
            want = G.rank_expected(proba, y, pred, sel, c0, n_cls, binary)
            idx = sel.astype(np.int64)
            for c in range(n_cls):
                pos = (y[idx] > 0) if binary else (y[idx] == c0 + c)
                s = proba[idx, c0 + c]
                if pos.any() and not pos.all():
                    # exactly scikit-learn's curve: its (fpr, tpr) points are integer counts over n_neg / n_pos, recovered here
                    # without loss, and their trapezoids are the same rational, divided once.  ``roc_auc_score`` itself rounds
                    # at every point and trapezoid (1 ulp off the rational at n = 255, three-value grid): 1e-12, the tolerance
                    # ``test_rank_metrics_without_a_sort`` holds it to
                    fpr, tpr, _ = roc_curve(pos, s.astype(np.float64), drop_intermediate=False)
                    n_pos = int(pos.sum())
                    fps, tps = np.rint(fpr * (n - n_pos)).astype(np.int64), np.rint(tpr * n_pos).astype(np.int64)
                    assert np.array_equal(fps / (n - n_pos), fpr) and np.array_equal(tps / n_pos, tpr)
                    area2 = sum(int(fps[i + 1] - fps[i]) * int(tps[i + 1] + tps[i]) for i in range(len(fps) - 1))
                    assert want[2 * c] == area2 / (2 * n_pos * (n - n_pos)), (n, pattern, Y, c)
                    assert abs(want[2 * c] - roc_auc_score(pos, s.astype(np.float64))) <= 1e-12
                    assert want[2 * c] == MET.roc_auc(torch.from_numpy(pos), torch.from_numpy(s))
                    if pattern == 'equal':
                        assert want[2 * c] == 0.5
                    seen += 1
                else:
                    assert np.isnan(want[2 * c])
                if pos.any():
                    assert abs(want[2 * c + 1] - average_precision_score(pos, s.astype(np.float64))) <= 1e-12
                    assert abs(want[2 * c + 1] - MET.average_precision(torch.from_numpy(pos), torch.from_numpy(s))) <= 1e-12
                else:
                    assert want[2 * c + 1] == 0.0
            assert want[2 * n_cls] == float(f((pred[idx] == y[idx]).sum()) / f(n))
    assert seen or n == 1


def test_rank_reference_orders_signed_zeros_and_subnormals():
    auc, ap = G.rank_reference(np.asarray([-0.0, 0.0], f), [True, False])
    assert auc == 0.5 and ap == 0.5
    auc, ap = G.rank_reference(np.asarray([2e-40, 1e-40], f), [True, False])
    assert auc == 1.0 and ap == 1.0
    auc, ap = G.rank_reference(np.asarray([1e-40, 2e-40], f), [True, False])
    assert auc == 0.0 and ap == 0.5
    assert np.isnan(G.rank_reference(np.zeros(3, f), [True] * 3)[0]) and G.rank_reference(np.zeros(3, f), [False] * 3)[1] == 0.0
    assert np.isnan(G.rank_reference(np.zeros(0, f), [])[0])


def test_the_stand_in_keeps_the_rank_contract():
    """``kernel_ref.rank_metrics`` against the reference, and THE ``pred=None`` contract: the accuracy slot is NaN -- no
    prediction given is not 0 % correct (every caller in ``fit.py`` passes one)"""
    assert math.isnan(G.ACC_WITHOUT_PRED)
    t = torch.from_numpy
    for n in (1, 257, 1025):
        for Y, c0, n_cls, binary in RANK_MODES:
            for pattern in G.RANK_PATTERNS:
                proba, y, pred, sel = G.rank_case(n, pattern, Y)
                for with_pred in (True, False):
                    out = torch.full((2 * n_cls + 1,), 7.0, dtype=torch.float64)
                    kernel_ref.rank_metrics(out, None, t(proba), t(y), pred32=t(pred) if with_pred else None, sel=t(sel), c0=c0, n_cls=n_cls,
                                            binary=binary)
                    want = G.rank_expected(proba, y, pred if with_pred else None, sel, c0, n_cls, binary)
                    got = out.numpy()
                    assert np.array_equal(np.isnan(got), np.isnan(want)), (n, Y, pattern, got, want)
                    assert np.nanmax(np.abs(got - want), initial=0.0) <= 1e-12
                    assert np.isnan(got[2 * n_cls]) == (not with_pred)
