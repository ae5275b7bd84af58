"""GPU: the fp32 MFMA GEMM family -- ``dv_gemm``, ``dv_gemm_pair``, ``dv_gemm_heads`` and the ragged-N split -- against its
arithmetic and memory contract, on every kernel variant ("route": a forced tiling plus dispatcher options,
tests/gemm_contract.py), layout and operand class:

1. identities that must hold bit for bit (one exact product per output),
2. accuracy against float64: an element-wise bound that is derived (K fma roundings + the K split's additions + the
   epilogue's own) and a norm-wise one (at most 2 x the error of a plain sequential fp32 fma chain),
3. the memory contract under poison: operands are views cut out of NaN-filled buffers (row pads, guard rows), outputs views
   in sentinel-filled buffers, pre-filled with NaN where beta == 0 -- every output finite and inside the bound, not a byte
   written outside a view, no operand changed,
4. non-finite operand elements poison exactly the outputs they feed,
5. every workgroup -> tile map covers every tile of a ragged grid,
6. the same descriptor twice gives the same bits,
7. beta == 0 never reads the output, for every launcher of drvae_amd/kernels.py that takes a beta.

tests/test_gemm_contract_cpu.py shows on the same operands that the references pass these checks and that faulty
emulations fail them.  Nothing here provokes a fault: the guard rows are there so that a stray access stays inside the
allocation and shows up as a NaN or a changed sentinel."""
import functools

import numpy as np
import pytest
import torch

from tests import gemm_contract as G
from tests import ref64
from tests.gemm_contract import CASES, EPILOGUES, LAYOUTS, NAN, ROUTES, SHIFT, U, Frame, case_id, route_id, routed
from tests.test_gpu_kernels import PRODUCT_TILINGS, tilings
from tests.test_gpu_x3 import store

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def K(dev):
    import drvae_amd.kernels as K
    from drvae_amd import _lib
    _lib.load()
    return K


def _marks(tiling):
    t = tilings(tiling)[0]                 # lab tilings carry the ``lab`` marker, as elsewhere
    return () if isinstance(t, int) else tuple(t.marks)


def route_params(routes=ROUTES, layouts=None):
    return [pytest.param(r, a, b, id='%s-%d%d' % (route_id(r), a, b), marks=_marks(r[0]))
            for r in routes for a, b in (layouts or G.route_layouts(r)) if a or not r[2]]


ROUTE_LAYOUTS = route_params()
CASE_IDS = [case_id(c) for c in CASES]
assert all(r[0] in PRODUCT_TILINGS for r in ROUTES)


def run_gemm(K, dev, Aop, Bop, a_kc, b_kc, cls, overread, e=None, init=None, **kw):
    """Aop (M, K), Bop (K, N) host tensors -> host result of ``gemm`` in the given layout, every operand a view into a
    poisoned buffer, C pre-filled with NaN unless it accumulates; the memory contract is verified on the way"""
    f = Frame(dev, cls)
    A, B = f.inp(G.stored(Aop, a_kc)), f.inp(G.stored(Bop.t(), b_kc))
    ekw = G.epilogue_kwargs(K, e, f.inp) if e is not None else {}
    if e is not None and e['beta']:
        init = e['C0']
    Cm = f.out(init if init is not None else (Aop.shape[0], Bop.shape[1]))
    K.gemm(Cm, A, B, a_kc, b_kc, overread=overread, **ekw, **kw)
    f.verify()
    return Cm.cpu()


@functools.lru_cache(maxsize=None)
def reference(M, N, Kd, name):
    """(want, bound, yardstick) of epilogue ``name`` on the case's random operands: computed once, shared, never changed"""
    A, B = G.random_operands(M, N, Kd)
    return G.expected(A, B, G.epilogue_case(name, M, N), acc=chain(M, N, Kd))


@functools.lru_cache(maxsize=None)
def chain(M, N, Kd):
    return G.chain_matmul(*G.random_operands(M, N, Kd))


def inside(got, want, bound, what):
    assert bool(torch.isfinite(got).all()), what
    worst = G.worst_excess(got, want, bound)
    assert worst <= 1.0, (what, worst)
    return worst


# ------------------------------------------------------------------------------------------------ 1. exact identities
@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
@pytest.mark.parametrize('route,a_kc,b_kc', ROUTE_LAYOUTS)
def test_exact_identities_bit_for_bit(K, dev, route, a_kc, b_kc, case):
    """A @ P and P @ B with full 24-bit significands against scaled selections: any precision lost in the operands or the
    matrix instruction, a wrong fragment or LDS map, a dropped or doubled K-split partial or a mishandled K tail changes
    bits.  Also as C = -0.5 A P + C0 on small integers: the exact product and one correctly rounded addition."""
    cls, M, N, Kd, over = case
    (A, P), (P2, B), C0 = G.identity_operands(M, N, Kd)
    with routed(K, route):
        assert torch.equal(run_gemm(K, dev, A, P, a_kc, b_kc, cls, over), G.exact_product(A, P))
        assert torch.equal(run_gemm(K, dev, P2, B, a_kc, b_kc, cls, over), G.exact_product(P2, B))
        got = run_gemm(K, dev, A, P, a_kc, b_kc, cls, over, init=C0, alpha=-0.5, beta=1.0)
        assert torch.equal(got, G.exact_product(A, P, -0.5, 1.0, C0))


# ------------------------------------------------------------------------------------------------ 2. accuracy
@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
@pytest.mark.parametrize('route,a_kc,b_kc', ROUTE_LAYOUTS)
def test_accuracy_against_float64(K, dev, route, a_kc, b_kc, case):
    """random normal operands through PLAIN and BWD with (alpha, beta) = (1, 0) and (-0.37, 1), and FWD with scale, bias, a
    split into identity | softplus + shift and a residual.  Element-wise: the derived bound of tests/gemm_contract.py.
    Norm-wise: the Frobenius error against float64 is at most 2 x that of a sequential fp32 fma chain through a plain
    fp32 epilogue (the cap the x3 tests use for the same quantity)."""
    cls, M, N, Kd, over = case
    A, B = G.random_operands(M, N, Kd)
    with routed(K, route):
        for name in EPILOGUES:
            want, bound, yard = reference(M, N, Kd, name)
            got = run_gemm(K, dev, A, B, a_kc, b_kc, cls, over, e=G.epilogue_case(name, M, N))
            worst, ratio = G.worst_excess(got, want, bound), G.norm_ratio(got, yard, want)
            print('gemm accuracy route=%s layout=(%d,%d) case=%s epi=%s: max err/bound %.3f, norm-wise ratio %.3f'
                  % (route_id(route), a_kc, b_kc, case_id(case), name, worst, ratio))
            assert worst <= 1.0, (name, worst)
            assert ratio <= 2.0, (name, ratio)


# ------------------------------------------------------------------------------------------------ 3. memory contract
@pytest.mark.parametrize('case', CASES[:4], ids=CASE_IDS[:4])
@pytest.mark.parametrize('route,a_kc,b_kc', ROUTE_LAYOUTS)
def test_poison_gemm(K, dev, route, a_kc, b_kc, case):
    """``gemm`` with and without the word that row ends may be over-read (no kpad / npad: the pads are NaN, not zero),
    plain, with the forward epilogue's side operands (scale, bias, resid) and the backward's (yref, old C)"""
    cls, M, N, Kd, _ = case
    A, B = G.random_operands(M, N, Kd)
    with routed(K, route):
        for over in (False, True):
            for name in ('plain', 'fwd', 'bwd-ab'):
                want, bound, _ = reference(M, N, Kd, name)
                got = run_gemm(K, dev, A, B, a_kc, b_kc, cls, over, e=G.epilogue_case(name, M, N))
                inside(got, want, bound, (name, over))


FEW_ROUTES = [pytest.param(r, id=route_id(r), marks=_marks(r[0])) for r in ROUTES if r[0] in (0, 1, 17) or 8 in r[1]]


@pytest.mark.parametrize('K1', [50, 52])
@pytest.mark.parametrize('route', FEW_ROUTES)
def test_poison_linear_fwd_two_sources(K, dev, route, K1):
    """``linear_fwd`` with ``x2`` (A2): K1 % 4 != 0 (a chunk could straddle the two sources: scalar loads) and K1 % 4 == 0"""
    M, N, K2 = 70, 90, 30
    A, B = G.random_operands(M, N, K1 + K2, seed=2)
    e = G.epilogue_case('fwd', M, N)
    want, bound, _ = G.expected(A, B, e)
    with routed(K, route):
        for cls in ('A', 'C'):
            for over in (False, True):
                f = Frame(dev, cls)
                x1, x2, W = f.inp(A[:, :K1]), f.inp(A[:, K1:]), f.inp(B.t())
                kw = G.epilogue_kwargs(K, e, f.inp)
                out = f.out((M, N))
                K.linear_fwd(out, x1, W, kw.pop('bias'), x2=x2, overread=over,
                             **{k: v for k, v in kw.items() if k not in ('alpha', 'beta', 'epi')})
                f.verify()
                inside(out.cpu(), want, bound, (cls, over))


@pytest.mark.parametrize('route', FEW_ROUTES)
def test_poison_linear_bwd_data(K, dev, route):
    """``linear_bwd_data`` with ``kscale`` (powers of two: the scaled operand is exact), ``yref`` and beta = 1"""
    _, M, N, Kd, _ = G.BASE
    A, B = G.random_operands(M, N, Kd)
    ks = torch.from_numpy(np.exp2(np.random.RandomState(1).randint(-2, 3, size=Kd)).astype(np.float32))
    e = dict(G.epilogue_case('bwd-ab', M, N), h=N)              # one activation (elu, shift 0) over all columns
    want, bound, _ = G.expected(A * ks, B, e)
    with routed(K, route):
        for cls in ('A', 'C'):
            for over in (False, True):
                f = Frame(dev, cls)
                dpre, W, yref, ksd = f.inp(A), f.inp(B), f.inp(e['yref']), f.inp(ks)
                dx = f.out(e['C0'])
                K.linear_bwd_data(dx, dpre, W, kscale=ksd, alpha=e['alpha'], beta=1.0, yref=yref, act='elu', overread=over)
                f.verify()
                inside(dx.cpu(), want, bound, (cls, over))


DW_ROUTES = [pytest.param(r, id=route_id(r), marks=_marks(r[0])) for r in ROUTES if not r[2]]


@pytest.mark.parametrize('N', [128, 300])
@pytest.mark.parametrize('route', DW_ROUTES)
def test_poison_linear_bwd_weight_with_dbias(K, dev, route, N):
    """``linear_bwd_weight`` with ``dbias``: the ones column on both staging forms (class A with the over-read word: the
    LDS-DMA ring where the route has one; otherwise register-staged), at N a multiple of every tile width (the column needs
    a tile of its own) and ragged; dW and db pre-filled with NaN (beta = colsum_beta = 0).  The 128-class tilings run the
    column sums as a launch of their own."""
    M, Kd = 150, 200
    dy, x = G.random_operands(M, N, Kd, seed=3)          # Aop = dy^T: (M, K); Bop = x: (K, N)
    want, bound, _ = G.expected(dy, x, G.epilogue_case('plain', M, N))
    db64, dbb = G.colsum_bound(dy.t())
    with routed(K, route):
        for cls in ('A', 'C'):
            for over in (False, True):
                f = Frame(dev, cls)
                dpre, xd = f.inp(dy.t()), f.inp(x)
                dW, db = f.out((M, N)), f.out((M,))
                K.linear_bwd_weight(dW, dpre, xd, dbias=db, overread=over)
                f.verify()
                inside(dW.cpu(), want, bound, ('dW', cls, over))
                inside(db.cpu(), db64, dbb + U * db64.abs(), ('db', cls, over))


# (dv_gemm_pair looks at the fused form first: below 1024 tiles the dense dW || dX launch is reached with opt[2] = 1 as well)
PAIR_FORMS = [{}, {2: 1}, {8: 1}, {2: 1, 8: 1}, {2: 1, 8: 1, 9: 1}, {3: -1}, {2: 1, 3: -1}, {2: 1, 3: -1, 8: 1}]


@pytest.mark.parametrize('form', PAIR_FORMS, ids=lambda o: route_id((0, o)))
def test_poison_linear_bwd_pair(K, dev, form):
    """``linear_bwd_pair``: the fused launch (also under opt[8] = 1 alone), two launches (opt[2] = 1), the dense dW || dX
    launch (opt[2] = 1, opt[8] = 1) and its two-launch form (opt[9] = 1); ring and register-staged (opt[3] = -1).  dx accumulates (beta_x = 1) through the
    activation backward, with and without a per-k scale; dW and db are pre-filled with NaN."""
    batch, Nout, Kin = 200, 152, 300
    dy, x = G.random_operands(Nout, Kin, batch, seed=5)                # dW = dy x: (Nout, batch) (batch, Kin)
    W = G.random_operands(batch, Kin, Nout, seed=6)[1]                 # dx = dy^T W: (batch, Nout) (Nout, Kin)
    ks = torch.from_numpy(np.exp2(np.random.RandomState(2).randint(-2, 3, size=Nout)).astype(np.float32))
    wW, bW, _ = G.expected(dy, x, G.epilogue_case('plain', Nout, Kin))
    db64, dbb = G.colsum_bound(dy.t())
    e = dict(G.epilogue_case('bwd-ab', batch, Kin), h=Kin)
    refX = {True: G.expected(dy.t() * ks, W, e), False: G.expected(dy.t(), W, e)}
    with routed(K, (0, form)):
        # (a per-k scale keeps the data gradient, and with it the fused launch, off the LDS-DMA ring: both ways)
        for cls, over, scaled in (('A', False, False), ('A', True, False), ('A', True, True), ('C', False, True), ('C', True, False)):
            f = Frame(dev, cls)
            dpre, xd, Wd, yref = f.inp(dy.t()), f.inp(x), f.inp(W), f.inp(e['yref'])
            ksd = f.inp(ks) if scaled else None
            dW, db, dx = f.out((Nout, Kin)), f.out((Nout,)), f.out(e['C0'])
            K.linear_bwd_pair(dW, db, dx, dpre, xd, Wd, kscale=ksd, alpha=e['alpha'], beta_x=1.0, yref=yref, act='elu',
                              overread=over)
            f.verify()
            inside(dW.cpu(), wW, bW, ('dW', cls, over, scaled))
            inside(db.cpu(), db64, dbb + U * db64.abs(), ('db', cls, over, scaled))
            inside(dx.cpu(), refX[scaled][0], refX[scaled][1], ('dx', cls, over, scaled))


HEADS_FORMS = [{}, {4: 3}, {3: -1}, {3: -1, 4: 3}]


@functools.lru_cache(maxsize=None)
def heads_sample_case():
    """70 rows, two heads of 45 columns (ragged against the 16-wide half tiles), K = 40; 47 source rows fan out to 0 .. 3
    sample rows each through a CSR list; ``out2 = z - sub``, a scattered copy (out3) and a CSR copy (out4)"""
    M, S, Kd, n_src = 70, 45, 40, 47
    g = torch.Generator().manual_seed(11)
    x, Wt = G.random_operands(M, 2 * S, Kd, seed=7)
    e = dict(kind='fwd', alpha=1.0, beta=0.0, h=S, C0=None, act1='identity', shift1=-2.0,
             scale=torch.randn(2 * S, generator=g).abs() + 0.5, bias=torch.randn(2 * S, generator=g),
             resid=torch.randn(M, S, generator=g))
    cnt = [(i % 3) + (1 if i % 5 == 0 else 0) for i in range(n_src)]
    ptr = np.concatenate([[0], np.cumsum(cnt)])
    R_ = int(ptr[-1])
    rows = torch.randperm(R_, generator=g)
    eps, sub = torch.randn(R_, S, generator=g), torch.randn(R_, S, generator=g)
    idx3 = torch.tensor([(i // 2 if i % 2 == 0 else -1) for i in range(R_)])
    ptr4 = np.concatenate([[0], np.cumsum([(i % 3) for i in range(R_)])])
    want, bound, _ = G.expected(x, Wt, e)
    # z = eps * exp(logvar / 2) + mu from the launch's own (mu | logvar): their bounds travel through (e^d - 1 <= d e^d),
    # the exponential on the hardware exp2 (its argument rounds twice: |logvar| U), the product and the sum round once
    src = torch.zeros(R_, dtype=torch.long)
    for m in range(n_src):
        src[rows[int(ptr[m]):int(ptr[m + 1])]] = m
    mu, lv, dmu, dlv = want[src, :S], want[src, S:], bound[src, :S], bound[src, S:]
    sd = torch.exp(0.5 * lv)
    z = eps.double() * sd + mu
    zb = dmu + (eps.double() * sd).abs() * (1.01 * 0.5 * dlv * torch.exp(0.5 * dlv) + U * (8 + 2 * lv.abs())) \
        + 2 * U * ((eps.double() * sd).abs() + z.abs())
    z2 = z - sub.double()
    sel3 = idx3 >= 0
    rep4 = torch.repeat_interleave(torch.arange(R_), torch.tensor(np.diff(ptr4)))
    return dict(M=M, S=S, Kd=Kd, n_src=n_src, x=x, W=Wt.t().contiguous(), e=e, ptr=torch.tensor(ptr, dtype=torch.int32),
                rows=rows.to(torch.int32), eps=eps, sub=sub, idx3=idx3.to(torch.int32), ptr4=torch.tensor(ptr4, dtype=torch.int32),
                want=want, bound=bound, z=z, zb=zb, z2=z2, z2b=zb + U * z2.abs(), n3=int(sel3.sum()), sel3=sel3,
                order3=idx3[sel3], rep4=rep4)


@pytest.mark.parametrize('cls', ['A', 'C'])
@pytest.mark.parametrize('form', HEADS_FORMS, ids=lambda o: route_id((0, o)))
def test_poison_linear_heads_sample(K, dev, form, cls):
    """``linear_heads`` / SAMPLE on the default kernel and the dense variant (opt[4] = 3), ring and register-staged: the
    (mu | logvar) rows and every sample output sit in sentinel buffers, pre-filled with NaN"""
    c = heads_sample_case()
    M, S, e = c['M'], c['S'], c['e']
    R_ = c['eps'].shape[0]
    with routed(K, (0, form)):
        for over in (False, True):
            f = Frame(dev, cls)
            x, W, eps, sub = f.inp(c['x']), f.inp(c['W']), f.inp(c['eps']), f.inp(c['sub'])
            kw = G.epilogue_kwargs(K, e, f.inp)
            q, z, z2 = f.out((M, 2 * S)), f.out((R_, S)), f.out((R_, S))
            o3, o4 = f.out((c['n3'], S)), f.out((int(c['ptr4'][-1]), S))
            K.linear_heads(q, x, W, kw['bias'], split=S, scale=kw['scale'], act0='identity', act1='identity', shift1=-2.0,
                           resid=kw['resid'], resid_cols=S, overread=over,
                           sample=dict(eps=eps, out=z, n_src=c['n_src'], seg_ptr=c['ptr'].to(dev), seg_rows=c['rows'].to(dev),
                                       sub=sub, out2=z2, out3=o3, out3_idx=c['idx3'].to(dev), out4=o4,
                                       out4_ptr=c['ptr4'].to(dev)))
            f.verify()
            inside(q.cpu(), c['want'], c['bound'], ('mu | logvar', over))
            inside(z.cpu(), c['z'], c['zb'], ('z', over))
            inside(z2.cpu(), c['z2'], c['z2b'], ('z - sub', over))
            inside(o3.cpu()[c['order3']], c['z'][c['sel3']], c['zb'][c['sel3']], ('out3', over))
            inside(o4.cpu(), c['z'][c['rep4']], c['zb'][c['rep4']], ('out4', over))


@functools.lru_cache(maxsize=None)
def heads_nll_case():
    """operands on a grid (x in {-2 .. 2}, W in {-2 .. 2} / 16, bias in eighths): every sum is exact in fp32 whatever its
    order, so (mu, pre-activation) reach the epilogue exactly and the bound is the epilogue's alone (tests/ref64.py)"""
    M, S, Kd = 70, 45, 40
    rs = np.random.RandomState(13)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))   # noqa: E731
    x, W = t(rs.randint(-2, 3, size=(M, Kd))), t(rs.randint(-2, 3, size=(2 * S, Kd)) / 16.0)
    b = t(rs.randint(-8, 9, size=2 * S) / 8.0)
    nx = M // 2
    xt = t(np.round(rs.uniform(-3, 3, size=(nx, S)) * 1024) / 1024)
    xidx = torch.tensor([i % nx for i in range(M)], dtype=torch.int32)
    coef = torch.tensor([1.0, -0.5, 2.0, 0.25])[torch.arange(M) % 4]
    heads = x.double() @ W.double().t() + b.double()
    assert torch.equal(heads.float().double(), heads)
    r = ref64.nll_sigma_pre(xt[xidx.long()], heads[:, :S], heads[:, S:], SHIFT, coef=coef[:, None])
    return dict(M=M, S=S, x=x, W=W, b=b, xt=xt, xidx=xidx, coef=coef, r=r)


@pytest.mark.parametrize('cls', ['A', 'C'])
@pytest.mark.parametrize('form', HEADS_FORMS, ids=lambda o: route_id((0, o)))
def test_poison_linear_heads_nll(K, dev, form, cls):
    """``linear_heads`` / NLL: the gradients w.r.t. (mu | pre-activation of std) and the per-tile partial row sums"""
    c = heads_nll_case()
    M, S, r = c['M'], c['S'], c['r']
    nt = K.heads_tiles(S)
    with routed(K, (0, form)):
        for over in (False, True):
            f = Frame(dev, cls)
            x, W, b, xt, coef = f.inp(c['x']), f.inp(c['W']), f.inp(c['b']), f.inp(c['xt']), f.inp(c['coef'])
            out, part = f.out((M, 2 * S)), f.out((M, nt), cls='D')
            K.linear_heads(out, x, W, b, split=S, act0='identity', act1='softplus', shift1=SHIFT, overread=over,
                           nll=dict(x=xt, xidx=c['xidx'].to(dev), coef=coef, part=part))
            f.verify()
            got, rows = out.cpu(), part.cpu()
            inside(got[:, :S], r['gm'], ref64.bound(G.C_NLL, r['gm_c'], r['gm_x']), ('d/dmu', over))
            inside(got[:, S:], r['gs'], ref64.bound(G.C_NLL, r['gs_c'], r['gs_x']), ('d/dpre', over))
            inside(rows.double().sum(1), -0.5 * r['term'].sum(1), G.rows_bound(G.C_NLL, r['term_c'], r['term_x'], S),
                   ('rows', over))


@pytest.mark.parametrize('a_kc,b_kc', LAYOUTS)
def test_poison_ragged_n_split(K, dev, a_kc, b_kc):
    """the chip-filling plain product whose last column of 128x256 tiles is narrow runs as two launches (the shape of
    tests/test_gpu_kernels.py::test_gemm_ragged_last_tile_column_runs_as_two_launches): both parts under poison"""
    M, N, Kd = 4096, 32 * 256 + 64, 64
    A, B = G.random_operands(M, N, Kd, seed=8)
    e = G.epilogue_case('plain-ab', M, N)
    want, bound, _ = G.expected(A, B, e)
    got = run_gemm(K, dev, A, B, a_kc, b_kc, 'A', True, e=e)
    inside(got, want, bound, 'split')
    K.gemm_set_option(6, -1)
    try:
        one = run_gemm(K, dev, A, B, a_kc, b_kc, 'A', True, e=e)
    finally:
        K.gemm_set_option(6, 0)
    inside(one, want, bound, 'one launch')
    assert torch.equal(got[:, :32 * 256], one[:, :32 * 256])          # the full tiles: the same kernel, the same tiles


# ------------------------------------------------------------------------------------------------ 4. non-finite operands
@pytest.mark.parametrize('cls,Kd', [('A', 200), ('D', 202)])
@pytest.mark.parametrize('route,a_kc,b_kc', ROUTE_LAYOUTS)
def test_non_finite_operands_poison_exactly_what_they_feed(K, dev, route, a_kc, b_kc, cls, Kd):
    """a NaN, a +inf and a -inf in the first and last row of Aop, the first and last column of Bop (what the edge tiles clamp
    to) and one interior element; otherwise randn (no zeros).  Class D: dense rows with K % 4 == 2 and the over-read word --
    the chunk that straddles K holds the start of the next row, which is non-finite for three of the five."""
    M, N = 150, 300
    A, B, want = G.poisoned_operands(M, N, Kd)
    with routed(K, route):
        got = run_gemm(K, dev, A, B, a_kc, b_kc, cls, True)
    assert torch.equal(~torch.isfinite(got), want)


@pytest.mark.parametrize('route', DW_ROUTES)
def test_non_finite_dy_poisons_exactly_its_bias_gradient(K, dev, route):
    M, N, Kd = 150, 128, 200
    dy, x = (t.clone() for t in G.random_operands(M, N, Kd, seed=3))
    bad = {0: (3, NAN), M - 1: (Kd - 1, float('inf')), 77: (0, float('-inf'))}
    for m, (k, v) in bad.items():
        dy[m, k] = v
    with routed(K, route):
        for cls in ('A', 'D'):
            f = Frame(dev, cls)
            dW, db = f.out((M, N)), f.out((M,))
            K.linear_bwd_weight(dW, f.inp(dy.t()), f.inp(x), dbias=db, overread=True)
            f.verify()
            assert sorted(torch.nonzero(~torch.isfinite(db.cpu())).flatten().tolist()) == sorted(bad), cls
            want = torch.zeros(M, N, dtype=torch.bool)
            want[sorted(bad), :] = True
            assert torch.equal(~torch.isfinite(dW.cpu()), want), cls


# ------------------------------------------------------------------------------------------------ 5. tile maps
@pytest.mark.parametrize('tmap', G.MAPS)
@pytest.mark.parametrize('tiling', tilings(2, 17, 1, 3, 40))
def test_tile_maps_cover_every_tile_once(K, dev, tiling, tmap):
    """dv_gemm_tune.opt[0] = 0 (linear), 1 (XCD chunk-major), 3 / 16 / 32 (bands) on grids ragged in both directions, tile
    counts no multiple of 8 or of a band height, wider than tall and taller than wide, at least 16 workgroups.  K = 8 on
    small integers: exact.  C starts as NaN: a tile never computed stays NaN, one written to the wrong place leaves wrong
    integers, one computed twice is harmless."""
    with routed(K, (tiling, {0: tmap})):
        for grid in G.MAP_GRIDS[tiling]:
            M, N = G.map_shape(tiling, grid)
            A, B = G.integer_operands(M, N, 8)
            want = A @ B
            for a_kc, b_kc in LAYOUTS:
                Cm = torch.full((M, N + 3), NAN, device=dev)[:, :N]
                K.gemm(Cm, store(A, a_kc, dev), store(B.t(), b_kc, dev), a_kc, b_kc, overread=True)
                assert torch.equal(Cm.cpu(), want), (grid, a_kc, b_kc)


# ------------------------------------------------------------------------------------------------ 6. reproducibility
@pytest.mark.parametrize('route,a_kc,b_kc', ROUTE_LAYOUTS)
def test_same_descriptor_twice_same_bits(K, dev, route, a_kc, b_kc):
    cls, M, N, Kd, over = G.BASE
    A, B = G.random_operands(M, N, Kd)
    f = Frame(dev, cls)
    Ad, Bd = f.inp(G.stored(A, a_kc)), f.inp(G.stored(B.t(), b_kc))
    C1, C2 = f.out((M, N)), f.out((M, N))
    with routed(K, route):
        K.gemm(C1, Ad, Bd, a_kc, b_kc, overread=over)
        K.gemm(C2, Ad, Bd, a_kc, b_kc, overread=over)
    f.verify()
    assert torch.equal(C1, C2) and bool(torch.isfinite(C1).all())


# ------------------------------------------------------------------------------------------------ 7. beta == 0
def rnd(dev, *shape, seed=0, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed + sum(shape))) * scale).to(dev)


def _colsum(K, dev, new):
    out = new(77)
    K.colsum(out, rnd(dev, 301, 80, seed=1)[:, :77], beta=0.0)
    return [out]


def _wn_bwd(K, dev, new):
    N, Kd = 45, 978
    W, g = rnd(dev, N, Kd, seed=3, scale=0.05), rnd(dev, N, seed=4).abs() + 0.5
    sc, nm = torch.empty(N, device=dev), torch.empty(N, device=dev)
    K.wn_scale(sc, nm, W, g)
    dW, dg = new(N, Kd), new(N)
    K.wn_bwd(dW, dg, rnd(dev, N, Kd, seed=5), W, g, nm, beta=0.0)
    return [dW, dg]


def _reparam_bwd(K, dev, new):
    n, reps, Z = 11, 3, 100
    Q = rnd(dev, n, 2 * Z, seed=1, scale=0.5)
    dQ = new(n, 2 * Z)
    K.reparam_bwd(dQ[:, :Z], dQ[:, Z:], rnd(dev, n * reps, Z, seed=4), rnd(dev, n * reps, Z, seed=2), Q[:, Z:], reps=reps, beta=0.0)
    return [dQ]


def _reparam_bwd_seg(K, dev, new):
    nq, Z, R_ = 23, 100, 90
    sd = rnd(dev, nq + 5, 2 * Z, seed=1, scale=0.5)[:, Z:]
    sizes = torch.randint(1, 5, (nq,), generator=torch.Generator().manual_seed(5))
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)]).to(torch.int32).to(dev)
    rows = torch.randint(0, R_, (int(ptr[-1]),), generator=torch.Generator().manual_seed(6)).to(torch.int32).to(dev)
    dq = new(nq, 2 * Z)
    K.reparam_bwd_seg(dq[:, :Z], dq[:, Z:], rnd(dev, R_, Z, seed=2), rnd(dev, R_, Z, seed=3), sd, ptr, rows, beta=0.0)
    return [dq]


def _kl_rows_bwd(K, dev, new):
    n, reps, Z, nq = 9, 2, 100, 12
    Rr = n * reps
    Q, P = rnd(dev, nq, 2 * Z, seed=1, scale=0.7), rnd(dev, Rr + 3, 2 * Z, seed=2, scale=0.7)
    g = torch.Generator().manual_seed(3)
    qidx = torch.randperm(nq, generator=g)[:n].to(torch.int32).to(dev)
    pidx = torch.randperm(Rr + 3, generator=g)[:Rr].to(torch.int32).to(dev)
    kw = dict(mode=0, qidx=qidx, reps=reps, free_bits=True, kl_min=float(Z) * 0.3, prior=(0.1, 0.2),
              mu_p=P[:, :Z], sd_p=P[:, Z:], pidx=pidx)
    out, raw = torch.empty(Rr, device=dev), torch.empty(Rr, device=dev)
    K.kl_rows_fwd(out, raw, Q[:, :Z], Q[:, Z:], **kw)
    dq, dp = new(Rr, 2 * Z), new(Rr, 2 * Z)
    K.kl_rows_bwd(dq[:, :Z], dq[:, Z:], dp[:, :Z], dp[:, Z:], rnd(dev, Rr, seed=3), raw, Q[:, :Z], Q[:, Z:], beta=0.0, **kw)
    return [dq, dp]


def _nll_rows_bwd(K, dev, new):
    M, nx, X = 23, 9, 978
    x, P = rnd(dev, nx, X, seed=1), rnd(dev, M, 2 * X, seed=2)
    mu, sd = P[:, :X], P[:, X:]
    sd.copy_(torch.nn.functional.softplus(sd) + 1e-3)
    xidx = torch.randint(0, nx, (M,), generator=torch.Generator().manual_seed(4)).to(torch.int32).to(dev)
    D, dx = new(M, 2 * X), new(M, X)
    K.nll_rows_bwd(D[:, :X], D[:, X:], rnd(dev, M, seed=3), x, mu, sd, mode=1, xidx=xidx, sd_act='softplus', sd_shift=1e-3,
                   dx=dx, beta=0.0)
    return [D, dx]


def _probs(K, dev, M, Y):
    p = torch.empty(M, Y, device=dev)
    K.softmax_clamp_fwd(p, rnd(dev, M, Y, seed=1, scale=4.0), False)
    return p


def _softmax_clamp_bwd(K, dev, new):
    M, Y = 301, 3
    dl = new(M, Y)
    K.softmax_clamp_bwd(dl, rnd(dev, M, Y, seed=2), _probs(K, dev, M, Y), False, beta=0.0)
    return [dl]


def _cat_terms_bwd(K, dev, new):
    M, Y = 301, 3
    labels = torch.randint(0, Y, (M,), generator=torch.Generator().manual_seed(2)).to(torch.int32).to(dev)
    prior = torch.softmax(rnd(dev, M, Y, seed=4), -1)
    dp = new(M, Y)
    K.cat_terms_bwd(dp, _probs(K, dev, M, Y), labels=labels, prior=prior, c_logp=rnd(dev, M, seed=5), g_kl=rnd(dev, M, Y, seed=6),
                    c_ent=rnd(dev, M, seed=7), beta=0.0)
    return [dp]


def _smalln_bwd_data(K, dev, new):
    M, K1, K2, Y = 301, 100, 100, 2
    W, g = rnd(dev, Y, K1 + K2, seed=3, scale=0.3), rnd(dev, M, Y, seed=5)
    d1, d2 = new(M, K1), new(M, K2)
    K.smalln_bwd_data([(d1, 0, 1.0, 0.0, K1, -1.0), (d2, K1, 1.0, 0.0)], g, _probs(K, dev, M, Y), W)
    return [d1, d2]


def _smalln_bwd_weight(K, dev, new):
    M, K1, K2, Y = 301, 100, 100, 2
    dW, db = new(Y, K1 + K2), new(Y)
    K.smalln_bwd_weight(dW, db, rnd(dev, M, Y, seed=5), _probs(K, dev, M, Y), rnd(dev, M, K1, seed=1), rnd(dev, M, K2, seed=2),
                        beta=0.0)
    return [dW, db]


def _rows_segment_sum(K, dev, new):
    ns, W = 30, 13
    g = torch.Generator().manual_seed(1)
    sizes = torch.randint(0, 4, (7,), generator=g)
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)]).to(torch.int32).to(dev)
    T = int(ptr[-1])
    rows = torch.randint(0, ns, (T,), generator=g).to(torch.int32).to(dev)
    didx = torch.randperm(7, generator=g).to(torch.int32).to(dev)
    dst = new(7, W)
    K.rows_segment_sum(dst, rnd(dev, ns, W + 2, seed=1)[:, :W], seg_ptr=ptr, seg_rows=rows, w=rnd(dev, T, seed=3), dst_idx=didx,
                       beta=0.0)
    return [dst]


def _weighted_sum(K, dev, new):
    o = new(1)
    K.weighted_sum(o, rnd(dev, 1000, seed=6), rnd(dev, 1000, seed=7), scale=0.5, beta=0.0)
    return [o]


def _axpby(K, dev, new):
    y = new(1000)
    K.axpby(y, rnd(dev, 1000, seed=6), a=-2.0, b=0.0)
    return [y]


BETA_CALLS = dict(colsum=_colsum, wn_bwd=_wn_bwd, reparam_bwd=_reparam_bwd, reparam_bwd_seg=_reparam_bwd_seg,
                  kl_rows_bwd=_kl_rows_bwd, nll_rows_bwd=_nll_rows_bwd, softmax_clamp_bwd=_softmax_clamp_bwd,
                  cat_terms_bwd=_cat_terms_bwd, smalln_bwd_data=_smalln_bwd_data, smalln_bwd_weight=_smalln_bwd_weight,
                  rows_segment_sum=_rows_segment_sum, weighted_sum=_weighted_sum, axpby=_axpby)


@pytest.mark.parametrize('name', sorted(BETA_CALLS))
def test_beta_zero_never_reads_the_output(K, dev, name):
    """every launcher with a ``beta`` (or ``b``), at the small shapes of its own test: outputs pre-filled with NaN and
    beta = 0 -- the result is finite and bit-equal to the same call on zero-filled outputs (0 * NaN would not be)"""
    res = {}
    for fill in (NAN, 0.0):
        res[fill == 0.0] = BETA_CALLS[name](K, dev, lambda *shape: torch.full(shape, fill, device=dev))
        torch.cuda.synchronize()
    for on_nan, on_zero in zip(res[False], res[True]):
        assert bool(torch.isfinite(on_nan).all())
        assert torch.equal(on_nan, on_zero)
