"""GPU: the deeper LDS-DMA rings of the latency-bound 32 x 32 x 64 launches (drvae_amd/csrc/ring_route.h) -- forced four slots
and forced three against the ring of two (dv_gemm_tune.opt[7] = 2 / 3 against 4) on the smallest shapes where a ring can go
wrong: K below, at and above a ring's worth of K tiles, with a ragged last tile and no multiple of 64; M and N of one element,
one short of, one past and a bit past a tile; all three layouts; the fused epilogues; the ones column of the bias gradient; the
fused pair and the sample-mode heads launch.

The ring's depth changes neither which wave owns which k nor the order of any sum, so every stored output has to agree BIT FOR
BIT between the depths; on top every output lies inside the fp32 GEMM contract of tests/gemm_contract.py against float64, the
guard bands around every operand and output stay untouched, and a second launch stores the same bits."""
import functools

import numpy as np
import pytest
import torch

from tests import gemm_contract as G
from tests import ref64
from tests.gemm_contract import LAYOUTS, U, Frame, routed

pytestmark = pytest.mark.gpu

KS = (4, 60, 64, 68, 128, 192, 256, 260, 324)       # K tiles of 64: 1 .. 6 -- below, at and above three and four slots
MN = (1, 31, 33, 40)
OPT_OF_DEPTH = {2: 4, 3: 3, 4: 2}                    # ring depth -> dv_gemm_tune.opt[7]
DEEP = (3, 4)


@pytest.fixture(scope='module')
def K(dev):
    import drvae_amd.kernels as K
    from drvae_amd import _lib
    _lib.load()
    return K


def at_every_depth(K, call):
    """``call()`` -> list of host outputs (it verifies its own guard bands), run twice at each depth on the 32 x 32 K-split
    tiling: the two launches of a depth and the depths among each other agree in every bit.  Returns the ring of two's"""
    res = {}
    for d in (2,) + DEEP:
        with routed(K, (2, {7: OPT_OF_DEPTH[d]})):
            first, second = call(), call()
        for i, (a, b) in enumerate(zip(first, second)):
            assert torch.equal(G.bits(a), G.bits(b)), 'depth %d, output %d: two launches differ' % (d, i)
        res[d] = first
    for d in DEEP:
        for i, (a, b) in enumerate(zip(res[2], res[d])):
            diff = int((G.bits(a) != G.bits(b)).sum())
            assert diff == 0, 'output %d: %d elements differ between two and %d ring slots' % (i, diff, d)
    return res[2]


def inside(got, want, bound, what):
    assert bool(torch.isfinite(got).all()), what
    worst = G.worst_excess(got, want, bound)
    print('ring depth %s: max err / bound %.3f' % (what, worst))
    assert worst <= 1.0, (what, worst)


# ------------------------------------------------------------------------------------------------ dv_gemm
@functools.lru_cache(maxsize=None)
def fwd_heads_case(M, N):
    g = torch.Generator().manual_seed(31 + 7 * M + N)
    return dict(bias=torch.randn(N, generator=g), h=(N + 1) // 2)


def fwd_elu_expected(A, B, e):
    """y = [elu(A B + bias) | A B + bias]: a bias, ELU on the first head and a split.  pre = acc + bias rounds once on top of
    the accumulator's bound (tests/gemm_contract.py); ELU is 1-Lipschitz and costs the rule of tests/ref64.py with C = 8 and
    its hardware-exp term"""
    c64, dacc = G.acc_bound(A, B)
    h = e['h']
    pre = c64 + e['bias'].double()
    dpre = dacc + U * (2 * c64.abs() + pre.abs())
    y = torch.cat([ref64.act('elu', pre[:, :h]), pre[:, h:]], 1)
    extra = torch.cat([ref64.act_exp_extra('elu', pre[:, :h]), torch.zeros_like(pre[:, h:])], 1)
    return y, 1.01 * dpre + ref64.bound(8, y.abs(), extra) + U * y.abs()


@pytest.mark.parametrize('a_kc,b_kc', LAYOUTS, ids=lambda v: str(int(v)))
@pytest.mark.parametrize('Kd', KS)
def test_products_agree_between_the_depths(K, dev, Kd, a_kc, b_kc):
    """``gemm`` in every layout: the forward epilogue with a bias, ELU and a head split; the activation backward with
    ``yref``; the plain product accumulating into C (alpha = -0.37, beta = 1)"""
    for M in MN:
        for N in MN:
            A, B = G.random_operands(M, N, Kd, seed=21)
            for name in ('fwd-elu', 'bwd', 'plain-ab'):
                if name == 'fwd-elu':
                    e = fwd_heads_case(M, N)
                    want, bound = fwd_elu_expected(A, B, e)
                else:
                    e = G.epilogue_case(name, M, N)
                    want, bound, _ = G.expected(A, B, e)

                def call():
                    f = Frame(dev, 'A')
                    Ad, Bd = f.inp(G.stored(A, a_kc)), f.inp(G.stored(B.t(), b_kc))
                    if name == 'fwd-elu':
                        kw = dict(epi=K.EPI_FWD, bias=f.inp(e['bias']), split=e['h'], act0='elu', act1='identity')
                        Cm = f.out((M, N))
                    else:
                        kw = G.epilogue_kwargs(K, e, f.inp)
                        Cm = f.out(e['C0'] if e['beta'] else (M, N))
                    K.gemm(Cm, Ad, Bd, a_kc, b_kc, overread=True, **kw)
                    f.verify()
                    return [Cm.cpu()]
                got, = at_every_depth(K, call)
                inside(got, want, bound, '%s %dx%dx%d (%d%d)' % (name, M, N, Kd, a_kc, b_kc))


@pytest.mark.parametrize('N', [31, 33, 32, 64])
def test_bias_gradient_on_the_ones_column(K, dev, N):
    """``linear_bwd_weight`` with ``dbias`` (dy^T x, four waves): the ones column's chunk is written into every ring slot up
    front -- N % 4 != 0 (it shares a tile with the matrix's last columns) and N % 32 == 0 (it needs a tile of its own)"""
    M = 40
    for Kd in KS:
        dy, x = G.random_operands(M, N, Kd, seed=23)          # Aop = dy^T: (M, K); Bop = x: (K, N)
        want, bound, _ = G.expected(dy, x, G.epilogue_case('plain', M, N))
        db64, dbb = G.colsum_bound(dy.t())

        def call():
            f = Frame(dev, 'A')
            dpre, xd = f.inp(dy.t()), f.inp(x)
            dW, db = f.out((M, N)), f.out((M,))
            K.linear_bwd_weight(dW, dpre, xd, dbias=db, overread=True)
            f.verify()
            return [dW.cpu(), db.cpu()]
        dW, db = at_every_depth(K, call)
        inside(dW, want, bound, 'dW %dx%dx%d' % (M, N, Kd))
        inside(db, db64, dbb + U * db64.abs(), 'db %dx%dx%d' % (M, N, Kd))


# ------------------------------------------------------------------------------------------------ dv_gemm_pair
# (rows of the batch = reduction of dW, output width = reduction of dX, input width)
PAIRS = ((324, 68, 33), (60, 260, 40), (256, 192, 31), (4, 64, 1), (128, 324, 40))


@pytest.mark.parametrize('batch,Nout,Kin', PAIRS)
def test_fused_pair_agrees_between_the_depths(K, dev, batch, Nout, Kin):
    """``linear_bwd_pair``, the fused dW || dX launch: dW and db pre-filled with NaN, dx accumulating (beta_x = 1) through the
    activation backward with ``yref``"""
    dy, x = G.random_operands(Nout, Kin, batch, seed=25)                # dW = dy x: (Nout, batch) (batch, Kin)
    W = G.random_operands(batch, Kin, Nout, seed=26)[1]                 # dx = dy^T W: (batch, Nout) (Nout, Kin)
    wW, bW, _ = G.expected(dy, x, G.epilogue_case('plain', Nout, Kin))
    db64, dbb = G.colsum_bound(dy.t())
    e = dict(G.epilogue_case('bwd-ab', batch, Kin), h=Kin)
    wX, bX, _ = G.expected(dy.t(), W, e)

    def call():
        f = Frame(dev, 'A')
        dpre, xd, Wd, yref = f.inp(dy.t()), f.inp(x), f.inp(W), f.inp(e['yref'])
        dW, db, dx = f.out((Nout, Kin)), f.out((Nout,)), f.out(e['C0'])
        K.linear_bwd_pair(dW, db, dx, dpre, xd, Wd, alpha=e['alpha'], beta_x=1.0, yref=yref, act='elu', overread=True)
        f.verify()
        return [dW.cpu(), db.cpu(), dx.cpu()]
    dW, db, dx = at_every_depth(K, call)
    inside(dW, wW, bW, 'pair dW')
    inside(db, db64, dbb + U * db64.abs(), 'pair db')
    inside(dx, wX, bX, 'pair dx')


# ------------------------------------------------------------------------------------------------ dv_gemm_heads
@functools.lru_cache(maxsize=None)
def heads_case(Kd):
    """33 rows, two heads of 20 columns (ragged against the 16-wide half tiles); 20 source rows fan out to 0 .. 3 sample rows
    each through a CSR list; ``out2 = z - sub`` and a scattered copy (out3).  References as tests/test_gpu_gemm_contract.py"""
    M, S, n_src = 33, 20, 20
    g = torch.Generator().manual_seed(41 + Kd)
    x, Wt = G.random_operands(M, 2 * S, Kd, seed=27)
    e = dict(kind='fwd', alpha=1.0, beta=0.0, h=S, C0=None, act1='identity', shift1=-2.0,
             scale=torch.randn(2 * S, generator=g).abs() + 0.5, bias=torch.randn(2 * S, generator=g),
             resid=torch.randn(M, S, generator=g))
    cnt = [(i % 3) + (1 if i % 5 == 0 else 0) for i in range(n_src)]
    ptr = np.concatenate([[0], np.cumsum(cnt)])
    R_ = int(ptr[-1])
    rows = torch.randperm(R_, generator=g)
    eps, sub = torch.randn(R_, S, generator=g), torch.randn(R_, S, generator=g)
    idx3 = torch.tensor([(i // 2 if i % 2 == 0 else -1) for i in range(R_)])
    want, bound, _ = G.expected(x, Wt, e)
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
    return dict(M=M, S=S, n_src=n_src, x=x, W=Wt.t().contiguous(), e=e, ptr=torch.tensor(ptr, dtype=torch.int32),
                rows=rows.to(torch.int32), eps=eps, sub=sub, idx3=idx3.to(torch.int32), want=want, bound=bound, z=z, zb=zb,
                z2=z2, z2b=zb + U * z2.abs(), n3=int(sel3.sum()), sel3=sel3, order3=idx3[sel3])


@pytest.mark.parametrize('Kd', KS)
def test_sample_heads_agree_between_the_depths(K, dev, Kd):
    """``linear_heads`` / SAMPLE on the eight-wave kernel: (mu | logvar), the samples, ``out2`` and ``out3``"""
    c = heads_case(Kd)
    M, S, e = c['M'], c['S'], c['e']
    R_ = c['eps'].shape[0]

    def call():
        f = Frame(dev, 'A')
        x, W, eps, sub = f.inp(c['x']), f.inp(c['W']), f.inp(c['eps']), f.inp(c['sub'])
        kw = G.epilogue_kwargs(K, e, f.inp)
        q, z, z2, o3 = f.out((M, 2 * S)), f.out((R_, S)), f.out((R_, S)), f.out((c['n3'], S))
        K.linear_heads(q, x, W, kw['bias'], split=S, scale=kw['scale'], act0='identity', act1='identity', shift1=-2.0,
                       resid=kw['resid'], resid_cols=S, overread=True,
                       sample=dict(eps=eps, out=z, n_src=c['n_src'], seg_ptr=c['ptr'].to(dev), seg_rows=c['rows'].to(dev),
                                   sub=sub, out2=z2, out3=o3, out3_idx=c['idx3'].to(dev)))
        f.verify()
        return [q.cpu(), z.cpu(), z2.cpu(), o3.cpu()]
    q, z, z2, o3 = at_every_depth(K, call)
    inside(q, c['want'], c['bound'], 'heads mu | logvar K=%d' % Kd)
    inside(z, c['z'], c['zb'], 'heads z K=%d' % Kd)
    inside(z2, c['z2'], c['z2b'], 'heads z - sub K=%d' % Kd)
    inside(o3[c['order3']], c['z'][c['sel3']], c['zb'][c['sel3']], 'heads out3 K=%d' % Kd)
