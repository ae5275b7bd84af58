"""The sample-mode paired-heads launch on 16 x (8 + 8) tiles (``gemm_heads16_kernel``, dv_gemm_tune.opt[4] = 4) against the
32-row launch it replaces (opt[4] = 5) on the same inputs: every wave owns the k values it owns there, feeds them to the matrix
core in the same order and the eight partials are summed in the same order, so the stored heads and every sample output
carry the SAME BITS; both stay inside the family's element-wise bound against float64 (tests/gemm_contract.py), and neither
writes outside its outputs.

Shapes: the smallest that reach every edge of the 16-row tile -- M = 17 / 33 (ragged last row tile, two and three row
tiles), split = 9 / 16 (ragged and exact 8-wide column tile), K = 64 / 68 / 132 (exact and ragged 128-deep K tile, one and
two ring tiles) and K = 66 (K % 4 != 0: no LDS-DMA ring, the forced launch has to fall back to the register-staged 32-row
kernel and still agree); n_src < M; segments of 0, 1, 3, 4 and 6 sample rows (four slots per element: 6 runs the strided
remainder); 0, 1 and 2 out4 rows per sample; with and without out2 / out3 / out4."""
import functools

import numpy as np
import pytest
import torch

from tests import gemm_contract as G
from tests.gemm_contract import U, Frame, bits, routed

pytestmark = pytest.mark.gpu

T16, T32 = (0, {4: 4}), (0, {4: 5})
SHAPES = [(M, S, Kd) for M in (17, 33) for S in (9, 16) for Kd in (64, 68, 132, 66)]


@pytest.fixture(scope='module')
def K(dev):
    import drvae_amd.kernels as K
    from drvae_amd import _lib
    _lib.load()
    return K


def inside(got, want, bound, what):
    x = G.worst_excess(got, want, bound)
    print('%s: worst |got - want| / bound = %.3f' % (what, x))
    assert x <= 1.0, (what, x)


@functools.lru_cache(maxsize=None)
def case(M, S, Kd):
    """as ``heads_sample_case`` of tests/test_gpu_gemm_contract.py, at (M, S, Kd): float64 heads and samples with their bounds"""
    n_src = M - 3
    g = torch.Generator().manual_seed(17 + M + 3 * S + 5 * Kd)
    x, Wt = G.random_operands(M, 2 * S, Kd, seed=9)
    e = dict(kind='fwd', alpha=1.0, beta=0.0, h=S, C0=None, act1='identity', shift1=-2.0,
             scale=torch.randn(2 * S, generator=g).abs() + 0.5, bias=torch.randn(2 * S, generator=g),
             resid=torch.randn(M, S, generator=g))
    cnt = [(0, 1, 3, 4, 6)[i % 5] for i in range(n_src)]
    ptr = np.concatenate([[0], np.cumsum(cnt)])
    R_ = int(ptr[-1])
    rows = torch.randperm(R_, generator=g)
    eps, sub = torch.randn(R_, S, generator=g), torch.randn(R_, S, generator=g)
    idx3 = torch.tensor([(i // 2 if i % 2 == 0 else -1) for i in range(R_)])
    ptr4 = np.concatenate([[0], np.cumsum([(i % 3) for i in range(R_)])])
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
    rep4 = torch.repeat_interleave(torch.arange(R_), torch.tensor(np.diff(ptr4)))
    return dict(n_src=n_src, x=x, W=Wt.t().contiguous(), e=e, ptr=torch.tensor(ptr, dtype=torch.int32),
                rows=rows.to(torch.int32), eps=eps, sub=sub, idx3=idx3.to(torch.int32), ptr4=torch.tensor(ptr4, dtype=torch.int32),
                want=want, bound=bound, z=z, zb=zb, z2=z2, z2b=zb + U * z2.abs(), n3=int(sel3.sum()), sel3=sel3,
                order3=idx3[sel3], rep4=rep4, R=R_)


def launch(K, dev, c, M, S, route, riders):
    """one launch on ``route`` in sentinel frames: (q, z, z2, o3, o4) on the host, the memory contract verified"""
    with routed(K, route):
        f = Frame(dev, 'A')
        x, W, eps, sub = f.inp(c['x']), f.inp(c['W']), f.inp(c['eps']), f.inp(c['sub'])
        kw = G.epilogue_kwargs(K, c['e'], f.inp)
        q, z = f.out((M, 2 * S)), f.out((c['R'], S))
        sample = dict(eps=eps, out=z, n_src=c['n_src'], seg_ptr=c['ptr'].to(dev), seg_rows=c['rows'].to(dev))
        z2 = o3 = o4 = None
        if riders:
            z2, o3, o4 = f.out((c['R'], S)), f.out((c['n3'], S)), f.out((int(c['ptr4'][-1]), S))
            sample.update(sub=sub, out2=z2, out3=o3, out3_idx=c['idx3'].to(dev), out4=o4, out4_ptr=c['ptr4'].to(dev))
        K.linear_heads(q, x, W, kw['bias'], split=S, scale=kw['scale'], act0='identity', act1='identity', shift1=-2.0,
                       resid=kw['resid'], resid_cols=S, overread=True, sample=sample)
        f.verify()
        return [None if t is None else t.cpu() for t in (q, z, z2, o3, o4)]


@pytest.mark.parametrize('riders', [True, False], ids=['riders', 'plain'])
@pytest.mark.parametrize('M,S,Kd', SHAPES, ids=lambda v: str(v))
def test_heads16_carries_the_bits_of_the_32_row_launch(K, dev, M, S, Kd, riders):
    c = case(M, S, Kd)
    new, again, old = (launch(K, dev, c, M, S, r, riders) for r in (T16, T16, T32))
    names = ('mu | logvar', 'z', 'z - sub', 'out3', 'out4')
    for n, a, b, o in zip(names, new, again, old):
        if a is None:
            continue
        assert torch.equal(bits(a), bits(b)), (n, 'two launches differ')
        diff = int((bits(a) != bits(o)).sum())
        print('%s: %d of %d elements differ from the 32-row launch' % (n, diff, a.numel()))
        assert diff == 0, (n, diff)
    for tag, (q, z, z2, o3, o4) in (('16-row', new), ('32-row', old)):
        inside(q, c['want'], c['bound'], (tag, 'mu | logvar'))
        # (sample rows of sources with an empty segment do not exist: every row of z belongs to exactly one source)
        inside(z, c['z'], c['zb'], (tag, 'z'))
        if riders:
            inside(z2, c['z2'], c['z2b'], (tag, 'z - sub'))
            inside(o3[c['order3']], c['z'][c['sel3']], c['zb'][c['sel3']], (tag, 'out3'))
            inside(o4, c['z'][c['rep4']], c['zb'][c['rep4']], (tag, 'out4'))


def test_heads16_without_a_segment_table(K, dev):
    """no CSR list: source row m owns sample row m (one slot of four works)"""
    M, S, Kd = 33, 9, 68
    c = case(M, S, Kd)
    outs = []
    for route in (T16, T32):
        with routed(K, route):
            f = Frame(dev, 'A')
            x, W, eps = f.inp(c['x']), f.inp(c['W']), f.inp(c['eps'][:c['n_src']])
            kw = G.epilogue_kwargs(K, c['e'], f.inp)
            q, z = f.out((M, 2 * S)), f.out((c['n_src'], S))
            K.linear_heads(q, x, W, kw['bias'], split=S, scale=kw['scale'], act0='identity', act1='identity', shift1=-2.0,
                           resid=kw['resid'], resid_cols=S, overread=True, sample=dict(eps=eps, out=z, n_src=c['n_src']))
            f.verify()
            outs.append((q.cpu(), z.cpu()))
    assert torch.equal(bits(outs[0][0]), bits(outs[1][0])) and torch.equal(bits(outs[0][1]), bits(outs[1][1]))
    inside(outs[0][0], c['want'], c['bound'], 'mu | logvar')
    assert not torch.isnan(outs[0][1]).any()
