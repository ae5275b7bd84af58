"""Float64 references of the MMD, BatchNorm and dropout row kernels (``dv_mmd_mix_*``, ``dv_mmd_identity_*``,
``dv_mmd_rff_*``, ``dv_bn_fwd`` / ``dv_bn_bwd``, ``dv_mask_scale``), their error bounds, the cases and the case runners the
device tests (tests/test_gpu_mmd_rows.py, tests/test_gpu_bn_rows.py) and the CPU file that holds the references themselves
(tests/test_mmd_bn_ref_cpu.py) share.

Independent of ``tests/kernel_ref.py``; follows ``tests/ref64.py``: values in float64 on the exact fp32 inputs a launch
received, derivatives in closed form in float64 (the CPU file holds them to float64 autograd), and ref64's rule

    |got - ref| <= C * U * sum |components| + 2 * U * extra + 2**-126,      U = 2**-24, C <= ref64.C_MAX

componentwise, never relative to a tensor's maximum.  The floor 2**-126: an fp32 result may flush where float64 still
holds 1e-40.  Sums follow each kernel's own order: a column summed by ``groups`` threads and a pairwise join costs
``col_sum_bound``; the 256-stride row sums ``ref64.row_sum_bound``.

One place where the algebra needs the second-order term that a first-order statement leaves out: a sum of squares of a
perturbed difference, (d + e)^2 - d^2 = 2 d e + e^2, carries the e^2.  Nothing else is widened."""
import math

import torch

from tests import ref64
from tests.gemm_contract import GUARD, SENTINEL
from tests.ref64 import U, bound, f32, f64

FLOOR = 2.0 ** -126
NAN = float('nan')
C_TRIG = 4          # cosf / sinf: within 2 ulp of a result of magnitude <= 1, i.e. an absolute 4 U (component 1)
C_W = 2             # W = (coef * gout) * dk: one rounding per product
DEFAULT_BW = tuple(1. / (2 * (x ** 2)) for x in (1., 2., 5., 8., 10.))


def c_mix(nb):
    """C of a mixture element: an fma and a square (poly) or the exp's own ulp and its argument's product (rbf), nb - 1
    additions, 1/nb as fp32 and the product with it, one to spare: nb + 4 <= 12"""
    return nb + 4


def col_sum_bound(terms, M, groups):
    """summation part of the bound of a column sum of M terms (rows along dim 0) accumulated by ``groups`` serial chains
    that are joined pairwise: (ceil(M / groups) + 3) U sum |terms|"""
    return (math.ceil(M / groups) + 3) * U * f64(terms).abs().sum(0)


# ================================================================================================ the references
def mix_elements(G, kind, gammas, sa=None, sb=None, e_G=None, e_sa=None, e_sb=None):
    """the kernel mixture per element of the Gram matrix ``G`` (taken as given fp32, like the squared norms ``sa`` /
    ``sb``: vectors): k, dk (= dk/dG for poly, dk/d(d2) for rbf), their bounds, and the components of k and dk.
    Whole operations pass the exact float64 products and what the Gram launches may be off by (``e_G``, ``e_sa``,
    ``e_sb``).  rbf's condition term is written as k_b expm1(gamma e_d2), the exact form of gamma e_d2 k_b: the two
    differ in the second order, which counts once a translated row set makes gamma e_d2 a few per cent."""
    G = f64(G)
    gam = [f32(g) for g in gammas]
    nb = len(gam)
    C = c_mix(nb)
    zero = torch.zeros_like(G)
    e_G = zero if e_G is None else f64(e_G)
    k, dk, kc, dkc, kx, dkx, kcond, dkcond = (torch.zeros_like(G) for _ in range(8))
    if kind == 'poly':
        for g in gam:
            t = g * G + 1
            k, dk = k + t * t, dk + 2 * g * t
            tc = (g * G).abs() + 1
            kc, dkc = kc + tc * tc, dkc + 2 * abs(g) * tc
            kcond, dkcond = kcond + 2 * abs(g) * tc * e_G + g * g * e_G * e_G, dkcond + 2 * g * g * e_G
    else:
        sa, sb = f64(sa).reshape(-1, 1), f64(sb).reshape(1, -1)
        d2 = torch.clamp(sa + sb - 2 * G, min=0.0)
        e_d2 = 3 * U * (sa.abs() + sb.abs() + 2 * G.abs()) + 2 * e_G   # also a clamp decided differently in fp32 and float64
        if e_sa is not None:
            e_d2 = e_d2 + f64(e_sa).reshape(-1, 1) + f64(e_sb).reshape(1, -1)
        for g in gam:
            kb = torch.exp(-g * d2)
            k, dk = k + kb, dk - g * kb
            kc, dkc = kc + kb, dkc + abs(g) * kb
            kcond, dkcond = kcond + torch.expm1(g * e_d2) * kb, dkcond + g * torch.expm1(g * e_d2) * kb
            kx, dkx = kx + (g * d2).abs() * kb, dkx + abs(g) * (g * d2).abs() * kb      # the hardware exp sees a = -g d2
    k, dk, kc, dkc, kx, dkx, kcond, dkcond = (t / nb for t in (k, dk, kc, dkc, kx, dkx, kcond, dkcond))
    return dict(k=k, dk=dk, k_c=kc, dk_c=dkc, k_b=bound(C, kc, kx) + kcond + FLOOR, dk_b=bound(C, dkc, dkx) + dkcond + FLOOR)


def mix_fwd(G, kind, gammas, sa=None, sb=None):
    """part[i] = sum_j k_ij: the elements' bounds summed plus the row sum's"""
    e = mix_elements(G, kind, gammas, sa, sb)
    N = e['k'].shape[1]
    return dict(part=e['k'].sum(1), part_b=e['k_b'].sum(1) + ref64.row_sum_bound(e['k_c'], N) + FLOOR)


def mix_bwd(G, kind, gammas, gout, coef, sa=None, sb=None):
    """W[i, j] = (coef * gout) * dk_ij and rs[i] = sum_j W[i, j]"""
    e = mix_elements(G, kind, gammas, sa, sb)
    N = e['dk'].shape[1]
    c = f32(coef) * float(f64(gout).reshape(-1)[0])
    W = c * e['dk']
    W_b = abs(c) * e['dk_b'] + C_W * U * W.abs() + FLOOR
    return dict(W=W, W_b=W_b, rs=W.sum(1), rs_b=W_b.sum(1) + ref64.row_sum_bound(abs(c) * e['dk_c'], N) + FLOOR)


def combine(p11, p12, p22, c11, c12, c22):
    """out = (m11 - 2 m12 + m22, m11, m12, m22), m = sum(p) / c with c as the fp32 passed; the kernel sums in double:
    only the roundings of the stores count"""
    m11, m12, m22 = (f64(p).sum() / f32(c) for p, c in ((p11, c11), (p12, c12), (p22, c22)))
    out = torch.stack([m11 - 2 * m12 + m22, m11, m12, m22])
    b = torch.stack([2 * (m11.abs() + 2 * m12.abs() + m22.abs()), m11.abs(), m12.abs(), m22.abs()]) * U + FLOOR
    return dict(out=out, out_b=b)


def _sumsq(diff, e_diff):
    """(sum_d diff^2, its bound) of a difference known to e_diff, summed by a 256-stride row sum"""
    d2 = diff * diff
    return d2.sum(), (2 * diff.abs() * e_diff + e_diff * e_diff).sum() + ref64.row_sum_bound(d2[None, :], diff.numel())[0] + FLOOR


def identity_fwd(x1, x2):
    """diff[d] = mean(x1[:, d]) - mean(x2[:, d]) (a column is one serial chain), out[0] = sum_d diff[d]^2"""
    x1, x2 = f64(x1), f64(x2)
    n1, n2 = x1.shape[0], x2.shape[0]
    m1, m2 = x1.mean(0), x2.mean(0)
    e1 = col_sum_bound(x1, n1, 1) / n1 + U * m1.abs()
    e2 = col_sum_bound(x2, n2, 1) / n2 + U * m2.abs()
    diff = m1 - m2
    e_diff = e1 + e2 + U * diff.abs() + FLOOR
    out, out_b = _sumsq(diff, e_diff)
    return dict(diff=diff, diff_b=e_diff, out=out.reshape(1), out_b=out_b.reshape(1))


def identity_bwd(diff, gout, coef, n):
    """dx[i, d] = (coef * gout) * diff[d] on the given fp32 diff"""
    dx = (f32(coef) * float(f64(gout).reshape(-1)[0]) * f64(diff))[None, :].expand(n, -1)
    return dict(dx=dx, dx_b=3 * U * dx.abs() + FLOOR)


def rff_fwd(th1, th2, c):
    """diff[r] = c * (mean_i cos th1[i, r] - mean_j cos th2[j, r]) on the given fp32 theta (four row groups per column),
    mmd2 = sum_r diff[r]^2"""
    c1, c2 = torch.cos(f64(th1)), torch.cos(f64(th2))
    n1, n2 = c1.shape[0], c2.shape[0]
    c = f32(c)
    m1, m2 = c1.mean(0), c2.mean(0)
    e1 = col_sum_bound(c1, n1, 4) / n1 + C_TRIG * U + U * m1.abs()       # (every cosine off by C_TRIG U: so is their mean)
    e2 = col_sum_bound(c2, n2, 4) / n2 + C_TRIG * U + U * m2.abs()
    diff = c * (m1 - m2)
    e_diff = abs(c) * (e1 + e2) + 2 * U * diff.abs() + FLOOR
    out, out_b = _sumsq(diff, e_diff)
    return dict(diff=diff, diff_b=e_diff, mmd2=out.reshape(1), mmd2_b=out_b.reshape(1))


def rff_bwd(th, diff, gout, coef):
    """G[i, r] = -(coef * gout) * diff[r] * sin th[i, r] on the given fp32 diff: three products, and the sine's C_TRIG"""
    s = f32(coef) * float(f64(gout).reshape(-1)[0])
    amp = (s * f64(diff)).abs()[None, :]
    Gm = -s * f64(diff)[None, :] * torch.sin(f64(th))
    return dict(G=Gm, G_b=3 * U * Gm.abs() + C_TRIG * U * amp + FLOOR)


def root_bound(v, e):
    """what sqrt(v) may be off by when v is known to e: sqrt(v) - sqrt(max(v - e, 0)) (the steeper side), and the root's
    own rounding"""
    v = torch.as_tensor(v, dtype=torch.float64)
    return torch.sqrt(v) - torch.sqrt(torch.clamp(v - e, min=0.0)) + 2 * U * torch.sqrt(v) + FLOOR


def objective(x1, x2, kernel, gammas=None):
    """(MMD^2 in the Gram form, its bound) of ``blocks.mmd_objective`` before the root, on fp32 rows: the three Gram
    products are off by ``gemm_contract.acc_bound`` (which enters rbf through e_d2, poly through dk/dG), every mean is a
    row-sum launch and a sum in double, the combination two roundings"""
    from tests.gemm_contract import acc_bound
    if kernel == 'identity':
        r = identity_fwd(x1, x2)
        return r['out'][0], r['out_b'][0]
    x1, x2 = x1.float(), x2.float()
    norm = lambda a: ((a.double() ** 2).sum(1), 1.01 * (a.shape[1] + 16) * U * (a.double() ** 2).sum(1))
    ms, es = [], []
    for a, b in ((x1, x1), (x1, x2), (x2, x2)):
        G, eG = acc_bound(a, b.t())
        (sa, e_sa), (sb, e_sb) = norm(a), norm(b)
        e = mix_elements(G, kernel, gammas, sa, sb, e_G=eG, e_sa=e_sa, e_sb=e_sb)
        cnt = G.numel()
        part_b = e['k_b'].sum(1) + ref64.row_sum_bound(e['k_c'], G.shape[1])
        m = e['k'].sum() / cnt
        ms.append(m)
        es.append(part_b.sum() / cnt + U * m.abs())
    mag = ms[0].abs() + 2 * ms[1].abs() + ms[2].abs()
    return ms[0] - 2 * ms[1] + ms[2], es[0] + 2 * es[1] + es[2] + 2 * U * mag + FLOOR


def grouped(z, cls, grp_ptr, rows, src, S, kind, w, ref, W=None, b=None, a=None, c=None):
    """bounds (e_theta, e_diff, e_m2, e_value; numpy float64) of the grouped MMD penalty (``dv_mmd_grouped_*``) around the
    float64 reference ``ref`` = ``nuisance_cases.mmd_ref(...)`` of the same problem:
    theta is a Z-term fma chain and one fma, (Z + 2) U (|a| sum |z w| + |phase|); diff carries that condition through the
    1-Lipschitz cosine (plus C_TRIG U), the side sums of 16 row groups that take 4 rows per pass, two divisions, the
    subtraction and the factor c; m2 is a 256-stride sum of squares; the value a root per term and their serial sum"""
    import numpy as np
    diff, m2, value, _, theta, _ = ref
    z = np.asarray(z, np.float64)
    cls, rows, src = np.asarray(cls), np.asarray(rows), np.asarray(src)
    Kc = 1 if S == 2 else S
    n_groups, E = len(grp_ptr) - 1, int(grp_ptr[-1])
    rff = kind == 'rbf_fourier'
    D, Z = diff.shape[1], z.shape[1]
    e_theta = np.zeros_like(theta) if rff else None
    e_diff, e_m2, e_val = np.zeros_like(diff), np.zeros_like(m2), 0.0
    for g in range(n_groups):
        e0, e1 = int(grp_ptr[g]), int(grp_ptr[g + 1])
        r, cj, n = rows[e0:e1], cls[src[e0:e1]], e1 - e0
        csum = (math.ceil(n / 64) * 4 + 16) * U
        for k in range(Kc):
            t = g * Kc + k
            side = cj == k
            if side.sum() == 0 or (~side).sum() == 0:
                continue
            if rff:
                mag = abs(f32(a)) * (np.abs(z[r]) @ np.abs(np.asarray(W[t], np.float64))) + 2 * math.pi * np.abs(np.asarray(b[t], np.float64))
                eth = (Z + 2) * U * mag + FLOOR
                e_theta[k * E + e0:k * E + e1] = eth
                v, e_v = np.cos(theta[k * E + e0:k * E + e1]), eth + C_TRIG * U
            else:
                v, e_v = z[r], np.zeros((n, D))
            e_means = 0.0
            for sd in (side, ~side):
                ns = int(sd.sum())
                e_means = e_means + (e_v[sd].sum(0) + csum * np.abs(v[sd]).sum(0)) / ns + U * np.abs(v[sd].sum(0) / ns)
            e_diff[t] = abs(c if rff else 1.0) * e_means + 2 * U * np.abs(diff[t]) + FLOOR
            e_m2[t] = (2 * np.abs(diff[t]) * e_diff[t] + e_diff[t] ** 2).sum() + (math.ceil(D / 256) + 16) * U * m2[t] + FLOOR
            rt = math.sqrt(m2[t])
            e_val += abs(w) * (rt - math.sqrt(max(m2[t] - e_m2[t], 0.0)) + 3 * U * rt)
    e_val += n_groups * Kc * U * abs(value) + FLOOR
    return e_theta, e_diff, e_m2, e_val


def bn_fwd(x, w, b, running_mean, running_var, eps=1e-5, momentum=0.1, training=True):
    """nn.BatchNorm1d over the rows of x: batch mean and biased variance in two passes (four row groups per column), the
    running statistics moved by ``momentum`` (running_var by the unbiased variance); eval: the running statistics"""
    x = f64(x)
    M, N = x.shape
    eps, mom = f32(eps), f32(momentum)
    w64 = f64(w) if w is not None else torch.ones(N, dtype=torch.float64)
    b64 = f64(b) if b is not None else torch.zeros(N, dtype=torch.float64)
    cs = (math.ceil(M / 4) + 3) * U
    out = {}
    if training:
        mu = x.mean(0)
        e_mu = cs * x.abs().sum(0) / M + U * mu.abs() + FLOOR
        d = (x - mu).abs()
        e_d = e_mu + U * d
        var = (d * d).mean(0)
        e_var = (cs * (d * d).sum(0) + (2 * d * e_d + e_d * e_d + U * d * d).sum(0)) / M + U * var + FLOOR
        if running_mean is not None:
            old_m, old_v = f64(running_mean), f64(running_var)
            unb = var * M / (M - 1) if M > 1 else var
            e_unb = e_var * M / (M - 1) if M > 1 else e_var
            out.update(running_mean=(1 - mom) * old_m + mom * mu,
                       running_mean_b=mom * e_mu + 3 * U * (old_m.abs() + mu.abs()) + FLOOR,
                       running_var=(1 - mom) * old_v + mom * unb,
                       running_var_b=mom * e_unb + 3 * U * (old_v.abs() + unb.abs()) + FLOOR)
    else:
        mu, var = f64(running_mean), f64(running_var)
        e_mu = torch.zeros_like(mu)
        e_var = torch.zeros_like(var)                      # (what is left of it: the rounding of rvar + eps, below)
        d = (x - mu).abs()
        e_d = U * d
    rstd = 1 / torch.sqrt(var + eps)
    e_rstd = rstd * (0.5 * (e_var + U * (var + eps)) / (var + eps) + 3 * U)
    y = (x - mu) * rstd * w64 + b64
    e_y = w64.abs() * (rstd * e_d + d * e_rstd) + 4 * U * (w64.abs() * d * rstd + b64.abs())
    out.update(mean=mu, mean_b=e_mu + FLOOR, rstd=rstd, rstd_b=e_rstd + FLOOR, y=y, y_b=e_y + FLOOR, var=var,
               var_b=e_var + FLOOR)
    return out


def bn_bwd(dy, x, mean, rstd, w, training=True, e_mean=None, e_rstd=None):
    """db = sum dy, dw = sum dy * xhat, xhat = (x - mean) * rstd on the saved mean / rstd -- taken as given fp32, or
    (whole operations: ``e_mean`` / ``e_rstd``) the float64 statistics which the saved ones match to those bounds;
    training: dx = w rstd (dy - db / M - xhat dw / M), eval: dx = dy w rstd"""
    dy, x, mu, rs = f64(dy), f64(x), f64(mean), f64(rstd)
    M, N = x.shape
    w64 = f64(w) if w is not None else torch.ones(N, dtype=torch.float64)
    e_rs = torch.zeros(N, dtype=torch.float64) if e_rstd is None else f64(e_rstd)
    xh = (x - mu) * rs
    e_xh = 2 * U * xh.abs()
    if e_mean is not None:
        e_xh = e_xh + rs * f64(e_mean) + (x - mu).abs() * e_rs
    db, dw = dy.sum(0), (dy * xh).sum(0)
    e_db = col_sum_bound(dy, M, 4) + FLOOR
    e_dw = col_sum_bound(dy * xh, M, 4) + (dy.abs() * e_xh + U * (dy * xh).abs()).sum(0) + FLOOR
    if training:
        t2, t3 = db / M, xh * dw / M
        e_t2 = (e_db + 2 * U * db.abs()) / M
        e_t3 = (xh.abs() * e_dw + dw.abs() * e_xh + 3 * U * (xh * dw).abs()) / M
        mag = dy.abs() + t2.abs() + t3.abs()
        dx = w64 * rs * (dy - t2 - t3)
        e_dx = (w64 * rs).abs() * (e_t2 + e_t3 + 2 * U * mag) + 3 * U * (w64 * rs).abs() * mag + w64.abs() * e_rs * mag
    else:
        dx = dy * w64 * rs
        e_dx = 3 * U * dx.abs() + (dy * w64).abs() * e_rs
    return dict(dx=dx, dx_b=e_dx + FLOOR, dw=dw, dw_b=e_dw, db=db, db_b=e_db)


def mask_scale(x, mask, scale):
    """exact: the fp32 product x * mask * scale, in that order"""
    x, mask = x.detach().cpu().float(), mask.detach().cpu().float()
    return (x * mask) * torch.tensor(scale, dtype=torch.float32)


# ================================================================================================ poisoned operands
class Strided:
    """host tensor ``t`` as a view with row stride ``width + pad`` in the middle of a buffer on ``dev`` whose row pads and
    ``GUARD`` rows (elements, for a vector) in front and behind hold ``fill``: NaN around an operand (whatever is read
    outside it poisons what it feeds), the sentinel around an output (whatever is written outside it shows)"""

    def __init__(self, t, dev, pad=3, fill=NAN):
        t = t.float()
        if t.dim() == 1:
            n = t.numel()
            self.buf = torch.full((GUARD + n + GUARD,), fill, dtype=torch.float32, device=dev)
            self.view = self.buf[GUARD:GUARD + n]
        else:
            r, c = t.shape
            self.buf = torch.full((GUARD + r + GUARD, c + pad), fill, dtype=torch.float32, device=dev)
            self.view = self.buf[GUARD:GUARD + r, :c]
        self.view.copy_(t.to(dev))
        self.inside = torch.zeros(self.buf.shape, dtype=torch.bool, device=dev)
        if t.dim() == 1:
            self.inside[GUARD:GUARD + t.numel()] = True
        else:
            self.inside[GUARD:GUARD + t.shape[0], :t.shape[1]] = True
        self.before = self.buf.view(torch.int32).clone()

    def same(self, outside_only):
        eq = self.buf.view(torch.int32) == self.before
        return bool(eq[~self.inside].all()) if outside_only else bool(eq.all())


class Frame:
    """the operands and outputs of one launch; ``verify``: operands unchanged, nothing written outside an output's view"""

    def __init__(self, dev):
        self.dev, self.ins, self.outs = dev, [], []

    def inp(self, t, pad=3):
        if t is None:
            return None
        self.ins.append(Strided(t, self.dev, pad))
        return self.ins[-1].view

    def out(self, init, pad=5):
        """``init``: a shape (the view starts as NaN: the launch may not read it) or its values (updated in place)"""
        if not torch.is_tensor(init):
            init = torch.full(tuple(init), NAN)
        self.outs.append(Strided(init, self.dev, pad, fill=SENTINEL))
        return self.outs[-1].view

    def verify(self, untouched=False):
        if self.dev.type == 'cuda':
            torch.cuda.synchronize()
        for i, p in enumerate(self.ins):
            assert p.same(False), 'operand %d was written' % i
        for i, p in enumerate(self.outs):
            assert p.same(not untouched), 'output %d: %s' % (i, 'was written by a refused launch' if untouched else
                                                         'bytes outside the view were written')


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def diag_matrix(v):
    """a square matrix whose diagonal is ``v`` and whose other elements are NaN: only the diagonal may be read"""
    n = v.numel()
    m = torch.full((n, n), NAN)
    m[torch.arange(n), torch.arange(n)] = v.float()
    return m


# ================================================================================================ cases
MIX_SHAPES = ((1, 1), (1, 9), (5, 255), (3, 256), (4, 257), (2, 600))
MIX_NB = (1, 5, 8)


def mix_coefs(M, N):
    """(coef, gout) of the backward launches: coef * gout of 0.7 and of -2 / (n1 n2), and one pair whose product rounds"""
    return ((0.7, 1.0), (-2.0 / (M * N), 1.0), (0.7, 1.3))
MIX_Z = 6


def mix_gammas(nb, kind):
    """nb bandwidths as ``mmd_objective`` forms them for Z = MIX_Z (1.22 .. 0.012, then their doubles).  rbf: between the
    rows around 0 and the rows offset by 10 d2 is about 600, so gamma d2 passes 104 for the first two (the exponential
    underflows) and stays below it for the others"""
    return [math.sqrt(MIX_Z) * DEFAULT_BW[i % 5] * (1 + i // 5) for i in range(nb)]


def mix_case(M, N, nb, kind, seed=0):
    """rows around 0 and rows offset by 3 and by 10 on both sides, one pair of identical rows; G, sa, sb are the fp32
    products of those rows (what the Gram launches hand over, up to their own rounding)"""
    g = torch.Generator().manual_seed(7919 * M + 31 * N + nb + seed)
    off = torch.tensor([0.0, 3.0, 10.0])
    a = torch.randn(M, MIX_Z, generator=g) * 0.5 + off[torch.arange(M) % 3][:, None]
    b = torch.randn(N, MIX_Z, generator=g) * 0.5 + off[(torch.arange(N) // 2) % 3][:, None]
    b[0] = a[0]                                                        # identical rows: d2 = 0 up to the products' rounding
    G = (a.double() @ b.double().t()).float()
    sa, sb = (a.double() ** 2).sum(1).float(), (b.double() ** 2).sum(1).float()
    return dict(G=G, sa=sa, sb=sb, gammas=mix_gammas(nb, kind), kind=kind, nb=nb, a=a, b=b)


def mix_clamped_case(nb):
    """sa = sb = s = 1e4 and G = s (1 + 2**-22): the raw d2 is negative; k = 1 and dk = -mean(gamma) exactly (gammas are
    powers of two; for nb = 5 the fp32 1/5 leaves the mean to two roundings)"""
    s = torch.full((3,), 1e4)
    G = torch.full((3, 3), float(1e4 * (1 + 2.0 ** -22)))
    assert float(G[0, 0]) > 1e4
    return dict(G=G, sa=s, sb=s, gammas=[2.0 ** (i - 3) for i in range(nb)], kind='rbf', nb=nb)


IDENTITY_SHAPES = ((1, 1, 1), (1, 9, 5), (7, 3, 255), (5, 6, 257), (130, 70, 600))


def identity_case(n1, n2, Z, offset):
    """columns around 0, or with the common offset 100 where the two populations differ by 1e-3"""
    g = torch.Generator().manual_seed(n1 * 1009 + n2 * 17 + Z)
    if offset:
        x1 = 100.0 + 0.05 * torch.randn(n1, Z, generator=g)
        x2 = 100.0 + 1e-3 + 0.05 * torch.randn(n2, Z, generator=g)
    else:
        x1, x2 = torch.randn(n1, Z, generator=g), torch.randn(n2, Z, generator=g) * 0.5 + 0.2
    return x1, x2


RFF_SHAPES = ((1, 1, 1), (3, 5, 63), (4, 4, 64), (5, 3, 65), (301, 33, 500))


def rff_case(n1, n2, R):
    """theta over [-50, 50], its last column exact fp32 multiples of pi / 2"""
    g = torch.Generator().manual_seed(n1 * 131 + n2 * 7 + R)
    th1, th2 = (torch.rand(n, R, generator=g) * 100 - 50 for n in (n1, n2))
    hp = torch.tensor(math.pi / 2, dtype=torch.float32)
    th1[:, -1] = (torch.arange(n1) - n1 // 2).float() * hp
    th2[:, -1] = (torch.arange(n2) + 1).float() * hp
    return th1, th2, math.sqrt(2.0 / R)


BN_M = (2, 3, 5, 67)
BN_N = (1, 63, 64, 65, 130)
BN_KINDS = ('normal', 'offset', 'constant', 'tiny', 'large')


def bn_input(M, N, with_constant=True, seed=0):
    """columns cycling through: N(0,1); 1e3 +- 1e-2; constant 0.1; 1e-20-scaled; 1e4-scaled"""
    g = torch.Generator().manual_seed(100 * M + N + seed)
    x = torch.randn(M, N, generator=g)
    kinds = [k for k in BN_KINDS if with_constant or k != 'constant']
    for j in range(N):
        k = kinds[j % len(kinds)]
        if k == 'offset':
            x[:, j] = 1e3 + 1e-2 * x[:, j]
        elif k == 'constant':
            x[:, j] = 0.1
        elif k == 'tiny':
            x[:, j] *= 1e-20
        elif k == 'large':
            x[:, j] *= 1e4
    return x


def bn_params(N, seed=0):
    g = torch.Generator().manual_seed(5 + N + seed)
    return dict(w=torch.randn(N, generator=g) * 0.5 + 1.0, b=torch.randn(N, generator=g),
                rm=torch.randn(N, generator=g), rv=torch.rand(N, generator=g) + 0.5)


# (training, affine, running statistics, momentum, eps)
BN_FWD_MODES = ((True, True, True, 0.1, 1e-5), (True, False, False, 0.1, 1e-5), (True, True, True, 1.0, 1e-5),
                (True, True, True, 0.1, 0.0), (False, True, True, 0.1, 1e-5), (False, False, True, 0.1, 0.0))
# (training, affine, which output is None)
BN_BWD_MODES = ((True, True, None), (True, False, 'dx'), (True, True, 'dw'), (True, True, 'db'), (False, True, None),
                (False, False, 'dw'))

MASK_SHAPES = ((1, 1), (3, 255), (2, 257), (67, 130))
MASK_SCALES = (2.0, 1 / 0.9)


def mask_case(M, N):
    g = torch.Generator().manual_seed(M * 13 + N)
    x = torch.randn(M, N, generator=g)
    mask = (torch.rand(M, N, generator=g) < 0.6).float()
    mask[M // 2] = 0.0
    return x, mask


# ================================================================================================ case runners
# ``K``: the launchers (drvae_amd.kernels on the device, the fp32 stand-ins of tests/kernel_ref.py on the host).  Every
# runner places the operands as strided views in poisoned buffers, launches twice (the same bits), checks the memory
# contract and returns the worst excess (error / bound) per check.
def _twice(launch, outs):
    launch()
    first = [o.clone() for o in outs]
    launch()
    for a, b in zip(first, outs):
        assert same_bits(a, b), 'two launches on the same operands stored different bits'


def run_mix(K, dev, case, coefs=((0.7, 1.0),)):
    """``coefs``: (coef, gout) pairs of the backward launches"""
    G, sa, sb, gam, kind = case['G'], case['sa'], case['sb'], case['gammas'], case['kind']
    M, N = G.shape
    rbf = kind == 'rbf'
    res = {}
    fr = Frame(dev)
    Gd = fr.inp(G, 3)
    sad = fr.inp(diag_matrix(sa), 5) if rbf else None
    sbd = fr.inp(diag_matrix(sb), 3) if rbf else None
    part = fr.out((M,))
    _twice(lambda: K.mmd_mix_fwd(part, Gd, kind, gam, sad, sbd), [part])
    fr.verify()
    r = mix_fwd(G, kind, gam, sa, sb)
    res['mix_%s part' % kind] = ref64.check('mmd_mix_fwd %s part' % kind, part, r['part'], r['part_b'])
    for coef, g0 in coefs:
        fr = Frame(dev)
        Gd = fr.inp(G, 5)
        sad = fr.inp(diag_matrix(sa), 3) if rbf else None
        sbd = fr.inp(diag_matrix(sb), 5) if rbf else None
        gout = fr.inp(torch.tensor([g0]))
        W, rs = fr.out((M, N), 3), fr.out((M,))
        _twice(lambda: K.mmd_mix_bwd(W, rs, Gd, kind, gam, gout, coef, sad, sbd), [W, rs])
        fr.verify()
        r = mix_bwd(G, kind, gam, torch.tensor([g0]), coef, sa, sb)
        res['mix_%s W' % kind] = max(res.get('mix_%s W' % kind, 0.0),
                                     ref64.check('mmd_mix_bwd %s W' % kind, W, r['W'], r['W_b'], G=G))
        res['mix_%s rs' % kind] = max(res.get('mix_%s rs' % kind, 0.0),
                                      ref64.check('mmd_mix_bwd %s rs' % kind, rs, r['rs'], r['rs_b']))
    return res


def run_mix_clamped(K, dev, nb):
    """the constructed case: k = 1 to the bit; dk = -mean(gamma), to the bit where the mean is formed exactly"""
    case = mix_clamped_case(nb)
    G, s, gam = case['G'], case['sa'], case['gammas']
    fr = Frame(dev)
    Gd, sad, sbd = fr.inp(G), fr.inp(diag_matrix(s), 5), fr.inp(diag_matrix(s), 3)
    gout = fr.inp(torch.tensor([1.0]))
    part, W, rs = fr.out((3,)), fr.out((3, 3)), fr.out((3,))
    K.mmd_mix_fwd(part, Gd, 'rbf', gam, sad, sbd)
    K.mmd_mix_bwd(W, rs, Gd, 'rbf', gam, gout, 1.0, sad, sbd)
    fr.verify()
    assert same_bits(part.cpu(), torch.full((3,), 3.0)), 'k != 1 under the clamp: part = %r' % part.tolist()
    mean = sum(gam) / nb
    tol = 0.0 if nb in (1, 8) else 2 * U * mean
    assert float((f64(W) + mean).abs().max()) <= tol, 'dk != -mean(gamma) under the clamp: %r' % W.tolist()
    r = mix_bwd(G, 'rbf', gam, torch.tensor([1.0]), 1.0, s, s)
    return {'mix_rbf clamped rs': ref64.check('mmd_mix_bwd clamped rs', rs, r['rs'], r['rs_b'])}


COMBINE_LENGTHS = (1, 9, 600)


def run_combine(K, dev, n):
    g = torch.Generator().manual_seed(n)
    p11, p12, p22 = (torch.rand(n, generator=g) * 4097 + 0.5 for _ in range(3))
    c = (float(4097 ** 2), float(n * 9), float(81))      # 4097^2 = 16785409 is no fp32: the launch receives 16785408
    assert f32(c[0]) != c[0]
    fr = Frame(dev)
    ps = [fr.inp(p) for p in (p11, p12, p22)]
    out = fr.out((4,))
    _twice(lambda: K.mmd_mix_combine(out, ps[0], ps[1], ps[2], *c), [out])
    fr.verify()
    r = combine(p11, p12, p22, *c)
    return {'mix combine': ref64.check('mmd_mix_combine', out, r['out'], r['out_b'])}


def run_identity(K, dev, n1, n2, Z, offset):
    x1, x2 = identity_case(n1, n2, Z, offset)
    fr = Frame(dev)
    a, b = fr.inp(x1, 3), fr.inp(x2, 5)
    diff, out = fr.out((Z,)), fr.out((1,))
    _twice(lambda: K.mmd_identity_fwd(diff, out, a, b), [diff, out])
    fr.verify()
    r = identity_fwd(x1, x2)
    res = {'identity diff': ref64.check('mmd_identity_fwd diff', diff, r['diff'], r['diff_b']),
           'identity out': ref64.check('mmd_identity_fwd out', out, r['out'], r['out_b'])}
    given = diff.detach().cpu().clone()
    for n, coef in ((n1, 2.0 / n1), (n2, -2.0 / n2)):
        fr = Frame(dev)
        dd, gout = fr.inp(given), fr.inp(torch.tensor([0.7]))
        dx = fr.out((n, Z), 3)
        _twice(lambda: K.mmd_identity_bwd(dx, dd, gout, coef), [dx])
        fr.verify()
        r = identity_bwd(given, torch.tensor([0.7]), coef, n)
        res['identity dx'] = max(res.get('identity dx', 0.0), ref64.check('mmd_identity_bwd dx', dx, r['dx'], r['dx_b']))
    return res


def run_rff(K, dev, n1, n2, R):
    th1, th2, c = rff_case(n1, n2, R)
    fr = Frame(dev)
    a, b = fr.inp(th1, 5), fr.inp(th2, 3)
    diff, m2 = fr.out((R,)), fr.out((1,))
    _twice(lambda: K.mmd_rff_fwd(diff, m2, a, b, c), [diff, m2])
    fr.verify()
    r = rff_fwd(th1, th2, c)
    res = {'rff diff': ref64.check('mmd_rff_fwd diff', diff, r['diff'], r['diff_b']),
           'rff mmd2': ref64.check('mmd_rff_fwd mmd2', m2, r['mmd2'], r['mmd2_b'])}
    given = diff.detach().cpu().clone()
    for th, coef in ((th1, 2.0 * c / n1), (th2, -2.0 * c / n2)):
        fr = Frame(dev)
        t, dd, gout = fr.inp(th, 3), fr.inp(given), fr.inp(torch.tensor([0.7]))
        Gm = fr.out(tuple(th.shape), 5)
        _twice(lambda: K.mmd_rff_bwd(Gm, t, dd, gout, coef), [Gm])
        fr.verify()
        r = rff_bwd(th, given, torch.tensor([0.7]), coef)
        res['rff G'] = max(res.get('rff G', 0.0), ref64.check('mmd_rff_bwd G', Gm, r['G'], r['G_b'], theta=th))
    return res


def run_bn_fwd(K, dev, M, N, mode):
    training, affine, running, mom, eps = mode
    x = bn_input(M, N, with_constant=eps > 0)
    p = bn_params(N)
    w, b = (p['w'], p['b']) if affine else (None, None)
    rm, rv = (p['rm'], p['rv']) if running else (None, None)
    fr = Frame(dev)
    xd, wd, bd = fr.inp(x, 3), fr.inp(w), fr.inp(b)
    y, mean, rstd = fr.out((M, N), 5), fr.out((N,)), fr.out((N,))
    rmd, rvd = (fr.out(rm), fr.out(rv)) if running else (None, None)
    K.bn_fwd(y, xd, wd, bd, mean, rstd, rmd, rvd, eps=eps, momentum=mom, training=training)
    fr.verify()
    first = [t.clone() for t in (y, mean, rstd)] + ([rmd.clone(), rvd.clone()] if running else [])
    if running:                                           # the second launch starts from the same running statistics
        rmd.copy_(rm.to(dev))
        rvd.copy_(rv.to(dev))
    K.bn_fwd(y, xd, wd, bd, mean, rstd, rmd, rvd, eps=eps, momentum=mom, training=training)
    fr.verify()
    for a, c in zip(first, [y, mean, rstd] + ([rmd, rvd] if running else [])):
        assert same_bits(a, c), 'two launches on the same operands stored different bits'
    r = bn_fwd(x, w, b, rm, rv, eps, mom, training)
    tag = 'bn_fwd %s' % ('train' if training else 'eval')
    res = {tag + ' mean': ref64.check(tag + ' mean', mean, r['mean'], r['mean_b']),
           tag + ' rstd': ref64.check(tag + ' rstd', rstd, r['rstd'], r['rstd_b'], var=r['var']),
           tag + ' y': ref64.check(tag + ' y', y, r['y'], r['y_b'], x=x)}
    if training and running:
        res[tag + ' running_mean'] = ref64.check(tag + ' running_mean', rmd, r['running_mean'], r['running_mean_b'])
        res[tag + ' running_var'] = ref64.check(tag + ' running_var', rvd, r['running_var'], r['running_var_b'])
    if not training:
        assert same_bits(mean.cpu(), rm) and same_bits(rmd.cpu(), rm) and same_bits(rvd.cpu(), rv), \
            'eval mode: the running statistics are read, never written, and mean is their copy'
    return res


def bn_saved(x, eps=1e-5):
    """the fp32 mean / rstd a forward pass would have saved"""
    mu = x.double().mean(0)
    var = ((x.double() - mu) ** 2).mean(0)
    return mu.float(), (1 / torch.sqrt(var + eps)).float()


def run_bn_bwd(K, dev, M, N, mode):
    training, affine, none = mode
    x = bn_input(M, N)
    g = torch.Generator().manual_seed(M + 3 * N)
    dy = torch.randn(M, N, generator=g)
    dy[:, N // 2] = 0.0                                     # a column of zeros
    w = bn_params(N)['w'] if affine else None
    mean, rstd = bn_saved(x)
    fr = Frame(dev)
    dyd, xd, md, rd, wd = fr.inp(dy, 5), fr.inp(x, 3), fr.inp(mean), fr.inp(rstd), fr.inp(w)
    dx = None if none == 'dx' else fr.out((M, N), 3)
    dw = None if none == 'dw' else fr.out((N,))
    db = None if none == 'db' else fr.out((N,))
    _twice(lambda: K.bn_bwd(dx, dw, db, dyd, xd, md, rd, wd, training=training), [t for t in (dx, dw, db) if t is not None])
    fr.verify()
    r = bn_bwd(dy, x, mean, rstd, w, training)
    tag = 'bn_bwd %s' % ('train' if training else 'eval')
    res = {}
    for name, t in (('dx', dx), ('dw', dw), ('db', db)):
        if t is not None:
            key = (tag + ' dx') if name == 'dx' else 'bn_bwd ' + name
            res[key] = ref64.check(key, t, r[name], r[name + '_b'])
    return res


def run_mask_scale(K, dev, M, N, scale):
    x, mask = mask_case(M, N)
    want = mask_scale(x, mask, scale)
    fr = Frame(dev)
    xd, md = fr.inp(x, 3), fr.inp(mask, 5)
    y = fr.out((M, N), 5)
    _twice(lambda: K.mask_scale(y, xd, md, scale), [y])
    fr.verify()
    assert same_bits(y.cpu(), want), 'mask_scale out of place: not the fp32 product x * mask * scale'
    fr = Frame(dev)
    md = fr.inp(mask, 3)
    xy = fr.out(x, 5)
    K.mask_scale(xy, xy, md, scale)
    fr.verify()
    assert same_bits(xy.cpu(), want), 'mask_scale in place (y is x): not the bits of the out-of-place launch'
    return {'mask_scale': 0.0}


def report(res):
    """one line per check for the profile note (``pytest -s``)"""
    for k in sorted(res):
        print('EXCESS %-34s %.3g' % (k, res[k]))
    return res
