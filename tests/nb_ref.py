"""Float64 reference of the negative-binomial reconstruction rows (``dv_rec_nll_rows``, kind ``DV_REC_NEGBIN``;
``type_rec='nb'``), the error bound the kernel is held to, fp32 emulations of the row formula -- a careful one and three
faulty ones the bound catches -- and a model-level float64 reference.  Test-only.

Parametrisation: mean mu > 0, inverse dispersion theta > 0 (Var = mu + mu^2 / theta), count x >= 0:

    log p    = [lgamma(x+theta) - lgamma(theta)] - lgamma(x+1) + theta log(theta/(theta+mu)) + x log(mu/(theta+mu))
    d/dmu    = x/mu - (x+theta)/(theta+mu)
    d/dtheta = [psi(x+theta) - psi(theta)] + log(theta/(theta+mu)) + (mu-x)/(theta+mu)

The heads are mu = softplus(a_m) + 1e-6 and theta = softplus(a_t) + 1e-3; the kernel receives the finished fp32 heads and
writes the gradients w.r.t. a_m / a_t with the softplus slope taken from the stored output, -expm1(-(v - shift)) (shift as
the fp32 number the kernel carries).

The bound (``tests/ref64.py``'s rule: |got - ref| <= C U sum|components|, U = 2^-24; a row sum adds ``row_sum_bound``).
The COMPONENTS are the float64 terms after each cancelling pair is combined -- |lgamma(x+theta) - lgamma(theta)|,
lgamma(x+1), |theta log(theta/(theta+mu))|, |x log(mu/(theta+mu))|; for the gradients |x/mu| + |(x+theta)/(theta+mu)| and
|psi(x+theta) - psi(theta)| + |log(theta/(theta+mu))| + |(mu-x)/(theta+mu)|, times the slope plus its condition term
|y g'(y)| (the derivative is taken from a stored output).  That choice is the contract: an implementation that forms a
pair from two large values loses what cancels and lands outside.

C counts roundings by the rule of ``tests/test_gpu_numerics.py`` (a transcendental: 3, a product, quotient or sum: 1; the
count of the term with the most, plus the sums and factors that follow it):

* rows, C = 32.  The lgamma pair by recurrence then asymptotic difference, both at once when x > 8 and theta < 8:
  8 products and a log (11); a = b + d (1), d log a (4), d / b and log1p (4), b - 1/2 and the fused product-sum (2), the
  series difference (2), three sums (3): 16; together 27, plus joining them (1): 28.  lgamma(x+1): 3.  Each log-ratio term:
  quotient, log1p, product (5).  The term's three sums: 3.  28 + 3 = 31 <= 32.
* d/da_m, C = 16.  (x - mu) / (mu (1 + mu/theta)): 5; the slope (difference with the shift, expm1 polynomial or exp): 5; two
  products with it and the row coefficient: 2; 12 <= 16.
* d/da_t, C = 40.  The digamma pair: 8 quotients and 8 sums (16) and, behind them, two reciprocals, d / b and log1p (6), the
  two correction products (6), three sums (3): 31.  log1p(mu/theta): 4; (mu - x) / (theta + mu): 3; the two sums: 2; slope 5 and
  two products 2: 31 + 2 + 7 = 40.

The three faulty emulations (``emulate_fp32(..., pair=..., ratio=..., psi=...)``) and where the bound catches them
(``tests/test_nb_cpu.py``): two fp32 lgammas subtracted (theta = 1e4: each is ~8e4 with an ulp of 8e-3, the pair ~9 x);
theta * (log theta - log(theta + mu)) (mu / theta = 1e-6: the two logs agree to 1e-6 relative, below their ulp); two fp32
digammas subtracted (theta = 1e4: psi ~ 9.2 with an ulp of 1e-6, the pair ~ x / theta = 1e-4 x)."""
import contextlib
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests import ref64
from tests.ref64 import U, bound, f64, row_sum_bound

MU_SHIFT, THETA_SHIFT = 1e-6, 1e-3
C_ROW, C_GM, C_GT = 32, 16, 40
ENC_IN_SCALE = 1e-3         # (``ModelRef``)


# ------------------------------------------------------------------------------------------- float64 terms
def lgamma_pair(x, theta):
    """lgamma(x + theta) - lgamma(theta) in float64.  Above theta = 1e7 (where the two lgammas' own float64 ulps show) the
    pair is x log theta + sum_{k<x} log1p(k/theta) with the sum expanded in power sums of k (x <= 3e4: x/theta <= 3e-3,
    the first neglected term is below 1e-12 of the pair)"""
    direct = torch.lgamma(x + theta) - torch.lgamma(theta)
    big = torch.clamp(theta, min=1.0)
    s1 = x * (x - 1) / 2
    s2 = (x - 1) * x * (2 * x - 1) / 6
    s3 = s1 * s1
    series = x * torch.log(big) + s1 / big - s2 / (2 * big ** 2) + s3 / (3 * big ** 3)
    return torch.where(theta > 1e7, series, direct)


def logp_terms(x, mu, theta):
    """the four float64 terms of log p, each cancelling pair combined: (pair, lgamma(x+1), theta log(theta/(theta+mu)),
    x log(mu/(theta+mu))); log p = pair - lgamma(x+1) + the two log-ratio terms"""
    return (lgamma_pair(x, theta), torch.lgamma(x + 1), -theta * torch.log1p(mu / theta), -x * torch.log1p(theta / mu))


def logp64(x, mu, theta):
    """log p per element, float64, differentiable"""
    pair, lx, tl, xl = logp_terms(x, mu, theta)
    return pair - lx + tl + xl


def grads64(x, mu, theta):
    """closed form: (d/dmu, d/dtheta) and the magnitudes of their terms (pairs combined)"""
    psi = torch.digamma(x + theta) - torch.digamma(theta)
    psi = torch.where(x == 0, torch.zeros_like(psi), psi)
    lt = -torch.log1p(mu / theta)
    r = (mu - x) / (theta + mu)
    gm_a, gm_b = x / mu, (x + theta) / (theta + mu)
    return gm_a - gm_b, psi + lt + r, gm_a.abs() + gm_b.abs(), psi.abs() + lt.abs() + r.abs()


def grads_autograd(x, mu, theta):
    """the same two derivatives by float64 autograd through ``logp64`` (the cross-check of the closed form)"""
    m, t = mu.clone().requires_grad_(True), theta.clone().requires_grad_(True)
    logp64(x, m, t).sum().backward()
    return m.grad, t.grad


def reference(x, v_mu, v_theta, coef=None, shift=MU_SHIFT):
    """everything the kernel tests compare with, from the exact fp32 values the kernel received: rows, their bound, and with
    ``coef`` the gradients w.r.t. the pre-activations with theirs"""
    X = x.shape[1]
    xx, mu, th = f64(x), f64(v_mu), f64(v_theta)
    pair, lx, tl, xl = logp_terms(xx, mu, th)
    comps = pair.abs() + lx + tl.abs() + xl.abs()
    out = dict(ll=pair - lx + tl + xl, pair=pair, comps=comps)
    out['rows'] = out['ll'].sum(1)
    out['rows_bound'] = bound(C_ROW, comps).sum(1) + row_sum_bound(comps, X)
    if coef is not None:
        c = f64(coef)[:, None]
        gm, gt, gm_c, gt_c = grads64(xx, mu, th)
        ym, yt = mu - ref64.f32(shift), th - ref64.f32(THETA_SHIFT)
        sm, st = ref64.dact_from_y('softplus', ym), ref64.dact_from_y('softplus', yt)
        out['gm'], out['gt'] = c * gm * sm, c * gt * st
        out['gm_bound'] = bound(C_GM, c.abs() * gm_c * (sm + ym.abs() * ref64.dact_from_y_slope('softplus', ym)))
        out['gt_bound'] = bound(C_GT, c.abs() * gt_c * (st + yt.abs() * ref64.dact_from_y_slope('softplus', yt)))
    return out


# ------------------------------------------------------------------------------------------------ the grid
A_M = np.arange(-30 * 16, 10 * 16 + 1) / 16.0
MU_EXTRA = (1e2, 1e4)
THETAS = (1e-3, 0.1, 1.0, 37.5, 1e4, 1e6)       # (the first: a_t = -30, theta = its shift)
COUNTS = (0.0, 1.0, 3.0, 20.0, 1000.0, 30000.0)


def edge_grid(X=256):
    """the edge grid as fp32 (x, mu, theta) matrices of X columns (the tail repeats the head) and the row coefficients"""
    mus = np.concatenate([np.log1p(np.exp(-np.abs(A_M))) + np.maximum(A_M, 0) + MU_SHIFT, np.asarray(MU_EXTRA)])
    n = mus.size * len(THETAS) * len(COUNTS)
    M = -(-n // X)
    k = np.arange(M * X)
    mu = mus[k % mus.size]
    th = np.asarray(THETAS)[(k // mus.size) % len(THETAS)]
    xs = np.asarray(COUNTS)[(k // (mus.size * len(THETAS))) % len(COUNTS)]
    t = lambda a: torch.from_numpy(a.astype(np.float32)).reshape(M, X)
    coef = torch.tensor([1.0, -0.5, 2.0, 0.25])[torch.arange(M) % 4]
    return t(xs), t(mu), t(th), coef


# ------------------------------------------------------------------------------------------ fp32 emulations
def _f(a):
    return np.asarray(a, np.float32)


def emulate_fp32(x, mu, theta, shift=MU_SHIFT, pair='careful', ratio='careful', psi='careful'):
    """the row formula evaluated in numpy float32, operation by operation: (log p, d/da_m, d/da_t) per element.
    'careful' is the kernel's construction (recurrence product / reciprocal sum for at most 8 steps, then the difference of the
    asymptotic series around log1p; the log ratios as log1p).  FAULTY on purpose: ``pair='lgamma2'`` (two lgammas
    subtracted), ``ratio='logdiff'`` (theta * (log theta - log(theta + mu))), ``psi='digamma2'`` (two digammas subtracted)"""
    import scipy.special as sp
    f = np.float32
    x, m, t = _f(x), _f(mu), _f(theta)
    with np.errstate(all='ignore'):
        n8 = np.where(t < 8, np.ceil(f(8) - t), f(0)).astype(f)
        n = np.minimum(x, n8)
        d = x - n
        prod, rsum = np.ones_like(t), np.zeros_like(t)
        for k in range(8):
            tk = t + f(k)
            on = f(k) < n
            prod = np.where(on, prod * tk, prod).astype(f)
            rsum = np.where(on, rsum + f(1) / tk, rsum).astype(f)
        lg = np.where(n > 0, np.log(prod), f(0)).astype(f)
        b = t + n
        a = b + d
        ra, rb = f(1) / a, f(1) / b
        ra2, rb2 = ra * ra, rb * rb
        l1 = np.log1p(d * rb)
        sa = ra * (f(1 / 12) - ra2 * (f(1 / 360) - ra2 * f(1 / 1260)))
        sb = rb * (f(1 / 12) - rb2 * (f(1 / 360) - rb2 * f(1 / 1260)))
        qa = ra2 * ra2 * (f(1 / 120) - ra2 * f(1 / 252))
        qb = rb2 * rb2 * (f(1 / 120) - rb2 * f(1 / 252))
        far = d > 0
        lg = np.where(far, lg + (d * np.log(a) + (((b - f(0.5)) * l1 - d) + (sa - sb))), lg).astype(f)
        ps = np.where(far, rsum + (l1 + d * ra * rb * (f(0.5) + (a + b) * ra * rb * f(1 / 12)) + (qa - qb)), rsum).astype(f)
        if pair == 'lgamma2':
            lg = (_f(sp.gammaln(x + t)) - _f(sp.gammaln(t))).astype(f)
        if psi == 'digamma2':
            ps = (_f(sp.digamma(x + t)) - _f(sp.digamma(t))).astype(f)
        lt = -np.log1p(m / t)
        lm = -np.log1p(t / m)
        if ratio == 'logdiff':
            lt = (np.log(t) - np.log(t + m)).astype(f)
            lm = (np.log(m) - np.log(t + m)).astype(f)
        ll = (lg - _f(sp.gammaln(x + f(1)))) + (t * lt + x * lm)
        sm = -np.expm1(-(m - f(shift)))
        st = -np.expm1(-(t - f(THETA_SHIFT)))
        gm = (x - m) / (m * (f(1) + m / t)) * sm
        gt = (ps + lt + (m - x) / (t + m)) * st
    assert ll.dtype == f and gm.dtype == f and gt.dtype == f
    return ll, gm, gt


# ------------------------------------------------------------------------------- model-level float64 reference
GAUSS_TO_NB = (('decoder_x.encoder_mu.linear_mu', 'decoder_x.decoder_m.linear_m'),
               ('decoder_x.encoder_sg.linear_sg', 'decoder_x.decoder_t.linear_t'))


def nb_name(k):
    """the oracle's (Gaussian-decoder) parameter name -> the negative-binomial model's"""
    for a, b in GAUSS_TO_NB:
        if k.startswith(a + '.'):
            return b + k[len(a):]
    return k


@contextlib.contextmanager
def oracle_as_nb():
    """inside: ``oracle.models_ref`` driven with a ``diag_gaussian`` spec IS the negative-binomial model in float64 -- its
    decoder has the same two heads over one trunk and the second is softplus + 1e-3 already; the first head's activation and
    the row log-likelihood are substituted at run time (nothing under oracle/ changes), and torch's default dtype is float64"""
    from oracle import blocks_ref as B
    saved = (B.diag_gaussian_sigma, B.logp_sigma_rows, torch.get_default_dtype())

    def heads(inputs, p, prefix, n_hidden, nonlin, constrain_means=False):
        h = B.mlp(inputs, p, prefix + '.nnet', n_hidden, nonlin)
        return (F.softplus(B.linear(h, p, prefix + '.encoder_mu.linear_mu')) + MU_SHIFT,
                F.softplus(B.linear(h, p, prefix + '.encoder_sg.linear_sg')) + THETA_SHIFT)

    B.diag_gaussian_sigma = heads
    B.logp_sigma_rows = lambda x, mu, theta: logp64(x, mu, theta).sum(1)
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        B.diag_gaussian_sigma, B.logp_sigma_rows = saved[:2]
        torch.set_default_dtype(saved[2])


def count_batch(spec, n_rows, seed=3):
    """``oracle.models_ref.make_batch`` turned into counts the way its Poisson cases are, floor(|3 x|), with a few entries
    raised to 10^3 .. 10^4"""
    from oracle import models_ref as M
    b = M.make_batch(spec, n_rows, seed=seed)
    rs = np.random.RandomState(seed + 1000)
    for k in ('x1', 'x2'):
        c = np.floor(np.abs(3 * b[k])).astype(np.float32)
        big = rs.rand(*c.shape) < 0.03
        c[big] = np.floor(10 ** rs.uniform(3, 4, int(big.sum()))).astype(np.float32)
        b[k] = c
    b['x2'] = b['x2'] * b['has_x2'][:, None].astype(np.float32)
    return b


def to64(d):
    """a batch / noise container with its floating arrays as float64 (what the float64 oracle reads)"""
    return {k: (v.astype(np.float64) if isinstance(v, np.ndarray) and v.dtype == np.float32 else v) for k, v in d.items()}


class ModelRef:
    """the float64 model-level reference: a ``RefTrainer`` on the Gaussian-shaped spec, every call inside ``oracle_as_nb``"""

    def __init__(self, spec, seed=9):
        from oracle import models_ref as M
        assert spec.type_rec == 'diag_gaussian'
        self.spec = spec
        self.init32 = M.init_params(spec, seed, as_numpy=True)         # fp32 values, oracle names
        # the batches hold raw counts up to 1e4 and the encoder reads them: through unit-scale first-layer weights the
        # log-variance head lands in the hundreds and exp() of it overflows in any precision.  The encoder's first layer
        # starts 1e-3 times smaller (its gain under WeightNorm) -- what normalising the encoder's input would do
        q = 'encoder_z1.nnet.model.linear1.'
        self.init32[q + ('g' if spec.weight_norm else 'weight')] *= np.float32(ENC_IN_SCALE)
        params = type(self.init32)((k, torch.tensor(v.astype(np.float64), requires_grad=True)) for k, v in self.init32.items())
        self.tr = M.RefTrainer(spec, params)

    def engine_params(self):
        """the initial parameters under the negative-binomial model's names, in its order"""
        return type(self.init32)((nb_name(k), v) for k, v in self.init32.items())

    def loss(self, batch, noise, training=True):
        with oracle_as_nb():
            return self.tr.loss(to64(batch), to64(noise), training)

    def step(self, batch, noise):
        with oracle_as_nb():
            return self.tr.step(to64(batch), to64(noise))

    def params(self):
        return {nb_name(k): v.detach().numpy() for k, v in self.tr.params.items()}

    def grads(self):
        return {nb_name(k): v.grad.numpy() for k, v in self.tr.params.items()}
