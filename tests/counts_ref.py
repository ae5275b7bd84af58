"""Float64 references of the raw-count inputs (``x_transform='log1p'``, ``library_size=True``): the split feed
(``dv_batch_feed`` with ``xt``), the library-scaled reconstruction rows (``dv_rec_nll_rows``, kinds ``DV_REC_POISSON_LIB`` /
``DV_REC_NEGBIN_LIB``) with both gradients, the bounds they are held to, fp32 emulations -- a careful one and three faulty ones
the bounds catch -- and a model-level float64 reference of one step.  Test-only; builds on ``tests/nb_ref.py``.

The size factor.  s = max(sum_g x_g, 1) / X.  For integer counts with a row total below 2^24 every partial sum is an integer
below 2^24, exact in fp32 in any order, so the kernel's s is ONE correctly rounded fp32 quotient whatever the path;
``size_factor32`` forms the same number on the host and the references take it as data, like the heads' fp32 values.

The split feed.  ``xt`` is the source row, bit for bit.  The encoder's row is fmaf(sigma, eps, log1p(x)): the project's count
for ``log1p`` (3, a transcendental: the tally of ``tests/nb_ref.py``) plus one for the fused product-sum, C = 4, on the
components |log1p x| + |sigma eps|.  Without a transform the row is the plain feed's fmaf(sigma, eps, x): C = 1.

The library rows.  With m = s v (v the mean head's fp32 output) the float64 terms are those of ``nb_ref`` at m, and

    d/da_m = d/dm * s * slope(v - shift) = (x - m) / (v (1 + m / theta)) * slope(v - shift),      d/da_t as in nb_ref, at m.

The kernel's m is fl(s v): ONE rounding more than ``nb_ref`` counts, in front of everything it counts.  Behind that rounding
the kernel runs nb_ref's operations on the rounded m (the same C_ROW / C_GM / C_GT on the same components: in d/da_m the
divisor m (1 + m/theta) became v (1 + m/theta) and the slope's argument v - shift, operation for operation), so the bound is
nb_ref's plus what one relative perturbation U of m moves each result by, |m d(result)/dm| U:

* row:     m dlogp/dm           = (x - m) / (1 + m/theta)                        -> U |x - m| / (1 + m/theta)   per element;
* d/da_m:  with h(m) = theta (x - m) / (theta + m), h'(m) = -theta (theta + x) / (theta + m)^2
                                                                                 -> U |c| slope / v * m theta (theta + x) / (theta + m)^2;
* d/da_t:  d/dm [log(theta/(theta+m)) + (m - x)/(theta + m)] = (x - m) / (theta + m)^2
                                                                                 -> U |c| slope_t * m |x - m| / (theta + m)^2.

Poisson (``tests/test_gpu_numerics.py``: C = 16 for the row terms and for the gradient): the row is x log m - m - lgamma(x+1)
at m = fl(s v), plus U |x - m| for the one rounding (m dlogp/dm = x - m); the gradient (x / v - s) * slope(v - shift) holds no
m at all: C = 16 on the components (x / v + s), nothing added."""
import contextlib
import dataclasses

import numpy as np
import torch

from tests import nb_ref as R
from tests import ref64
from tests.ref64 import U, bound, f64, row_sum_bound

C_LOG1P, C_FMA = 3, 1
C_ENC = C_LOG1P + C_FMA         # the encoder rows with the transform
C_POIS = 16                     # tests/test_gpu_numerics.py::test_rec_nll_poisson_small_rates


# ------------------------------------------------------------------------------------------------ size factor
def size_factor32(x):
    """the fp32 size factor of every row of ``x`` (rows of integer counts, total < 2^24): one correctly rounded quotient"""
    x = np.asarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x, np.float64)
    tot = x.sum(1)
    assert np.all(tot < 2 ** 24) and np.all(x == np.floor(x)) and np.all(x >= 0)
    return (np.maximum(tot, 1.0).astype(np.float32) / np.float32(x.shape[1])).astype(np.float32)


def size_factor64(x):
    """float64, differentiable-free torch form (model level): max(sum, 1) / X per row"""
    return torch.clamp(x.sum(1), min=1.0) / x.shape[1]


# ---------------------------------------------------------------------------------------------------- the feed
def feed_reference(src, noise=None, sigma=0.0, transform='log1p'):
    """``src``: the gathered source rows (fp32).  Returns (xt, xin64, xin_bound): the targets (the rows themselves), the
    encoder's rows in float64 and their bound"""
    x = f64(src)
    t = torch.log1p(x) if transform == 'log1p' else x
    e = f64(ref64.f32(sigma)) * f64(noise) if noise is not None else torch.zeros_like(x)
    C = C_ENC if transform == 'log1p' else C_FMA
    return src.clone(), t + e, bound(C, t.abs() + e.abs())


# ---------------------------------------------------------------------------------------------------- the rows
def reference(kind, x, v_mu, v_theta=None, coef=None, shift=R.MU_SHIFT, s=None):
    """everything the library-rows tests compare with, from the exact fp32 values the kernel received.  ``x``: the TARGET row of
    every decoder row (already gathered through ``xidx``); ``s``: fp32 size factors per row (default: those of ``x``).
    ``kind``: 'nb' | 'poisson'.  Keys as ``nb_ref.reference``: ll, rows, rows_bound, gm, gm_bound[, gt, gt_bound]"""
    X = x.shape[1]
    s32 = size_factor32(x) if s is None else np.asarray(s, np.float32)
    S = f64(s32)[:, None]
    xx, V = f64(x), f64(v_mu)
    m = S * V
    c = f64(coef)[:, None] if coef is not None else None
    ym = V - ref64.f32(shift)
    sm = ref64.dact_from_y('softplus', ym)
    cond_m = sm + ym.abs() * ref64.dact_from_y_slope('softplus', ym)
    out = dict(s=S, m=m)
    if kind == 'poisson':
        lgam = torch.lgamma(xx + 1)
        xl = xx * torch.log(m)
        comps = xl.abs() + m + lgam
        out['ll'] = xl - m - lgam
        out['ll_bound'] = bound(C_POIS, comps) + U * (xx - m).abs()
        out['rows'] = out['ll'].sum(1)
        out['rows_bound'] = out['ll_bound'].sum(1) + row_sum_bound(comps, X)
        if coef is not None:
            out['gm'] = c * (xx / V - S) * sm
            out['gm_bound'] = bound(C_POIS, c.abs() * (xx / V + S) * cond_m)
        return out
    th = f64(v_theta)
    pair, lx, tl, xl = R.logp_terms(xx, m, th)
    comps = pair.abs() + lx + tl.abs() + xl.abs()
    out['ll'] = pair - lx + tl + xl
    out['comps'] = comps
    out['ll_bound'] = bound(R.C_ROW, comps) + U * (xx - m).abs() / (1 + m / th)
    out['rows'] = out['ll'].sum(1)
    out['rows_bound'] = out['ll_bound'].sum(1) + row_sum_bound(comps, X)
    if coef is not None:
        gm, gt, gm_c, gt_c = R.grads64(xx, m, th)
        yt = th - ref64.f32(R.THETA_SHIFT)
        st = ref64.dact_from_y('softplus', yt)
        out['gm'], out['gt'] = c * gm * S * sm, c * gt * st
        out['gm_bound'] = bound(R.C_GM, c.abs() * S * gm_c * cond_m) + \
            U * c.abs() * sm / V * m * th * (th + xx) / (th + m) ** 2
        out['gt_bound'] = bound(R.C_GT, c.abs() * gt_c * (st + yt.abs() * ref64.dact_from_y_slope('softplus', yt))) + \
            U * c.abs() * st * m * (xx - m).abs() / (th + m) ** 2
    return out


def grads_autograd(kind, x, a_m, a_t, s, shift=R.MU_SHIFT):
    """d sum log p / d(a_m, a_t) by float64 autograd through m = s * (softplus(a_m) + shift) (the cross-check of the closed forms)"""
    import torch.nn.functional as F
    am = a_m.clone().requires_grad_(True)
    m = s[:, None] * (F.softplus(am) + shift)
    if kind == 'poisson':
        (x * torch.log(m) - m - torch.lgamma(x + 1)).sum().backward()
        return am.grad, None
    at = a_t.clone().requires_grad_(True)
    R.logp64(x, m, F.softplus(at) + R.THETA_SHIFT).sum().backward()
    return am.grad, at.grad


# ------------------------------------------------------------------------------------------ fp32 emulations
def emulate_fp32(x, v, theta, s, shift=R.MU_SHIFT, slope='head', factor_s=True):
    """the library NB row formula in numpy float32, operation by operation: (log p, d/da_m, d/da_t) per element; ``s``: fp32
    per row.  Careful = the kernel's construction: m = fl(s v), ``nb_ref.emulate_fp32`` at m for the row and d/da_t, and
    d/da_m = (x - m) / (v (1 + m/t)) * slope(v - shift).  FAULTY on purpose: ``slope='scaled'`` (the slope taken from the scaled
    mean, slope(m - shift)); ``factor_s=False`` (d/dm times the slope, the factor s = dm/dv forgotten)"""
    f = np.float32
    x, v, t = R._f(x), R._f(v), R._f(theta)
    s = R._f(s).reshape(-1, 1)
    with np.errstate(all='ignore'):
        m = (s * v).astype(f)
        ll, _, gt = R.emulate_fp32(x, m, t, shift=shift)
        sl = -np.expm1(-((m if slope == 'scaled' else v) - f(shift)))
        div = (v if factor_s else m) * (f(1) + m / t)
        gm = ((x - m) / div * sl).astype(f)
    assert ll.dtype == f and gm.dtype == f and gt.dtype == f
    return ll, gm, gt


# ------------------------------------------------------------------------------- model-level float64 reference
@contextlib.contextmanager
def oracle_as_counts(spec, x_transform=None, library_size=False):
    """inside: ``oracle.models_ref`` driven with the Gaussian-shaped ``spec`` IS the negative-binomial model with the raw-count
    switches, in float64 (``nb_ref.oracle_as_nb`` plus three run-time substitutions; nothing under oracle/ changes):

    * the oracle adds its input noise to ``x`` BEFORE encoder and likelihood both read it; here it is driven with
      ``add_noise_var = 0`` (encoder and likelihood see the raw rows) and the ENCODER's first input becomes
      T(x) + sigma * eps, with the rows of ``nx1`` on the first encoder pass of a data group and ``nx2`` on the second;
    * the row log-likelihood is evaluated at the size-scaled mean, s from the raw target row it is handed."""
    from oracle import blocks_ref as B
    from oracle import models_ref as M
    sigma = float(spec.add_noise_var)
    state = {}
    saved = (M._group_losses, B.diag_gaussian)

    def group_losses(spec_, p, acc, idx, x1, x2, y, noise, iters, training, s=None):
        state.update(idx=idx, noise=noise, training=training, n=0)
        return saved[0](dataclasses.replace(spec_, add_noise_var=0.0), p, acc, idx, x1, x2, y, noise, iters, training, s=s)

    def diag_gaussian(inputs, p, prefix, *a, **k):
        if prefix == 'encoder_z1':
            x = inputs[0]
            t = torch.log1p(x) if x_transform == 'log1p' else x
            if state['training'] and sigma > 0.:
                key = ('nx1', 'nx2')[state['n']]
                t = t + torch.as_tensor(np.asarray(state['noise'][key], np.float64))[state['idx']] * sigma
            state['n'] += 1
            inputs = [t] + list(inputs[1:])
        return saved[1](inputs, p, prefix, *a, **k)

    with R.oracle_as_nb():
        rows = B.logp_sigma_rows
        if library_size:
            B.logp_sigma_rows = lambda x, mu, theta: rows(x, mu * size_factor64(x)[:, None], theta)
        M._group_losses, B.diag_gaussian = group_losses, diag_gaussian
        try:
            yield
        finally:
            M._group_losses, B.diag_gaussian = saved
            B.logp_sigma_rows = rows


def count_batch(spec, n_rows, seed=3, depth_decades=1.0):
    """``nb_ref.count_batch`` with the rows' depths spread log-uniformly over ``depth_decades`` (floor of the scaled counts:
    still integers), so that the size factors differ from row to row"""
    b = R.count_batch(spec, n_rows, seed=seed)
    rs = np.random.RandomState(seed + 2000)
    d = 10 ** rs.uniform(-depth_decades / 2, depth_decades / 2, n_rows).astype(np.float32)
    for k in ('x1', 'x2'):
        b[k] = np.floor(b[k] * d[:, None]).astype(np.float32)
    return b


class ModelRef(R.ModelRef):
    """``nb_ref.ModelRef`` with the switches: every call inside ``oracle_as_counts``"""

    def __init__(self, spec, seed=9, x_transform=None, library_size=False):
        super().__init__(spec, seed)
        self.sw = dict(x_transform=x_transform, library_size=library_size)

    @contextlib.contextmanager
    def context(self):
        with oracle_as_counts(self.spec, **self.sw):
            yield

    def loss(self, batch, noise, training=True, counts=None):
        with self.context():
            return self.tr.loss(R.to64(batch), R.to64(noise), training, **(dict(counts=counts) if counts else {}))

    def step(self, batch, noise, counts=None):
        with self.context():
            return self.tr.step(R.to64(batch), R.to64(noise), **(dict(counts=counts) if counts else {}))


# ------------------------------------------------------- the riders on top: dropout, clipping, annealing, the average
CHAIN_BLOCK = {'c_enc': 'encoder_z1', 'c_decx': 'decoder_x', 'c_dz1': 'decoder_z1', 'c_clf': 'encoder_y'}      # + 'c_top'


def chain_block(spec, chain):
    """the oracle's block behind a chain of the engine (``FusedStep.dropout_sites()[i]['chain']``)"""
    return ('encoder_z2' if spec.kind == 'vfae' else 'encoder_z3') if chain == 'c_top' else CHAIN_BLOCK[chain]


class RidersRef(ModelRef):
    """``ModelRef`` with the step's riders, each from the float64 piece its own round tests it with:

    * hidden-layer dropout with COLUMN masks (``tests/test_dropout_cpu.py``'s: one keep vector per site, the same in every row,
      so the engine's stacking of rows does not enter): the trunk output of block b is multiplied by cols[b] / keep in a
      training pass -- every block here has one hidden layer, its site is the heads' input;
    * the annealed ELBO / CMPL recombined from the oracle's pieces (``tests/anneal_ref.recombine``), differentiated as such;
    * torch's ``clip_grad_norm_`` in float64 between backward and the optimiser (the record of ``tests/clip_ref.py``:
      coef = min(1, max_norm / (norm + 1e-6)));
    * the average e += (1 - d)(p_new - e) behind every step, started at the parameters (``tests/avg_ref.ref_avg``)."""

    def __init__(self, spec, seed=9, x_transform=None, library_size=False, sched=None, max_grad_norm=None, ema_decay=None,
                 keep=1.0, cols=None):
        from tests import anneal_ref as AR
        super().__init__(spec, seed, x_transform, library_size)
        self.sched = AR.settings(**(sched or {}))
        self.max_norm, self.decay, self.keep, self.cols = max_grad_norm, ema_decay, float(keep), dict(cols or {})
        self.avg = {k: v.detach().clone() for k, v in self.tr.params.items()}
        self._training = True

    @contextlib.contextmanager
    def context(self):
        from oracle import blocks_ref as B
        with super().context():
            mlp = B.mlp

            def dropped(inputs, p, prefix, n_hidden, nonlin):
                h = mlp(inputs, p, prefix, n_hidden, nonlin)
                block = prefix[:-len('.nnet')]
                if self._training and block in self.cols:
                    assert n_hidden == 1
                    h = h * (torch.as_tensor(np.asarray(self.cols[block], np.float64)) / self.keep)[None, :]
                return h
            B.mlp = dropped
            try:
                yield
            finally:
                B.mlp = mlp

    def loss(self, batch, noise, training=True, counts=None):
        from tests import anneal_ref as AR
        self._training = training
        losses, rows = super().loss(batch, noise, training, counts)
        return AR.recombine(self.spec, self.sched, losses, self.tr.iters), rows

    def step(self, batch, noise, counts=None):
        from tests import anneal_ref as AR
        tr = self.tr
        tr.opt.zero_grad()
        losses, rows = self.loss(batch, noise, True, counts)
        with self.context():
            losses['CMPL'].backward()
        if self.max_norm is not None:
            torch.nn.utils.clip_grad_norm_(list(tr.params.values()), self.max_norm, norm_type=2)
        tr.opt.param_groups[0]['lr'] = AR.spec_coefficients(self.spec, tr.iters, self.sched)['lr_scale'] * self.spec.learning_rate
        tr.opt.step()
        tr.iters += 1
        if self.decay is not None:
            for k, v in tr.params.items():
                self.avg[k] += (1.0 - self.decay) * (v.detach() - self.avg[k])
        return losses, rows

    def averaged(self):
        return {R.nb_name(k): v.numpy() for k, v in self.avg.items()}
