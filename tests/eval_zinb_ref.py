"""Float64 reference of the zero-inflated kind of ``dv_recon_rows`` (``kernels.recon_rows(kind='zinb', ...)``: the whole-set
evaluation of ``type_rec='zinb'`` models), its bounds, test cases and an fp32 emulation -- a careful one and six faulty ones the
bounds catch.  Test-only; nothing here is new arithmetic: it joins ``tests/eval_counts_ref.py`` and ``tests/zinb_ref.py``.

What the launch forms, per target row x[i,:], from the finished mean head v, theta and the RAW dropout logit a:

    r       = v, or fl(s v) with a size source (s = max(sum_g xs[i,g], 1) / X): the NEGATIVE-BINOMIAL mean, never (1 - pi) r
    rows    = the six statistics between x and r                        -- those of kind 'nb': the logit does not enter
    rec_out = r                                                         -- the same
    ll      = sum_g log p_ZINB(x_g | r_g, theta_g, a_g)                 -- ``dv_rec_nll_rows``' kinds DV_REC_ZINB[_LIB]

so ``rows`` / ``rec`` and their bounds are ``eval_counts_ref.reference('nb', ...)``'s as they stand and ``ll`` / ``ll_bound`` are
``zinb_ref.reference(..., library=..., s=...)``'s row sums, with s the fp32 size factor of the size source's rows.  Neither
theta nor the logit is ever scaled."""
import numpy as np
import torch

from tests import counts_ref as CR
from tests import eval_counts_ref as ER
from tests import nb_ref as R
from tests import zinb_ref as Z

FAULTS = ('nb_ll', 'mixture_mean', 'logit_scaled', 'swapped', 'naive_zero', 'll_unscaled')


def reference(x, mu, theta, logit, size_from=None):
    """``rows`` (M, 6), ``ll`` (M), ``rec`` (M, X) and their bounds (``*_bound``), from the exact fp32 values the kernel
    received; ``s``: the fp32 size factors (None without a size source)"""
    nb = ER.reference('nb', x, mu, theta, size_from)
    lib = size_from is not None
    z = Z.reference(x, mu, theta, logit, library=lib, s=nb['s'] if lib else None)
    return dict(rows=nb['rows'], rows_bound=nb['rows_bound'], rec=nb['rec'], rec_bound=nb['rec_bound'], s=nb['s'],
                ll=z['rows'], ll_bound=z['rows_bound'])


def case(M, X, seed=0, scaled=False, other=False, counts='mixed'):
    """fp32 host tensors (x, mu, theta, logit, size_from | None): ``eval_counts_ref.case('nb', ...)`` with at least a third of
    the targets set to zero (row 0 all zero), and logits drawn from ``zinb_ref.LOGITS``.  ``scaled`` without ``other``: the
    size source IS the target tensor; with ``other`` another, deeper matrix (row 0 all zero, row 1 equal to its target)"""
    x, mu, theta, size = ER.case('nb', M, X, seed=seed, scaled=scaled, other=other, counts=counts)
    rs = np.random.RandomState(77 + 1000 * seed + 7 * M + X)
    x = x.clone()
    flat = x.reshape(-1)
    idx = rs.permutation(M * X)[:-(-M * X // 3)]
    flat[torch.from_numpy(idx)] = 0.0
    x[0] = 0.0
    assert float((x == 0).double().mean()) >= 1.0 / 3
    logit = torch.from_numpy(np.asarray(Z.LOGITS, np.float32)[rs.randint(0, len(Z.LOGITS), (M, X))])
    if scaled and not other:
        size = x
    elif scaled:
        size = size.clone()
        if M > 1:
            size[1] = x[1]
    return x, mu, theta, logit, size


def emulate(x, mu, theta, logit, size_from=None, fault=None):
    """the launch in numpy float32, operation by operation -> dict(rows, ll, rec): ``eval_counts_ref.emulate('nb')`` for the
    statistics and the stored mean, ``zinb_ref.emulate_fp32`` for the terms, the kernel's summation order.  ``fault`` None: the
    kernel's construction.  FAULTY on purpose (``FAULTS``): 'nb_ll' (the zero inflation forgotten: the negative binomial's
    terms), 'mixture_mean' (the statistics and the stored mean at (1 - pi) r), 'logit_scaled' (s multiplies the logit),
    'swapped' (the theta and logit blocks exchanged), 'naive_zero' (log(pi + (1 - pi) exp(L0)) at the zeros), 'll_unscaled'
    (the term at the head v, not at s v)"""
    f = np.float32
    assert fault is None or fault in FAULTS
    x, v, t, a = (R._f(w.numpy() if torch.is_tensor(w) else w) for w in (x, mu, theta, logit))
    lib = size_from is not None
    s = CR.size_factor32(size_from) if lib else None
    with np.errstate(all='ignore'):
        if fault == 'swapped':
            t, a = a, t
        base = ER.emulate('nb', x, v, t, size_from)
        out = dict(rows=base['rows'], rec=base['rec'])
        if fault == 'mixture_mean':
            e = np.exp(-np.abs(a))
            q = np.where(a >= 0, e / (f(1) + e), f(1) / (f(1) + e)).astype(f)
            mixed = ER.emulate('nb', x, (q * base['rec']).astype(f), t, None)
            out = dict(rows=mixed['rows'], rec=mixed['rec'])
        if fault == 'nb_ll':
            out['ll'] = base['ll']
            return out
        al = (a * s.reshape(-1, 1)).astype(f) if (fault == 'logit_scaled' and lib) else a
        ll = Z.emulate_fp32(x, v, t, al, s=None if fault == 'll_unscaled' else s,
                            zero='naive' if fault == 'naive_zero' else 'careful')[0]
        out['ll'] = ER._sum32(ll)
    return out
