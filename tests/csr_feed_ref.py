"""Test-only helpers of the sparse (CSR) batch feed: the CPU stand-in of the launch -- densify the selected rows, then the
existing ``tests/kernel_ref.batch_feed`` --, the case generator of the kernel grid (row layouts x widths), and the step driver
the CPU and the GPU tests share (a model trained on a ``CsrRows`` dataset against the same model on the densified one).

What is held to what.  Integer counts: the sparse launch writes the BITS of the dense launch on the densified matrix (``xin``,
``xt``, every label output).  Non-integer values: ``xt`` and the transforms 0 / 1 still bit for bit (elementwise operations on
the same staged values); transform 3 sums rows wider than 1024 columns from the CSR values, another order than the dense
walk, so it is held to the float64 reference and the bound of ``tests/depth_ref.py`` as they are (``norm_reference``).  That
bound (C_NORM = 5 roundings on |T| + |sigma eps|) is derived for a size factor that is ONE correctly rounded quotient, i.e. for
a row total that fp32 sums exactly in any order -- ``counts_ref.size_factor32`` refuses anything else.  The non-integer rows it
is applied to therefore lie on a grid of 1/4 with totals below 2^22 (``layout(..., integer=False, grid=4)``): every partial sum
is a multiple of 1/4 below 2^22, exact in fp32, and the premise holds.  Values off any grid make s depend on the order of the
sum -- for the dense launch as much as for this one -- which that bound does not cover; such rows are used where no sum is
taken (``xt``, transforms 0 / 1) and where the order is the dense launch's (transform 3 up to 1024 columns: equal bits)."""
import numpy as np
import torch

from tests import depth_ref as DR
from tests import kernel_ref
from tests import ref64

XS = (1, 3, 4, 255, 978, 1024, 1028, 2052, 4100)       # every width at which the kernel changes path; 4100: five chunks
SEAMS = (1023, 1024, 2047, 2048, 4095, 4096)            # both columns of every chunk seam
LAYOUTS = ('empty', 'full', 'p07', 'gap', 'first', 'last', 'seams')
N_SRC = 7


class _Rows:
    """what ``kernel_ref.batch_feed`` indexes: ``x[rows]`` densifies the selected rows of the CSR matrix"""

    def __init__(self, csr):
        self.csr = csr

    def __getitem__(self, rows):
        return self.csr.to_dense(rows)


def batch_feed(xin, x1, x2, *args, **kw):
    """CPU stand-in of ``kernels.batch_feed`` with ``CsrRows`` operands: the dense stand-in on the densified selected rows"""
    from drvae_amd.sparse_rows import CsrRows
    sparse = [isinstance(x, CsrRows) for x in (x1, x2)]
    kernel_ref.CALLS['csr_feed'] = kernel_ref.CALLS.get('csr_feed', 0) + any(sparse)
    return kernel_ref.batch_feed(xin, _Rows(x1) if sparse[0] else x1, _Rows(x2) if sparse[1] else x2, *args, **kw)


def install(monkeypatch):
    """every CPU stand-in (``gene_batch_ref.install``: ``kernel_ref``'s and the gene-wise row passes') with the feed's replaced
    by the one that takes sparse rows"""
    import drvae_amd.kernels as K
    from tests import gene_batch_ref
    gene_batch_ref.install(monkeypatch)
    kernel_ref.CALLS['csr_feed'] = 0
    monkeypatch.setattr(K, 'batch_feed', batch_feed)


# ------------------------------------------------------------------------------------------------- the kernel grid
def norm_reference(rows, noise=None, sigma=0.0):
    """``depth_ref.feed_reference`` for rows whose totals fp32 sums exactly without being integers (multiples of 1/4, totals
    below 2^22): the same float64 formula and the same bound, s the one correctly rounded quotient.  Returns (xin64, bound)"""
    x = ref64.f64(rows)
    tot = x.sum(1).numpy()
    assert np.all(x.numpy() * 4 == np.floor(x.numpy() * 4)) and np.all(tot < 2 ** 22) and np.all(x.numpy() >= 0)
    s = (np.maximum(tot, 1.0).astype(np.float32) / np.float32(x.shape[1])).astype(np.float32)
    t = torch.log1p(x / ref64.f64(s)[:, None])
    e = ref64.f64(ref64.f32(sigma)) * ref64.f64(noise) if noise is not None else torch.zeros_like(x)
    return t + e, ref64.bound(DR.C_NORM, t.abs() + e.abs())


def layout(name, X, seed=0, integer=True, grid=None):
    """``N_SRC`` source rows of width ``X`` (dense fp32) in the named layout.  Integer counts with totals below 2^22, or
    (``integer=False``) positive non-integer values -- any fp32 values, or with ``grid`` = g multiples of 1/g"""
    rs = np.random.RandomState(seed * 131 + X)
    full = rs.poisson(rs.gamma(2.0, 40.0, (N_SRC, X))).astype(np.float32) + 1.0
    if not integer:
        full = (full * rs.uniform(0.3, 1.7, full.shape)).astype(np.float32)
        if grid:
            full = (np.floor(full * grid) + 1).astype(np.float32) / np.float32(grid)
            assert not np.all(full == np.floor(full))
    assert full.astype(np.float64).sum(1).max() < 2 ** 22 and full.min() > 0
    x = np.zeros_like(full)
    if name == 'empty':
        pass
    elif name == 'full':
        x = full
    elif name == 'p07':
        keep = rs.uniform(size=full.shape) < 0.07
        x = np.where(keep, full, 0).astype(np.float32)
    elif name == 'gap':                 # an empty row between two full ones, then the pattern again
        x = full.copy()
        x[1::2] = 0
    elif name == 'first':
        x[:, 0] = full[:, 0]
    elif name == 'last':
        x[:, X - 1] = full[:, X - 1]
    elif name == 'seams':
        cols = [c for c in SEAMS if c < X] or [0, X - 1]
        x[:, cols] = full[:, cols]
    else:
        raise KeyError(name)
    return x


def to_csr_dataset(ds, which=('x1', 'x2')):
    """the dataset with the named matrices as ``CsrRows`` (the other fields shared)"""
    from drvae_amd import data as D
    from drvae_amd.sparse_rows import CsrRows
    conv = lambda k: CsrRows.from_dense(getattr(ds, k)) if k in which else getattr(ds, k)
    if isinstance(ds, D.VFAEDataset):
        return D.VFAEDataset(conv('x1'), ds.s, ds.y, ds.has_y)
    return D.DrVAEDataset(conv('x1'), conv('x2'), ds.s, ds.y, ds.has_x2, ds.has_y)


def counts_dataset(kind, n, X, seed, dev='cpu', n_s=1, density=0.3):
    """sparse integer counts: Gamma-Poisson entries kept with probability ``density``, x2 only on the pair rows"""
    from drvae_amd import data as D
    rs = np.random.RandomState(seed)
    y = rs.randint(0, 2, n)
    hx = (np.arange(n) % 3 == 0).astype(np.int64)
    hy = (np.arange(n) % 4 != 1).astype(np.int64)
    s = rs.randint(0, n_s, n)
    draw = lambda: (rs.poisson(rs.gamma(2.0, 2.0, (n, X))) * (rs.uniform(size=(n, X)) < density)).astype(np.float32)
    x1, x2 = draw(), draw() * hx[:, None].astype(np.float32)
    x1[1] = 0                                        # (an empty row in the set)
    t = lambda a: torch.from_numpy(a).to(dev)
    if kind == 'vfae':
        return D.VFAEDataset(t(x1), t(s), t(y), t(hy))
    return D.DrVAEDataset(t(x1), t(x2), t(s), t(y), t(hx), t(hy))


# ------------------------------------------------------------------------------------------------- the step
STEP_MODELS = {
    'drvae-nb': ('drvae', dict(type_rec='nb', x_transform='log1p', library_size=True), {}),
    'pvae-zinb-norm': ('pvae', dict(type_rec='zinb', x_transform='log1p_norm'), {}),
    'vfae-use_s-gene-batch': ('vfae', dict(type_rec='nb', x_transform='log1p', library_size=True, use_s=True, dim_s=2,
                                           dispersion='gene-batch'), dict(mode='sampler', carry_s='masked')),
    'drvae-gauss': ('drvae', {}, dict(mode='stratified')),         # (a Gaussian model: the plain feed)
}


def trajectory(name, ds, how, dev='cpu', steps=3, table=None, batch=8, **model_kw):
    """``steps`` train steps of the model ``name`` of ``STEP_MODELS`` on ``ds`` through a ``DeviceBatcher``; ``how``: 'eager' /
    'captured' (the epoch feed; ``table``: the epoch's table given instead of drawn) or 'feed' (``feed()`` with the rows of
    ``table``).  Returns (losses per step, [parameters, first moments, second moments], the epoch's table)"""
    import warnings
    from drvae_amd import data as D
    from tests.test_dropout_cpu import tiny_model
    kind, kw, bat_kw = STEP_MODELS[name]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model = tiny_model(kind, device=dev, dim_x=ds.x1.shape[1], **dict(kw, **model_kw))
    eng = model.engine()
    bat = D.DeviceBatcher(ds, torch.ones(len(ds)), batch, seed=5, **(bat_kw or dict(mode='sampler')))
    bat.bind(eng)
    losses = []
    if how == 'feed':
        for b in range(steps):
            bat.feed(table[b].long())
            eng.train_step()
            losses.append(eng.losses())
    else:
        table = bat.begin_epoch(n_batches=steps, table=table).clone()
        for b in range(steps):
            if how == 'captured':
                if eng._graph_key is None:
                    eng.capture()
                    bat.rebase()
                eng.replay()
            else:
                eng.train_step()
            losses.append(eng.losses())
    if torch.device(dev).type == 'cuda':
        torch.cuda.synchronize()
    a = eng.arena
    return losses, [getattr(a, w).clone() for w in ('param', 'exp_avg', 'exp_avg_sq')], table


def same_trajectory(a, b):
    return a[0] == b[0] and all(torch.equal(p, q) for p, q in zip(a[1], b[1])) and \
        all(np.isfinite(v) for l in a[0] for v in l.values())
