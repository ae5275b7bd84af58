"""Helpers of ``tests/test_eval_trace_cpu.py``: the whole-set evaluators (``_EvalGraph`` as one replay and as one rank's row
shard, ``_ChunkedEval``) built and run on the CPU stand-ins, recorded call by call.  A trace holds, in order,

  * every call of a ``drvae_amd.kernels`` launcher made from the evaluator's constructor to the end of ``run()`` (the loss
    pass that builds the plan, the warm-up of the sequences, the pass under capture, the finalising sequence, ``run()``);
  * between those calls -- from the first one on: what a constructor reads off the data set's flags before it launches
    anything (index lists, the chunk partition) is host set-up, not a sequence -- every torch op that writes tensor data -- ``copy_``, ``index_select``, ``index_copy_``, ``zero_``,
    ``add_``, ``sum``, ``stack``, ``repeat``, dtype conversions ...: what becomes a node of a captured graph.  Views, metadata
    ops and whatever a stand-in launcher issues itself are left out.  So are the plain factories (``zeros``, ``empty``,
    ``full``, ``*_like`` ...): WHERE a buffer is allocated is not behaviour, a buffer is known by its first use;
  * the events of the three inert stand-ins of ``torch.cuda`` (``CUDAGraph`` / ``graph`` / ``synchronize``): where a capture
    begins and ends, which graph ``run()`` replays and when, and the all-reduce of the sharded evaluation.

A tensor is described by [number of its storage in order of first appearance, offset, shape, strides, dtype]: aliasing and
layout count, the names of the attributes that hold the buffers do not.  Scalars as in ``tests/fold_trace.describe``.

``python -m tests.eval_trace`` writes ``tests/golden/eval_trace.json``: per case the names of the calls in full and a
digest of each call's arguments -- the first call that differs is named by the test.  The golden file is the recording of
the commit in front of ``drvae_amd/evaluate.py`` (the evaluators still at the end of ``fit.py``); the restructured
evaluators keep it call for call."""
import contextlib
import functools
import hashlib
import json
import os
import warnings

import numpy as np
import torch
from torch.utils._python_dispatch import TorchDispatchMode
from torch.utils._pytree import tree_flatten

from tests import eval_zinb_ref, gene_batch_ref, kernel_ref
from tests.fold_trace import HELPERS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'eval_trace.json')
_FACTORIES = {'empty_like', 'zeros_like', 'ones_like', 'full_like', 'new_empty', 'new_zeros', 'new_ones', 'new_full',
              'new_empty_strided', 'empty_strided'}

# name -> (model kind, model keywords, data-set keywords)
_COUNTS = dict(x_transform='log1p', library_size=True)
VARIANTS = {
    'drvae': ('drvae', {}, {}),
    'pvae': ('pvae', {}, {}),
    'vfae': ('vfae', {}, {}),
    'vfae_use_s': ('vfae', dict(dim_s=2, use_s=True), dict(classes=2)),
    'drvae_nb': ('drvae', dict(type_rec='nb'), dict(counts=True)),
    'drvae_cont': ('drvae', dict(type_y='cont'), dict(cont=True)),
    'drvae_zinb': ('drvae', dict(type_rec='zinb', **_COUNTS), dict(counts=True)),
    'drvae_nb_gene': ('drvae', dict(type_rec='nb', dispersion='gene', **_COUNTS), dict(counts=True)),
    'drvae_zinb_gene_batch': ('drvae', dict(type_rec='zinb', dispersion='gene-batch', use_s=True, dim_s=2, **_COUNTS),
                              dict(counts=True, classes=2)),
    'drvae_no_x2': ('drvae', {}, dict(no_x2=True)),
    'drvae_no_labels': ('drvae', {}, dict(no_y=True)),              # (the sort-and-scan fallback of the metrics)
    'vfae_supervised_only': ('vfae', dict(semi_supervised=False), {}),      # (``sel`` is set; X = 13: the padded x1 rows)
}
ROUTES = ('one', 'dp0', 'dp1', 'chunk5')


def dataset(kind, n=12, X=13, counts=False, cont=False, classes=1, no_x2=False, no_y=False):
    """the 12-row host data set of ``tests/test_eval_chunks_cpu._host_dataset``, with the switches the variants need"""
    from drvae_amd import data as D
    rs = np.random.RandomState(0)
    t = torch.from_numpy
    draw = (lambda: rs.poisson(3.0, (n, X)).astype(np.float32)) if counts else (lambda: rs.randn(n, X).astype(np.float32))
    x1, x2 = t(draw()), t(draw())
    s = t(rs.randint(0, classes, n).astype(np.int64))
    y = t(rs.randn(n, 2).astype(np.float32)) if cont else t(rs.randint(0, 2, n))
    hx = t(((np.arange(n) % 3 == 0) & (not no_x2)).astype(np.int64))
    hy = t(((np.arange(n) % 4 != 1) & (not no_y)).astype(np.int64))
    if kind == 'vfae':
        return D.VFAEDataset(x1, s, y, hy)
    return D.DrVAEDataset(x1, x2, s, y, hx, hy)


def recon_rows(rows, ll, x, mu, sd, *, kind=None, size_from=None, rec_out=None, **kw):
    """``kernel_ref.recon_rows`` plus the zero-inflated kind it leaves out (``tests/eval_zinb_ref.py``: ``sd`` = [theta | logit])"""
    if kind != 'zinb':
        return kernel_ref.recon_rows(rows, ll, x, mu, sd, kind=kind, size_from=size_from, rec_out=rec_out, **kw)
    X = mu.shape[1]
    ref = eval_zinb_ref.reference(x, mu, sd[:, :X], sd[:, X:], size_from)
    rows.copy_(ref['rows'].to(rows.dtype))
    if ll is not None:
        ll.copy_(ref['ll'].to(ll.dtype))
    if rec_out is not None:
        rec_out.copy_(ref['rec'].to(rec_out.dtype))


def model_of(kind, **kw):
    """``tests.test_dropout_cpu.tiny_model``; the supervised-only VFAE (which it has no switch for) with the same sizes"""
    from tests.test_dropout_cpu import tiny_model
    if 'semi_supervised' not in kw:
        return tiny_model(kind, **kw)
    from drvae_amd.VFAE import VFAE
    common = dict(dim_x=13, dim_s=1, dim_y=2, dim_h_en_z1=[7], dim_h_de_x=[8], dim_z1=5, type_rec='diag_gaussian',
                  nonlinearity='elu', learning_rate=5e-3, L=2, weight_decay=0.01, add_noise_var=0.01, use_MMD=False,
                  random_seed=5, epochs=2, batch_size=8, device='cpu')
    common.update(kw)
    return VFAE(dim_h_de_z1=[6], dim_h_en_z2=[6], dim_h_clf=[], dim_z2=4, **common)


class Recorder(TorchDispatchMode):
    """the calls of one evaluator, in order: [name, described arguments]"""

    def __init__(self):
        super().__init__()
        self.calls, self.depth, self.started = [], 0, False
        self.storages, self.alive = {}, []
        self.graphs = []

    # ---------------------------------------------------------------- describing
    def tensor(self, t):
        if t.numel() == 0:
            sid = 'empty'
        else:
            st = t.untyped_storage()
            sid = self.storages.get(st._cdata)
            if sid is None:
                sid = self.storages[st._cdata] = len(self.storages)
                self.alive.append(st)          # (a freed storage's address could come back as another buffer's)
        return [sid, t.storage_offset(), list(t.shape), list(t.stride()), str(t.dtype).replace('torch.', '')]

    def describe(self, a):
        if torch.is_tensor(a):
            return self.tensor(a)
        if isinstance(a, dict):
            return {str(k): self.describe(v) for k, v in sorted(a.items())}
        if isinstance(a, (list, tuple)):
            return [self.describe(v) for v in a]
        if isinstance(a, float):
            return repr(float(a))
        if a is None or isinstance(a, (bool, int, str)):
            return a
        if isinstance(a, (torch.dtype, torch.device, torch.memory_format, torch.layout)):
            return str(a)
        return type(a).__name__

    def note(self, name, *what):
        if self.started:
            self.calls.append([name, self.describe(what)])

    # ---------------------------------------------------------------- the launchers and the stand-ins of torch.cuda
    def launcher(self, name, fn, *a, **kw):
        if self.depth == 0:
            self.started = True
            self.note('K.' + name, a, kw)
        self.depth += 1
        try:
            return fn(*a, **kw)
        finally:
            self.depth -= 1

    def install(self, mp):
        import drvae_amd.kernels as K
        import drvae_amd.dist as D
        import drvae_amd.gene_batch_rows as GB
        import drvae_amd.gene_rows as G
        rec = self
        mp.setattr(K, 'recon_rows', recon_rows)
        for name in kernel_ref.FUNCTIONS:
            if name not in HELPERS:
                mp.setattr(K, name, functools.partial(self.launcher, name, getattr(K, name)))
        mp.setattr(G, 'gene_rows', functools.partial(self.launcher, 'gene_rows', G.gene_rows))
        mp.setattr(GB, 'gene_batch_rows', functools.partial(self.launcher, 'gene_batch_rows', GB.gene_batch_rows))
        mp.setattr(D, 'allreduce_sum', functools.partial(self.launcher, 'allreduce_sum', D.allreduce_sum))

        class Graph:
            def __init__(self):
                rec.graphs.append(self)

            def replay(self):                   # (inert: the trace is about what is launched, not about values)
                rec.note('graph.replay', [i for i, g in enumerate(rec.graphs) if g is self][0])

        @contextlib.contextmanager
        def capture(g, *a, **kw):
            n = [i for i, h in enumerate(rec.graphs) if h is g][0]
            rec.note('capture.begin', n)
            yield
            rec.note('capture.end', n)

        mp.setattr(torch.cuda, 'CUDAGraph', Graph)
        mp.setattr(torch.cuda, 'graph', capture)
        mp.setattr(torch.cuda, 'synchronize', lambda *a, **kw: rec.note('synchronize'))

    # ---------------------------------------------------------------- torch ops
    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        out = func(*args, **kwargs)
        if self.depth:
            return out
        schema = func._schema
        if any(r.alias_info is not None and not r.alias_info.is_write for r in schema.returns):
            return out                                                      # a view
        outs = [o for o in tree_flatten(out)[0] if torch.is_tensor(o)]
        if not schema.is_mutable and not outs:
            return out                                                      # metadata, a scalar for the host
        if func.overloadpacket.__name__ in _FACTORIES or \
                not any(torch.is_tensor(a) for a in tree_flatten((args, kwargs))[0]):
            return out                                                      # a factory
        self.note(str(func), args, kwargs, out)
        return out


def make(variant):
    """(model, data set) of a variant: a fresh model, outside the recording"""
    kind, mkw, dkw = VARIANTS[variant]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return model_of(kind, **mkw), dataset(kind, **dkw)


def build(model, ds, route):
    """the evaluator of a route, inside the caller's stand-ins"""
    from drvae_amd.fit import _ChunkedEval, _EvalGraph
    sig = ('trace', route)
    if route == 'chunk5':
        return _ChunkedEval(model, ds, 5, sig)
    return _EvalGraph(model, ds, sig, dp=None if route == 'one' else (int(route[2:]), 2))


def trace(variant, route):
    """-> {'names': [...], 'digests': [...], 'calls': [[name, arguments], ...]} of one case"""
    import pytest
    with pytest.MonkeyPatch.context() as mp:
        gene_batch_ref.install(mp)               # (``kernel_ref.install`` and the two gene-wise dispersion launches)
        rec = Recorder()
        rec.install(mp)
        model, ds = make(variant)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            with rec:
                build(model, ds, route).run()
    calls = json.loads(json.dumps(rec.calls))
    digest = lambda c: hashlib.sha1(json.dumps(c[1], sort_keys=True, separators=(',', ':')).encode()).hexdigest()[:8]
    return dict(names=[c[0] for c in calls], digests=[digest(c) for c in calls], calls=calls)


def pack(tr):
    """a trace as it is stored: the names in full (indices into their table), the digests joined"""
    table = sorted(set(tr['names']))
    return dict(table=table, names=[table.index(n) for n in tr['names']], digests=''.join(tr['digests']))


def unpack(stored):
    d = stored['digests']
    return dict(names=[stored['table'][i] for i in stored['names']], digests=[d[i:i + 8] for i in range(0, len(d), 8)])


if __name__ == '__main__':
    out, left_out = {}, []
    for v in VARIANTS:
        for r in ROUTES:
            try:
                out['%s/%s' % (v, r)] = pack(trace(v, r))
            except Exception as e:              # a case that does not build on the recorded commit is left out
                left_out.append('%s/%s: %s: %s' % (v, r, type(e).__name__, str(e)[:200]))
    with open(GOLDEN, 'w') as f:
        json.dump(out, f, separators=(',', ':'), sort_keys=True)
    print('wrote', GOLDEN, os.path.getsize(GOLDEN), 'bytes,', len(out), 'cases')
    for line in left_out:
        print('left out:', line)
