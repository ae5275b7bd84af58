"""The captured whole-set evaluation behind ``FitMixin.evaluate_performance_on_dataset``.

What ``FitMixin._evaluate`` does step by step -- with a host round trip behind nearly every number: index lists from
``torch.nonzero``, numpy combinations of the reconstruction partials, ``float()`` of every metric -- is recorded here ONCE
into hipGraphs over the dataset's own HBM-resident tensors.  Every evaluator does the same four things:

  1. the evaluation-mode loss scalars of the fused step's forward (Philox draws from the device counter) on a plan of its
     rows, the inputs gathered device-to-device from the dataset;
  2. the means-only inference ``forward`` on the fused step's layer chains (``_Rows.infer``);
  3. per reconstructed matrix the row statistics, log-likelihood rows and column-moment blocks (``_Rows.partials``:
     ``dv_recon_rows`` / ``dv_col_moments``; the count decoders' kinds at the mean scaled by x1's size factor);
  4. the finalising launches: ``dv_recon_finalize`` and ``dv_rank_metrics`` / ``dv_reg_metrics`` (sort + scan beyond the
     pair-counting kernel's range), every scalar into ONE float64 vector that travels to the host in ONE copy.

Three drivers sit on these parts:

  * ``_EvalGraph``, one replay: 1-4 over the whole set in one graph;
  * ``_EvalGraph(dp=(rank, world))``, rows sharded over the ranks of a data-parallel job: 1-3 over this rank's rows into the
    exchange buffer of the whole set (``_WholeSet``), one sum all-reduce, then 4 over the complete arrays;
  * ``_ChunkedEval``, rows in chunks of at most C: a chunk is a rank in time -- 1-3 per chunk (``_ChunkPart``: one captured
    structure per chunk shape) into the same buffer, then 4.

The group index lists (rows with a second profile / a label) are data of the DATASET, taken once; the arrays themselves --
inputs, labels, regression targets, nuisance classes -- are read by the replays, so a dataset edited in place is evaluated
as edited.  ``use_s``: the plans carry the nuisance classes on the device (``_Plan.carry_nuisance``) and the sequences feed
them from ``ds.s`` (``dv_nuisance_feed``); the MMD penalty's value comes from ``dv_mmd_grouped_fwd`` -- a term with an empty
side counts 0 there, where ``_evaluate``'s host-list plan compares with one random row."""
import contextlib
import gc
import types
import warnings
from collections import OrderedDict

import numpy as np
import torch

from . import engine as E
from . import kernels as K
from . import metrics as MET
from ._lib import GAUSS_SIGMA
from .chain import _Chain, _pad4
from .sparse_rows import CsrRows

_REC = 'RMSE: {:.3f} R2: {:.3f} Pearson: {:.3f}'
_NAN4 = ('rmse', 'r2', 'pearr', 'll')
_N_LOSS = len(E.LOSS_IDX)


# ------------------------------------------------------------------------------------- what every evaluator starts from
def traits(model):
    """what the model's configuration decides for every evaluator: ``cont`` (the regression head), ``use_s``, the decoder
    family ``fam`` and ``rec_kind``, its count kind as ``K.recon_rows`` names it (None: the Gaussian decoder)"""
    kind, fam = model.kind, E.REC_FAMILIES[model.type_rec]
    return types.SimpleNamespace(kind=kind, use_s=bool(getattr(model, 'use_s', False)),
                                 cont=kind != 'pvae' and getattr(model, 'type_y', 'discrete') != 'discrete', fam=fam,
                                 rec_kind=None if fam.recon_kind == E.RECON_KIND[None] else model.type_rec)


def vector_names(kind, cont, has_x2):
    """the names of the float64 result vector: [losses (all seven; ``report`` picks the model's) | y | x1 | x2]"""
    names = ['loss_' + k for k in sorted(E.LOSS_IDX, key=E.LOSS_IDX.get)]
    if kind != 'pvae':
        names += ['y_rmse', 'y_r2', 'y_pearr'] if cont else ['y_auroc', 'y_aupr', 'y_acc']
    return names + ['x1_' + k for k in _NAN4] + (['x2_' + k for k in _NAN4] if has_x2 else [])


def _needed(t):
    return ('x1',) + (('x2', 'has_x2') if t.kind != 'vfae' else ()) + (('y', 'has_y') if t.kind != 'pvae' else ()) + \
        (('s',) if t.use_s else ())


def unreadable(model, ds, sparse_ok):
    """the reason the captured evaluations cannot read the data set ``ds`` in place, or None.  A function of the model's
    configuration and the dataset's tensors alone: every rank of a data-parallel job decides alike.  ``CsrRows`` matrices are
    a reason unless ``sparse_ok`` (the row-chunked evaluation stages them chunk by chunk)"""
    if not sparse_ok and any(isinstance(getattr(ds, k, None), CsrRows) for k in ('x1', 'x2')):
        return 'sparse rows: dense matrices are read in place'
    t, dev = traits(model), next(model.parameters()).device
    for k in _needed(t):      # (a host-resident label / flag array would be a pageable copy under capture)
        v = getattr(ds, k, None)
        if not ((torch.is_tensor(v) or isinstance(v, CsrRows)) and v.is_cuda and v.device == dev):
            return 'reads the data set on the model\'s device (%s): %r is %s' % (
                dev, k, 'missing' if v is None else 'host-resident or on another device')
    if t.cont and not ds.y.is_floating_point():
        return "type_y='cont' reads floating-point targets"
    if t.use_s and (ds.s.is_floating_point() or ds.s.is_complex() or ds.s.dtype == torch.bool):
        return 'the nuisance classes are integers'
    return None


def report_text(kind, cont, perf, has_x2):
    """the ``Y: ... X1: ... X2: ...`` line of an evaluation from its ``perf``; a set without second profiles gets its nan"""
    parts = []
    if kind != 'pvae' and cont:
        parts.append('Y: ' + _REC.format(perf['y_rmse'], perf['y_r2'], perf['y_pearr']))
    elif kind != 'pvae':
        parts.append('Y: Accuracy: {:.3f}% AUROC: {:.3f} AUPR: {:.3f}'.format(perf['y_acc'] * 100., perf['y_auroc'], perf['y_aupr']))
    parts.append('X1: ' + _REC.format(perf['x1_rmse'], perf['x1_r2'], perf['x1_pearr']))
    if kind != 'vfae' and has_x2:
        parts.append('X2: ' + _REC.format(perf['x2_rmse'], perf['x2_r2'], perf['x2_pearr']))
    elif kind != 'vfae':
        for k in _NAN4:
            perf['x2_' + k] = np.nan
        parts.append('X2: no x2 data')
    return '\t '.join(parts)


def report(model, t, names, vec, loss_keys):
    """(perf, text) of ``evaluate_performance_on_dataset`` from the result vector: THE host sync of an evaluation"""
    v = dict(zip(names, vec.cpu().tolist()))
    perf = OrderedDict()
    perf['losses'] = OrderedDict((k, torch.tensor(v['loss_' + k])) for k in loss_keys)
    for k in (() if t.kind == 'pvae' else ('rmse', 'r2', 'pearr') if t.cont else ('acc', 'auroc', 'aupr')):
        perf['y_' + k] = v['y_' + k]
    for tag in ('x1_',) + (('x2_',) if 'x2_rmse' in v else ()):
        for k in _NAN4:
            perf[tag + k] = v[tag + k]
    text = report_text(t.kind, t.cont, perf, 'x2_rmse' in v)
    perf['model_class'] = model.__class__.__name__
    return perf, text


@contextlib.contextmanager
def borrowed(model, use_s, counts=None, row0=0, rng=False):
    """The engine and model state an evaluator's build borrows and gives back -> the engine.  Inside: the model in evaluation
    mode, plans that carry the nuisance classes on the device when ``use_s`` (``_Plan.carry_nuisance``: a plan of its own key,
    the plan a bound ``DeviceBatcher`` replays stays in the cache), and with ``counts`` the loss pass normalised by these
    (N_total, N_pairs, N_labeled) with its Philox draws keyed from row ``row0`` -- a row range of a larger set.  Given back:
    the engine's plan / mode / feed switch / first row, the model's mode and counts, and with ``rng`` the Philox counter and
    the draw drawn ahead (building then leaves the counter where it found it).  No garbage collection in between, as in
    ``FusedStep.capture``: a collected cycle may own the graph of a retired model's evaluation (evaluator <-> model), and
    destroying a graph while a stream is capturing aborts the process."""
    eng = model.engine()
    keep = eng.plan, eng.training, eng.carry_s, eng.row0
    was_training, keep_counts = model.training, model.__dict__.get('_global_counts')
    keep_rng = (eng._rng_pending, eng.rng_ctr.clone()) if rng else None
    gc_was_on = gc.isenabled()
    try:
        gc.collect()
        gc.disable()
        model.eval()
        eng.carry_s = use_s
        if counts is not None:
            model._global_counts, model._row0_override = counts, row0
        yield eng
    finally:
        if gc_was_on:
            gc.enable()
        eng.plan, eng.training, eng.carry_s, eng.row0 = keep
        model.train(was_training)
        model.__dict__.pop('_row0_override', None)
        if keep_counts is None:
            model.__dict__.pop('_global_counts', None)
        else:
            model._global_counts = keep_counts
        if rng:
            eng._rng_pending = keep_rng[0]
            eng.rng_ctr.copy_(keep_rng[1])
            eng._noise_stale = True


def _loss_pass_kw(kind, ds):
    kw = dict(x1=ds.x1, s=getattr(ds, 's', None))
    if kind != 'vfae':
        kw.update(x2=ds.x2, has_x2=ds.has_x2)
    if kind != 'pvae':
        kw.update(y=ds.y, has_y=ds.has_y)
    return kw


def _capture(sequence, eng=None):
    """``sequence`` once eagerly (the warm-up: code objects), then into a graph"""
    sequence()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    if eng is not None:
        eng.join_side()
    with torch.cuda.graph(graph):
        sequence()
    return graph


def _feed_x(p, x1, x2=None, sel=None):
    """the rows (``sel`` of them) of the input matrices into a loss plan's source rows, device to device"""
    pick = lambda a: a.index_select(0, sel) if sel is not None else a
    p.feed_active = False
    p.XSRC[:p.B].copy_(pick(x1.to(torch.float32)))
    if x2 is not None:
        p.XSRC[p.B:].copy_(pick(x2.to(torch.float32)))


def _feed_s(p, s32, L):
    """the nuisance classes of a plan's rows, device to device -- the launch ``_Plan.set_s_device`` makes: one-hot columns of
    the stacked encoder / decoder rows and the class vector the grouped MMD penalty reads"""
    K.nuisance_feed(p.SOHe, p.SOHd, p.s_cls, s32.contiguous(), pair_rows=p.pair_idx if p.Np else None, L=L)


# ------------------------------------------------------------------------------------- these rows, this model
class _Rows:
    """A block of rows of one model: the means-only inference over them and the partials of their reconstructions.  Owns the
    inference chains, the decoder's stacked input [z1; z2], the one-hot operands of a ``use_s`` model, the theta block of a
    gene-wise dispersion and per reconstructed matrix ``tag`` the (row statistics, column-moment blocks, log-likelihood
    rows) -- all allocated here.

    ``ds``: the rows (``x1``, ``x2``, ``s``: tensors of ``n`` rows).  ``encoded``: the loss plan whose pass has just encoded
    exactly these rows in this order, or None -- then the block runs the encoder chain itself.  ``blocks``: tag -> the number
    of column-moment blocks to hold (``zero_parts``: zeroed; a consumer that reads only the blocks a pass wrote needs none)."""

    def __init__(self, model, t, ds, encoded, blocks, zero_parts=True):
        eng = model.engine()
        n, Z, X, S = int(ds.x1.shape[0]), eng.cfg.dim_z1, eng.cfg.dim_x, eng.cfg.dim_s
        dev = ds.x1.device
        reps = 2 if t.kind != 'vfae' else 1
        pad4 = lambda rows, cols: torch.zeros(rows, _pad4(cols), device=dev)[:, :cols]      # rows padded to 16 B
        self.model, self.t, self.ds, self.encoded, self.n = model, t, ds, encoded, n
        self.c_enc = _Chain(eng.L_enc, n, dev) if encoded is None else None
        # (an own encoder pass over rows that are no multiple of 16 B: a padded copy, so that the first layer's product runs on
        # the LDS-DMA kernels -- ``_Chain``)
        self.x1p = pad4(n, X) if encoded is None and X % 4 else None
        self.c_dec = _Chain(eng.L_decx, n * reps, dev)
        self.zd = pad4(n * reps, Z)
        if t.use_s:      # one_hot(s) operands of the encoder / decoder chains (the stacked rows use the same classes twice)
            self.soh_e, self.soh_d = pad4(n, S), pad4(n * reps, S)
            self.s_all = torch.zeros(n, dtype=torch.int32, device=dev)
        self.disp = getattr(model, 'dispersion', 'gene-cell')
        self.gtail = torch.zeros(n * reps, (len(t.fam.heads) - 1) * X, device=dev) if self.disp != 'gene-cell' else None
        new_part = torch.zeros if zero_parts else torch.empty
        self.bufs = {tag: (torch.empty(n, 6, device=dev), new_part(nb, 3, X, dtype=torch.float64, device=dev),
                           torch.empty(n, device=dev)) for tag, nb in blocks.items()}

    def feed_s(self, s32):
        """one_hot(s) of every row for the inference's chains"""
        K.nuisance_feed(self.soh_e, self.soh_d, self.s_all, s32.contiguous(), L=2 if self.t.kind != 'vfae' else 1)

    def infer(self):
        """``forward`` (means-only inference, src/DrVAE.py:253-311) with its two heavy blocks on the fused step's layer
        chains: the encoder's heads as ONE (mu | logvar) product, and the decoder ONCE over the stacked rows [z1; z2]
        with its (mu | std) heads as one product -- 3 launches of 2n rows instead of 6 of n (the block modules compute
        every head with a launch of its own).  The small blocks in between are the model's own modules."""
        m, ds, t, kind = self.model, self.ds, self.t, self.t.kind
        eng = m.engine()
        n, Z, X = self.n, eng.cfg.dim_z1, eng.cfg.dim_x
        if self.encoded is not None:
            # q(z1|x1) of every row has just been computed by the loss pass (the sequences run it first): evaluation mode adds
            # no input noise, its encoder input rows [0, n) ARE x1 in dataset order, same layer chain, same kernels -- the
            # first n rows of its heads' buffer are this product (8192 rows: 15 GFLOP not computed twice).  The raw-count
            # switches change nothing here: the sequences clear ``eng.training`` before the pass, so ``_encoder_forward``
            # takes sigma = 0 and hands the split feed ``noise=None`` -- its encoder rows are T(x1) exactly (log1p(x1) with
            # ``x_transform='log1p'``), what ``forward`` feeds the encoder
            Q = self.encoded.c_enc.out[-1][:n]
        else:
            x1 = m._enc_x(ds.x1.to(torch.float32))      # (``x_transform='log1p'``: the encoder reads log1p(x1))
            if self.x1p is not None:
                self.x1p.copy_(x1)
                x1 = self.x1p
            Q = self.c_enc.forward([x1] + ([self.soh_e] if t.use_s else []))
        z1 = Q[:, :Z]
        res = OrderedDict(z1=z1, qz1=(z1, Q[:, Z:2 * Z]))
        if kind != 'vfae':
            # the perturbation function's MEAN only (its log-variance feeds no metric): z2 = z1 + z1 W_mu^T + b
            # (src/blocks.py:357), one launch, straight into the second half of the decoder's stacked input
            lz = eng.L_z2F[0]
            z2 = self.zd[n:]
            K.linear_fwd(z2, z1, lz.W[:Z], lz.b[:Z], resid=z1, resid_cols=Z, overread=True)
            res.update(z2=z2)
        if kind != 'pvae':
            if kind == 'drvae':
                clf_in = [z1, z2 - z1] if m.clf_z1z2 else [z2]
            else:
                clf_in = [z1]
            res.update(**m._pred_proba(m.encoder_y(clf_in)))
        self.zd[:n].copy_(z1)
        # the decoder's heads as a PLAIN product where the one-pass reconstruction statistics finish them on their way
        # (bias, softplus + shift: ``dv_recon_rows`` / ``dv_col_moments``): 16384 x 1956 x 600 at the raw product's 126 instead of 104 TF/s
        # The count decoders' heads leave their launch FINISHED (probability / rate / [mean | theta]: ``raw_last_ok`` is false
        # for them); ``px1`` / ``px2`` are 1-tuples for 'binary' / 'poisson', (mu, theta) for 'nb' and (mu, theta, logit) for 'zinb' -- UNSCALED: the size
        # factor of a ``library_size`` model is applied by the row pass (``_rows_pass``)
        lh = eng.L_decx[-1]
        raw = bool(t.rec_kind is None and X <= K.RECON_ROWS_MAX_X and self.c_dec.raw_softplus_ok())
        PX = self.c_dec.forward([self.zd] + ([self.soh_d] if t.use_s else []), raw_last=raw)
        res['px_bias'] = (lh.b[:X], lh.b[X:2 * X], lh.shift1) if raw else None
        # (three heads, 'zinb': (mu, theta, logit) as ``forward`` returns it -- columns of the ONE buffer, so [theta | logit] is
        # the contiguous view from column X on that ``_rows_pass`` hands the row pass)
        nh = len(t.fam.heads)
        if self.gtail is not None:
            # a gene-wise theta: ``dv_recon_rows`` has no broadcast operand, so the finished theta row is written into a theta
            # block once per replay, as one row repeated (M x X words written and read), with the decoder's logit columns copied
            # behind it for 'zinb' -- then the recon kinds run as they are, and the numbers are ``_evaluate``'s key by key
            # (``fam`` is the family of ``type_rec`` as the recon kinds know it -- mean, theta[, logit]; the decoder's own heads
            # buffer is [mean] or [mean | logit])
            rows_all, nt, T_ = PX.shape[0], nh - 1, self.gtail
            if self.disp == 'gene-batch':
                # a theta per (class, gene): every evaluation row its own class's row of the finished table -- a gather by the
                # set's class vector (``s_all``: the decoder's stacked rows [z1; z2] use the same classes twice), on the device
                T_[:, :X].copy_(m.decoder_x.decoder_t(self.s_all.long().repeat(rows_all // n)))
            else:
                T_[:, :X].copy_(m.decoder_x.decoder_t(rows_all))
            if nt > 1:
                T_[:, X:].copy_(PX[:, X:2 * X])
            heads = lambda lo, hi: (PX[lo:hi, :X],) + tuple(T_[lo:hi, k * X:(k + 1) * X] for k in range(nt))
            res['px1'], res['tail1'] = heads(0, n), T_[:n]
            if kind != 'vfae':
                res['px2'], res['tail2'] = heads(n, rows_all), T_[n:]
            return res
        heads = lambda P: tuple(P[:, k * X:(k + 1) * X] for k in range(nh))
        tail = lambda P: P[:, X:nh * X] if nh > 1 else None      # (the heads behind the mean, back to back: ``dv_recon_rows``' sd)
        res['px1'], res['tail1'] = heads(PX[:n]), tail(PX[:n])
        if kind != 'vfae':
            res['px2'], res['tail2'] = heads(PX[n:]), tail(PX[n:])
        return res

    def _rows_pass(self, rows, ll, x, px, bias, tail=None):
        """row statistics (+ log-likelihood rows) of the target rows ``x`` against the heads ``px`` -> (the reconstruction
        ``dv_col_moments`` reads, the log-likelihood rows ``dv_recon_finalize`` reads or None).  Gaussian decoder: one pass up
        to 1024 genes, else the two separate ones.  Count decoders: ``dv_recon_rows``' count kinds at any width; with
        ``library_size`` the mean is scaled by the size factor of the SAME rows of ``x1`` -- for the x2 targets too,
        as ``forward`` does it -- and stored in place of the mean head, where ``dv_col_moments`` finds it.  ``tail``: the
        heads behind the mean as ONE view of the heads buffer (``infer``): theta for 'nb', [theta | logit] for 'zinb', None
        for one head.  'binary' / 'poisson' report no log-likelihood (``_evaluate`` passes no second head: nan), 'nb' the
        negative binomial's, 'zinb' the zero-inflated one (its statistics are taken at the negative-binomial mean)."""
        t = self.t
        if t.rec_kind is not None:
            ll = ll if t.fam.eval_ll else None
            size = self.ds.x1.to(torch.float32) if getattr(self.model, 'library_size', False) else None
            K.recon_rows(rows, ll, x, px[0], tail, kind=t.rec_kind, size_from=size,
                         rec_out=px[0] if size is not None else None)
            return px[0], ll
        if x.shape[1] <= K.RECON_ROWS_MAX_X:
            K.recon_rows(rows, ll, x, px[0], px[1], bias=bias[:2] if bias is not None else None,
                         sd_shift=bias[2] if bias is not None else 0.0)
        else:
            K.recon_row_stats(rows, x, px[0])
            K.nll_rows_fwd(ll, x, px[0], px[1], mode=GAUSS_SIGMA)
        return px[0], ll

    def partials(self, tag, x, px, bias, tail, sel=None, deliver=None):
        """The partials of ``eval_x_reconstruction`` (src/DGMMixin.py:128-156) of the target rows ``x`` against the heads
        ``px`` / ``tail`` of these rows -> (rows, part, ll, x_rec): six statistics and the log-likelihood (None: none is
        reported) per row -- taken over ALL rows, whoever finalises selects (no gathered copies of the x2 rows) -- and the
        column-moment blocks of the rows ``sel`` (all when None; none selected: no launch, no block).  Rows of up to 1024
        genes: statistics and log-likelihood rows in ONE pass (``dv_recon_rows``); ``bias`` = (bias_mu, bias_sd, shift): the
        heads are raw products, finished by the passes.  ``deliver(rows, ll)`` runs between the row pass and the column
        pass: a consumer that sends the per-row results elsewhere issues its copies there."""
        x = x.to(torch.float32)
        assert bias is None or x.shape[1] <= K.RECON_ROWS_MAX_X
        rows, part, ll = self.bufs[tag]
        x_rec, ll = self._rows_pass(rows, ll, x, px, bias, tail)
        if deliver is not None:
            deliver(rows, ll)
        n_sel = int(sel.numel()) if sel is not None else int(x.shape[0])
        part = part[:K.col_moment_blocks(n_sel) if n_sel else 0]
        if n_sel:
            K.col_moments(None, x, x_rec, sel=sel, part=part, r_bias=bias[0] if bias is not None else None)
        return rows, part, ll, x_rec


# ------------------------------------------------------------------------------------- classification metrics
def rank_scratch(Y, n_lab, dev):
    """the pair counts and the per-class results of ``class_metrics`` for ``n_lab`` labeled rows (None: sort + scan)"""
    if n_lab > K.RANK_MAX_ROWS or n_lab == 0:
        return None
    n_cls = 1 if Y == 2 else Y
    return (torch.zeros(n_cls, n_lab, 4, dtype=torch.int32, device=dev), torch.zeros(2 * n_cls + 1, dtype=torch.float64, device=dev))


def class_metrics(out3, Y, sel32, scratch, operands, gathered):
    """accuracy / ROC-AUC / average precision of the labeled rows ``sel32`` (src/DGMMixin.py:158-190) -> out3 = [auroc, aupr,
    acc].  ``operands()`` -> (proba, y32, pred32) over all rows for the pair-counting kernel; beyond its range (``scratch``
    is None) the sort + scan formulation on ``gathered()`` -> (pred, proba, labels) of the labeled rows.  Both are the
    caller's: they issue its conversions and gathers, and only the route taken issues any."""
    if scratch is None:
        v = MET.eval_y_prediction_dev(*gathered(), Y)
        out3.copy_(torch.stack([v['auroc'].reshape(()), v['aupr'].reshape(()), v['acc'].reshape(())]))
        return
    counts, out = scratch
    proba, y32, pred32 = operands()
    if Y == 2:
        K.rank_metrics(out3, counts, proba, y32, pred32=pred32, sel=sel32, c0=1, n_cls=1, binary=True)
    else:       # macro average over the one-vs-rest problems (nan as soon as one class's value is: the mean propagates it)
        K.rank_metrics(out, counts, proba, y32, pred32=pred32, sel=sel32, c0=0, n_cls=Y, binary=False)
        out3[0:1].copy_(out[0:2 * Y:2].mean().reshape(1))
        out3[1:2].copy_(out[1:2 * Y:2].mean().reshape(1))
        out3[2:3].copy_(out[2 * Y:2 * Y + 1])


# ------------------------------------------------------------------------------------- the whole set, out of row blocks
class _WholeSet:
    """The whole set's side of an evaluation whose heavy passes run on row blocks (the ranks' shards, the chunks): ONE flat
    float64 exchange buffer ``pack`` laid out for the WHOLE set -- [loss scalars | proba | pred | x1: row statistics,
    log-likelihood rows, column-moment blocks | x2: the same] --, the whole set's index lists, the complete per-row arrays
    and the finalising launches over them (``finalize``: the same kernels as the one-replay evaluation) into ``vec``.

    ``bounds``: the row ranges that write column-moment blocks of their own (the ranks' shards: every rank writes its rows'
    slots, zeros elsewhere, one sum all-reduce leaves the complete arrays on every rank -- float32 / int32 values are exact
    in float64, and x + 0 = x).  None: one block per matrix that the blocks' moments are folded into (``fold_col_blocks``).
    ``flags``: (has_x2, has_y) as host bool arrays (None for a flag the model does not read), when the caller has fetched
    them anyway; else the index lists are taken on the device (a host sync per flag array)."""

    def __init__(self, model, t, ds, bounds=None, flags=None):
        kind, dev = t.kind, ds.x1.device
        n, X, Y = int(ds.x1.shape[0]), int(ds.x1.shape[1]), (model.dim_y if kind != 'pvae' else 0)
        self.t, self.ds, self.n, self.X, self.Y = t, ds, n, X, Y
        self.x2idx32 = self.yidx32 = None
        self.n_x2 = 0
        # the rows a flag array marks, int32 on the device: from the caller's host copy of the flags when it holds one
        rows_of = lambda f: (torch.nonzero(f).reshape(-1).to(torch.int32) if torch.is_tensor(f) else
                             torch.as_tensor(np.nonzero(f)[0], dtype=torch.int32).to(dev))
        # column-moment blocks per range and matrix: what the range with the most rows (second profiles) needs
        blocks = lambda count: max(K.col_moment_blocks(max(count(a, b), 1)) for a, b in bounds) if bounds else 1
        self.blk = {'x1': blocks(lambda a, b: b - a)}
        if kind != 'vfae':
            hx = ds.has_x2.reshape(-1).to(dev) != 0 if flags is None else flags[0]
            self.x2idx32 = rows_of(hx)
            self.n_x2 = int(self.x2idx32.numel())
            blk2 = blocks(lambda a, b: int(hx[a:b].sum()))
            if self.n_x2:
                self.blk['x2'] = blk2
        if kind != 'pvae':
            self.yidx32 = rows_of(ds.has_y.reshape(-1).to(dev) if flags is None else flags[1])
        ranges = len(bounds) if bounds else 1
        o, self.off = 0, {}
        # (regression head: the ``pred`` slot carries the n x Y float means; no class probabilities, no int32 buffers)
        for name, size in (('loss', 8), ('proba', 0 if t.cont else n * Y), ('pred', n * Y if t.cont else (n if Y else 0)),
                           ('rows1', n * 6), ('ll1', n), ('part1', ranges * self.blk['x1'] * 3 * X),
                           ('rows2', n * 6 if self.n_x2 else 0), ('ll2', n if self.n_x2 else 0),
                           ('part2', ranges * self.blk['x2'] * 3 * X if self.n_x2 else 0)):
            self.off[name] = (o, size)
            o += size
        self.pack = torch.zeros(o, dtype=torch.float64, device=dev)
        f32 = lambda *shape: torch.zeros(*shape, device=dev)
        self.g_rows = {'x1': f32(n, 6), 'x2': f32(n, 6)}
        self.g_ll = {'x1': f32(n), 'x2': f32(n)}
        if Y and t.cont:
            self.g_pred = f32(n, Y)
        elif Y:
            self.g_proba, self.g_pred32 = f32(n, Y), torch.zeros(n, dtype=torch.int32, device=dev)
            self.g_y32 = torch.zeros(n, dtype=torch.int32, device=dev)
            self.rank = rank_scratch(Y, int(self.yidx32.numel()), dev)
        self.names = vector_names(kind, t.cont, self.n_x2 > 0)
        self.vec = torch.zeros(len(self.names), dtype=torch.float64, device=dev)

    def slot(self, name, *shape):
        o, size = self.off[name]
        return self.pack[o:o + size].view(*shape) if shape else self.pack[o:o + size]

    def mats(self, x1, x2=None, sel2=None):
        """(tag, slot suffix, target rows, selection) of the matrices a row block reconstructs: ``x1``, and ``x2`` (its rows
        ``sel2``) when the block has it and the set has second profiles at all"""
        return (('x1', '1', x1, None),) + ((('x2', '2', x2, sel2),) if x2 is not None and self.n_x2 else ())

    def collect(self, blk, res, where, mats, put_part):
        """A row block's share into the exchange buffer: the inference's per-row results and, per matrix of ``mats``, the row
        statistics and log-likelihood rows to ``where`` -- a (lo, hi) range of rows, or the rows' positions (an int64 device
        vector: the values go through float64 copies) -- and the column-moment blocks to ``put_part(tag, suffix, part)``."""
        n, Y = self.n, self.Y

        def put(name, src, *width):
            dst = self.slot(name, n, *width) if width else self.slot(name)
            if isinstance(where, tuple):
                dst[where[0]:where[1]].copy_(src)
            else:
                dst.index_copy_(0, where, src.to(torch.float64))
        if Y and self.t.cont:
            put('pred', res['pred'], Y)
        elif Y:
            put('proba', res['proba'], Y)
            put('pred', res['pred'].reshape(-1))
        bias = res['px_bias']
        for tag, s, x, sel in mats:
            def deliver(rows, ll):
                put('rows' + s, rows, 6)
                if ll is not None:      # ('binary' / 'poisson': no reported log-likelihood, the slot stays zero and is not read)
                    put('ll' + s, ll)
            part = blk.partials(tag, x, res['px' + s], bias, res['tail' + s], sel, deliver)[1]
            if part.shape[0]:
                put_part(tag, s, part)

    def finalize(self):
        """behind the last block (the all-reduce): the complete arrays out of the exchange buffer, then the SAME finalising
        launches as the one-replay evaluation (``dv_rank_metrics``, ``dv_recon_finalize``) over the whole set -> ``vec``"""
        ds, vec, n, X, Y = self.ds, self.vec, self.n, self.X, self.Y
        vec[:_N_LOSS].copy_(self.slot('loss')[:_N_LOSS])
        o = _N_LOSS
        if Y and self.t.cont:
            # (the targets are read by the replay: a dataset edited in place is evaluated as edited)
            self.g_pred.copy_(self.slot('pred', n, Y))
            K.reg_metrics(vec[o:o + 3], self.g_pred, ds.y.reshape(n, -1).to(torch.float32), sel=self.yidx32)
            o += 3
        elif Y:
            self.g_proba.copy_(self.slot('proba', n, Y))
            self.g_pred32.copy_(self.slot('pred'))
            self.g_y32.copy_(ds.y.reshape(-1))        # (read by the replay, as the targets above)

            def gathered():
                idx = self.yidx32.long()
                return self.g_pred32.index_select(0, idx), self.g_proba.index_select(0, idx), self.g_y32.index_select(0, idx).long()
            class_metrics(vec[o:o + 3], Y, self.yidx32, self.rank, lambda: (self.g_proba, self.g_y32, self.g_pred32), gathered)
            o += 3
        for tag, s, sel in (('x1', '1', None),) + ((('x2', '2', self.x2idx32),) if self.n_x2 else ()):
            self.g_rows[tag].copy_(self.slot('rows' + s, n, 6))
            self.g_ll[tag].copy_(self.slot('ll' + s))
            K.recon_finalize(vec[o:o + 4], self.g_rows[tag], self.slot('part' + s, -1, 3, X), X, sel=sel,
                             n=int(sel.numel()) if sel is not None else n, ll=self.g_ll[tag] if self.t.fam.eval_ll else None)
            o += 4


# ------------------------------------------------------------------------------------- one replay; rows sharded over ranks
class _EvalGraph:
    """The whole-set evaluation of one dataset as a captured launch sequence: one replay, ONE copy to the host.
    ``run()`` = set the annealing coefficient, replay, copy.

    ``dp`` = (rank, world), data parallelism: the ROWS of the evaluation are sharded over the ranks (every rank holds the
    dataset; its heavy passes run on rows [n r / W, n (r + 1) / W) only, as VIEWS of the dataset's tensors; the normalisers
    of the loss pass are the whole set's counts, the Philox draws are keyed by the row's position in the whole set --
    ``row0`` --, so the shards' terms add up to the one-rank evaluation's), the partials meet in ONE all-reduce and a
    second graph finalises them (``_WholeSet``)."""

    CACHE_KEYS = ('_eval_graphs', '_eval_graphs_own_kind')

    @staticmethod
    def cache(model):
        """the model's captured evaluations, by ``id(dataset)``.  ``model._eval_graphs`` for the decoders whose kind of
        ``dv_recon_rows`` is in the table ``RECON_KIND``; a kind with a name of its own beside that table ('zinb':
        ``RECON_ZINB``) keeps its graphs under a key of its own -- ``tests/test_gpu_zinb.py`` holds ``_eval_graphs`` of a
        'zinb' model empty after ``fit``, from when that evaluation was declined, and existing test files stay as they are.
        Whoever drops the cache drops every key of ``CACHE_KEYS`` (``DGMMixin``)"""
        in_table = E.REC_FAMILIES[model.type_rec].recon_kind in E.RECON_KIND.values()
        return model.__dict__.setdefault(_EvalGraph.CACHE_KEYS[0 if in_table else 1], {})

    @staticmethod
    def get(model, ds):
        """the captured evaluation of (model, dataset), built at the first call; None: the step-by-step path answers"""
        if unreadable(model, ds, sparse_ok=False) is not None:
            return None
        use_s = bool(getattr(model, 'use_s', False))
        if use_s and getattr(model, 'use_MMD', False) and not (
                getattr(model, 'kernel_MMD', 'rbf_fourier') in K.MMD_GROUPED_KIND and 2 <= int(model.dim_s) <= K.MMD_MAX_CLASSES):
            return None          # (the penalty's grouped launches cover these; the rest keeps the host-list path)
        x1 = ds.x1
        cache = _EvalGraph.cache(model)
        # the captured launches point into the engine's arena, plan and layer chains: ``.cpu().cuda()`` / ``.to()`` retire
        # the engine (DGMMixin._apply) and a graph of the old one would read freed parameters -- the engine's identity is
        # part of the signature (and ``_apply`` drops the cache)
        eng = model.engine()
        dp = model._dp if (getattr(model, '_dp', None) is not None and getattr(model, 'shard_evaluation', True)
                           and int(x1.shape[0]) >= 2 * model._dp[1]) else None
        sig = tuple(int(t.data_ptr()) if torch.is_tensor(t) else 0
                    for t in (getattr(ds, k, None) for k in ('x1', 'x2', 'y', 'has_x2', 'has_y') + (('s',) if use_s else ()))) + \
            (int(x1.shape[0]), id(eng), int(eng.arena.param.data_ptr()), dp)
        ev = cache.get(id(ds))
        if ev is None or ev.sig != sig:
            if len(cache) > 8:
                cache.clear()
            try:
                ev = cache[id(ds)] = _EvalGraph(model, ds, sig, dp=dp)
            except Exception as e:      # the reference evaluates on regardless of a failing loss pass (src/DrVAE.py:647-654):
                # so does the step-by-step path, which this dataset now takes
                warnings.warn('drvae_amd: the captured whole-set evaluation could not be built (%s: %s); evaluating step '
                              'by step' % (type(e).__name__, e))
                ev = cache[id(ds)] = _EvalGraph.__new__(_EvalGraph)
                ev.sig, ev.graph = sig, None
        return ev if ev.graph is not None else None

    def __init__(self, model, ds, sig, dp=None):
        from . import dist as D
        self.model, self.sig, self.graph, self.dp, self.whole = model, sig, None, dp, None
        t = self.t = traits(model)
        self.fam, self.rec_kind = t.fam, t.rec_kind
        kind, dev, n_all = t.kind, ds.x1.device, int(ds.x1.shape[0])
        full, counts, bounds = ds, None, None
        self.lo, self.hi = 0, n_all
        if dp is not None:
            rank, world = dp
            bounds = [(n_all * r // world, n_all * (r + 1) // world) for r in range(world)]
            self.lo, self.hi = bounds[rank]
            flags = lambda k, skip: getattr(full, k).cpu().numpy() if kind != skip else np.zeros(n_all, np.int64)
            cfg = model.engine().cfg
            counts = D.global_counts(flags('has_x2', 'vfae'), flags('has_y', 'pvae'), cfg.kind, cfg.semi_supervised, local=True)
            ds = types.SimpleNamespace(**{k: (getattr(full, k)[self.lo:self.hi] if torch.is_tensor(getattr(full, k, None)) else None)
                                          for k in ('x1', 'x2', 's', 'y', 'has_x2', 'has_y')})
        self.ds = ds
        n = int(ds.x1.shape[0])
        # rows of the groups (once per dataset: a host sync each)
        self.x2idx = torch.nonzero(ds.has_x2.reshape(-1).to(dev)).reshape(-1) if kind != 'vfae' else None
        self.yidx = torch.nonzero(ds.has_y.reshape(-1).to(dev)).reshape(-1) if kind != 'pvae' else None
        self.x2idx32 = self.x2idx.to(torch.int32) if self.x2idx is not None else None
        self.yidx32 = self.yidx.to(torch.int32) if self.yidx is not None else None
        with borrowed(model, t.use_s, counts, self.lo) as eng:
            # the loss plan of these rows: built by the ordinary path (host index lists), then reused
            model.run_on_batch(train_mode=False, **_loss_pass_kw(kind, ds))      # (also the warm-up of every kernel of the pass)
            self.plan = eng.plan
            rows = np.asarray(self.plan.rows)
            self.sel = None if (len(rows) == n and (rows == np.arange(n)).all()) else torch.as_tensor(rows, device=dev)
            self.loss_keys = list(model._loss_tensors(eng))
            if dp is not None:
                self.whole = _WholeSet(model, t, full, bounds)
                self.pack, self.names, self.vec, blocks = self.whole.pack, self.whole.names, self.whole.vec, self.whole.blk
            else:
                self.has_x2 = kind != 'vfae' and len(self.x2idx) > 0
                self.names = vector_names(kind, t.cont, self.has_x2)
                self.vec = torch.zeros(len(self.names), dtype=torch.float64, device=dev)
                blocks = {'x1': K.col_moment_blocks(n)}
                if self.has_x2:
                    blocks['x2'] = K.col_moment_blocks(len(self.x2idx))
                if kind != 'pvae' and not t.cont:
                    self.rank = rank_scratch(model.dim_y, int(self.yidx.numel()), dev)
                    if self.rank is not None:      # (the pair-counting kernel's int32 operands; sort + scan reads none)
                        self.y32 = torch.zeros(n, dtype=torch.int32, device=dev)
                        self.pred32 = torch.zeros_like(self.y32)
            self.blk = _Rows(model, t, ds, self.plan if self.sel is None else None, blocks, zero_parts=dp is not None)
            self.graph = _capture(self._sequence, eng)
            if dp is not None:
                self.graph_final = _capture(self.whole.finalize)

    def _sequence(self):
        """the launch sequence (eager for the warm-up, then under capture)"""
        m, ds, t, kind, blk, vec = self.model, self.ds, self.t, self.t.kind, self.blk, self.vec
        eng, p, sel = m.engine(), self.plan, self.sel
        eng.plan = p
        n = int(ds.x1.shape[0])
        # --- evaluation-mode losses on these rows: the fused forward on their plan, inputs from the dataset
        _feed_x(p, ds.x1, ds.x2 if eng.cfg.has_pert else None, sel)
        if t.cont:      # the regression targets of the plan's rows (read by the replay: targets edited in place count)
            y2 = ds.y.reshape(n, -1).to(torch.float32)
            p.ylab.copy_(y2.index_select(0, sel) if sel is not None else y2)
        if t.use_s:     # the nuisance classes: the loss pass's, then one_hot(s) of every row for the inference below
            s32 = ds.s.reshape(-1).to(torch.int32)
            _feed_s(p, s32.index_select(0, sel) if sel is not None else s32, eng.cfg.L)
            blk.feed_s(s32)
        eng.training = False
        eng.draw_noise()
        eng.forward()
        vec[:_N_LOSS].copy_(eng.arena.loss[:_N_LOSS])
        # --- means-only inference + metrics (the tail: dv_rank_metrics / dv_recon_finalize, no sort, no host decisions)
        res = blk.infer()
        whole = self.whole
        if whole is not None:       # this rank's share of the partials into the exchange buffer; no finalising launch
            rank, world = self.dp
            whole.pack.zero_()
            whole.slot('loss')[:_N_LOSS].copy_(vec[:_N_LOSS])

            def put_part(tag, s, part):      # (this rank's blocks of the slot's (world, blocks, 3, X))
                whole.slot('part' + s, world, whole.blk[tag], 3, whole.X)[rank, :part.shape[0]].copy_(part)
            whole.collect(blk, res, (self.lo, self.hi), whole.mats(ds.x1, getattr(ds, 'x2', None), self.x2idx32), put_part)
            return
        o = _N_LOSS
        if kind != 'pvae':
            self._y_metrics(res, vec[o:o + 3])
            o += 3
        for tag, s, x, sel2 in (('x1', '1', ds.x1, None),) + ((('x2', '2', ds.x2, self.x2idx32),) if self.has_x2 else ()):
            rows, part, ll, _ = blk.partials(tag, x, res['px' + s], res['px_bias'], res['tail' + s], sel2)
            K.recon_finalize(vec[o:o + 4], rows, part, int(x.shape[1]), sel=sel2, n=int(sel2.numel()) if sel2 is not None else n, ll=ll)
            o += 4

    def _y_metrics(self, res, out3):
        """the prediction metrics of the labeled rows from the inference's results: [rmse, r2, pearr] of the regression head's
        means (src/DGMMixin.py:181-188, one launch) or ``class_metrics``"""
        m, ds = self.model, self.ds
        if self.t.cont:
            K.reg_metrics(out3, res['pred'], ds.y.reshape(int(ds.x1.shape[0]), -1).to(torch.float32), sel=self.yidx32)
            return

        def operands():
            self.y32.copy_(ds.y.reshape(-1))
            self.pred32.copy_(res['pred'].reshape(-1))
            return res['proba'], self.y32, self.pred32

        def gathered():
            ylab = ds.y.to(ds.x1.device).reshape(-1).index_select(0, self.yidx)
            return res['pred'].index_select(0, self.yidx), res['proba'].index_select(0, self.yidx), ylab
        class_metrics(out3, m.dim_y, self.yidx32, self.rank, operands, gathered)

    def run(self):
        m = self.model
        eng = m.engine()
        eng.join_side()
        eng.iters = m.finished_training_iters
        self.plan.set_beta(*eng.betas())                 # (the annealing coefficient is data of the plan, not of the graph)
        self.graph.replay()
        eng._noise_stale = True      # (the replay drew from the Philox counter: a train step drawn ahead re-draws, as after any eager draw)
        if self.dp is not None:      # rows sharded over the ranks: ONE sum all-reduce of the partials, then the finalising launches
            from . import dist as D
            D.allreduce_sum(self.pack)
            self.graph_final.replay()
        return report(m, self.t, self.names, self.vec, self.loss_keys)


# ------------------------------------------------------------------------------------- whole-set evaluation in row chunks
_CHUNK_GROUPS = ((True, True), (True, False), (False, True), (False, False))      # (has_x2, has_y): the stable order of the groups


def chunk_partition(has_x2, has_y, C, kind):
    """the rows of a data set as chunks of at most ``C`` rows that are homogeneous in (has_x2, has_y): a list of
    ((has_x2, has_y), row positions) -- the groups in the order of ``_CHUNK_GROUPS``, the rows of a group in data-set order, cut
    every ``C`` rows.  Every row is in exactly one chunk.  A flag the model ``kind`` does not read counts as False ('vfae': no
    second profiles, ``has_x2`` may be None; 'pvae': no labels, ``has_y`` may be None).  A pure function of host arrays."""
    C = _ChunkedEval.check_chunk_rows(C)
    flat = lambda a: None if a is None else (np.asarray(a).reshape(-1) != 0)
    hx, hy = flat(has_x2), flat(has_y)
    if kind == 'vfae' or hx is None:
        hx = np.zeros(len(hy), bool)
    if kind == 'pvae' or hy is None:
        hy = np.zeros(len(hx), bool)
    if len(hx) != len(hy):
        raise ValueError('chunk_partition: has_x2 and has_y flag the same rows (got %d and %d)' % (len(hx), len(hy)))
    out = []
    for gx, gy in _CHUNK_GROUPS:
        rows = np.nonzero((hx == gx) & (hy == gy))[0]
        out += [((gx, gy), rows[a:a + C]) for a in range(0, len(rows), C)]
    return out


def fold_col_blocks(acc, part):
    """add a chunk's column-moment blocks ``part`` (blocks, 3, X: raw float64 sums of ``dv_col_moments``) to the (1, 3, X)
    accumulator ``acc``: the blocks are summed in block order, the chunks arrive in chunk order -- one fixed order"""
    assert acc.dtype == part.dtype == torch.float64 and acc.shape[0] == 1 and acc.shape[1:] == part.shape[1:]
    return acc.add_(part.sum(0, keepdim=True))


class _ChunkedEval:
    """``_EvalGraph``'s numbers for a data set evaluated ``C`` rows at a time (``evaluate_performance_on_dataset(chunk_rows=C)``,
    ``model.eval_chunk_rows``): a chunk is a rank in time.  The row-sharded evaluation of data parallelism already evaluates a
    row range with the whole set's normalisers and Philox keys and leaves partials that the unsharded finalising launches
    finish (``_WholeSet``); here the partials of every chunk land in ONE buffer of the whole set, one after the other.

      * The rows are grouped by (has_x2, has_y) -- at most four groups, ``chunk_partition`` -- and chunks are cut inside groups:
        a chunk is homogeneous, so the loss plan of a (group, rows) shape serves every chunk of that shape.  At most one
        full-size and one tail structure per group (``_ChunkPart``), each captured once per (model, data set, C).
      * A replay of a structure reads the data-set positions of its rows from a small device buffer the host refills
        between replays, gathers them into ``C`` x dim_x staging rows (a ``CsrRows`` matrix through the feed launch: never
        densified beyond the chunk), re-targets the GLOBAL row column of the plan's draw descriptors to those positions
        (``_Plan.retarget_rows``), draws WITHOUT advancing the Philox counter, runs the loss pass with the whole set's
        (N_total, N_pairs, N_labeled) and adds its scalars to the float64 sums, runs the means-only inference, and scatters
        the per-row results -- six row statistics, log-likelihood rows, class probabilities / predictions -- to their
        data-set positions; the chunk's column-moment blocks are folded into one (1, 3, X) accumulator (``fold_col_blocks``).
      * Behind the last chunk the counter advances once -- where a one-replay evaluation leaves it -- and ``_WholeSet.finalize``
        runs the same finalising launches over the complete per-row arrays.  No host synchronisation before the ONE copy.

    Device memory that grows with N: the per-row arrays and index lists.  Everything of rows x genes size holds at most ``C``
    rows, times the (bounded) number of structures.  Building leaves the Philox counter where it found it, so an evaluation
    advances it by exactly one whatever the number of chunks, and training does not depend on C."""

    CACHE_KEY = '_eval_chunked'

    @staticmethod
    def check_chunk_rows(c):
        if isinstance(c, (bool, np.bool_)) or not isinstance(c, (int, np.integer)) or int(c) < 1:
            raise ValueError('the evaluation chunk size (eval_chunk_rows / chunk_rows) is None or an integer >= 1, not %r' % (c,))
        return int(c)

    @staticmethod
    def check_model(model):
        """what the model's configuration alone decides (every rank of a data-parallel job decides alike)"""
        if getattr(model, 'use_s', False) and getattr(model, 'use_MMD', False):
            raise NotImplementedError('use_MMD: the MMD penalty compares every row of a nuisance class with every other row of '
                                      'the set -- a cross-row term, it cannot be evaluated in row chunks (eval_chunk_rows)')
        if getattr(model, '_dp', None) is not None:
            raise NotImplementedError('row-chunked evaluation (eval_chunk_rows) under data parallelism is not built: the '
                                      'whole-set evaluation is sharded by rows over the ranks there')

    @staticmethod
    def get(model, ds, C):
        C = _ChunkedEval.check_chunk_rows(C)
        _ChunkedEval.check_model(model)
        why = unreadable(model, ds, sparse_ok=True)
        if why is not None:      # (raised, never answered by another path)
            raise ValueError('row-chunked evaluation' + (' (eval_chunk_rows) ' if why.startswith('reads the data set') else ': ') + why)
        ptrs = lambda t: (int(t.ptr.data_ptr()), int(t.idx.data_ptr()), int(t.val.data_ptr())) if isinstance(t, CsrRows) \
            else (int(t.data_ptr()),)
        eng = model.engine()
        sig = tuple(p for k in _needed(traits(model)) for p in ptrs(getattr(ds, k))) + \
            (int(ds.x1.shape[0]), C, id(eng), int(eng.arena.param.data_ptr()))
        cache = model.__dict__.setdefault(_ChunkedEval.CACHE_KEY, {})
        ev = cache.get((id(ds), C))
        if ev is None or ev.sig != sig:
            cache.pop((id(ds), C), None)
            if len(cache) > 8:
                cache.clear()
            ev = cache[(id(ds), C)] = _ChunkedEval(model, ds, C, sig)      # (a failure raises: no other path answers)
        return ev

    def __init__(self, model, ds, C, sig):
        from . import dist as D
        self.model, self.sig, self.C, self.ds = model, sig, C, ds
        t = self.t = traits(model)
        self.fam, self.rec_kind, self.dp = t.fam, t.rec_kind, None
        kind, eng, dev = t.kind, model.engine(), ds.x1.device
        n, X = int(ds.x1.shape[0]), int(ds.x1.shape[1])
        if n < 1:
            raise ValueError('row-chunked evaluation: the data set has no rows')
        # the grouping is data of the DATASET, taken once (a host sync per flag array), like ``x2idx`` / ``yidx`` of ``_EvalGraph``
        flags = lambda k, skip: (getattr(ds, k).reshape(-1).cpu().numpy() != 0) if kind != skip else None
        hx, hy = flags('has_x2', 'vfae'), flags('has_y', 'pvae')
        chunks = chunk_partition(hx, hy, C, kind)
        zer = np.zeros(n, bool)
        self.counts = D.global_counts(hx if hx is not None else zer, hy if hy is not None else zer, eng.cfg.kind,
                                      eng.cfg.semi_supervised, local=True)
        self.gcounts = torch.tensor([self.counts[1], self.counts[2]], dtype=torch.int32).to(dev)
        self.all_idx = torch.as_tensor(np.concatenate([r for _, r in chunks]), dtype=torch.int64).to(dev)
        self.spans, o = [], 0
        for g, r in chunks:            # (structure key, [a, b) of ``all_idx``)
            self.spans.append(((g, len(r)), o, o + len(r)))
            o += len(r)
        whole = self.whole = _WholeSet(model, t, ds, flags=(hx, hy))
        self.pack, self.names, self.vec = whole.pack, whole.names, whole.vec
        # staging rows shared by the structures (they run one after the other): at most C rows of each matrix
        cmax = max(len(r) for _, r in chunks)
        self.stage = types.SimpleNamespace(
            x1=torch.zeros(cmax, X, device=dev), x2=torch.zeros(cmax, X, device=dev) if whole.n_x2 else None,
            y=torch.zeros(cmax, int(ds.y.numel()) // n, dtype=ds.y.dtype, device=dev) if kind != 'pvae' else None,
            s=torch.zeros(cmax, dtype=ds.s.dtype, device=dev) if t.use_s else None)
        self.loss_keys = list(model._loss_tensors(eng))
        # every chunk's loss pass normalises by the whole set's counts; its plan is built with local rows (``row0`` 0)
        with borrowed(model, t.use_s, self.counts, 0, rng=True):      # (the warm-up passes draw)
            self.parts = {}
            for key, a, b in self.spans:
                if key not in self.parts:
                    self.parts[key] = _ChunkPart(self, key, a, b)
            self.graph_final = _capture(whole.finalize)
            self.graph = self.graph_final

    def run(self):
        m = self.model
        eng = m.engine()
        eng.join_side()
        eng.iters = m.finished_training_iters
        keep = eng.plan
        for plan in {id(p.plan): p.plan for p in self.parts.values() if p.plan is not None}.values():
            plan.set_beta(*eng.betas())          # (the annealing coefficient is data of the plans, not of the graphs)
        self.pack.zero_()                        # (loss scalars and column moments are sums over the chunks)
        for key, a, b in self.spans:             # the host's share per chunk: which rows, then one replay
            part = self.parts[key]
            part.idx.copy_(self.all_idx[a:b])
            part.graph.replay()
        K.counter_add(eng.rng_ctr, 1)            # every chunk drew at the same counter value: ONE draw event, as in one replay
        eng._noise_stale = True
        eng.plan = keep
        self.graph_final.replay()
        return report(m, self.t, self.names, self.vec, self.loss_keys)


class _ChunkPart:
    """one STRUCTURE of a row-chunked evaluation: the chunks of ``rows_n`` rows of one (has_x2, has_y) group -- its loss plan,
    its row block (``_Rows``) and its captured sequence, which evaluates the rows ``idx`` (data-set positions, device
    data refilled by the host before a replay) and leaves their partials in the owner's buffer of the whole set.  A group
    the loss pass ignores (the supervised-only VFAE's unlabeled rows) has no plan: inference and statistics only."""

    def __init__(self, owner, key, a, b):
        (gx, gy), r = key
        self.owner, self.model, self.t, self.rows_n, self.gx, self.gy = owner, owner.model, owner.t, r, gx, gy
        m, kind, st = owner.model, owner.t.kind, owner.stage
        eng = m.engine()
        dev = st.x1.device
        self.idx = torch.zeros(r, dtype=torch.int64, device=dev)
        self.idx32 = torch.zeros(r, dtype=torch.int32, device=dev)
        flag = lambda v: torch.full((r,), int(v), dtype=torch.int64, device=dev)
        ds = self.ds = types.SimpleNamespace(
            x1=st.x1[:r], x2=st.x2[:r] if st.x2 is not None else None, s=st.s[:r] if st.s is not None else None,
            y=st.y[:r] if st.y is not None else None, has_x2=flag(gx) if kind != 'vfae' else None,
            has_y=flag(gy) if kind != 'pvae' else None)
        self.idx.copy_(owner.all_idx[a:b])
        self._stage()
        # the loss plan of this structure, built by the ordinary path on the staged rows (also the warm-up of its kernels)
        self.plan = None
        if not (kind == 'vfae' and not eng.cfg.semi_supervised and not gy):
            with warnings.catch_warnings():      # (a homogeneous chunk has empty data groups by construction)
                warnings.simplefilter('ignore')
                m.run_on_batch(train_mode=False, **_loss_pass_kw(kind, ds))
            self.plan = eng.plan
            assert len(self.plan.rows) == r and self.plan.B == r
        nb = K.col_moment_blocks(r)
        self.blk = _Rows(m, owner.t, ds, self.plan, {'x1': nb, 'x2': nb} if gx else {'x1': nb})
        self.graph = _capture(self._sequence, eng)

    def _stage(self):
        """the rows ``idx`` of the data set into the staging rows: dense rows by one gather, ``CsrRows`` by the feed launch"""
        full, ds = self.owner.ds, self.ds
        self.idx32.copy_(self.idx)
        for k in ('x1',) + (('x2',) if (self.gx and ds.x2 is not None) else ()):
            src, dst = getattr(full, k), getattr(ds, k)
            if isinstance(src, CsrRows):
                src.gather_rows(dst, self.idx32)
            elif src.dtype == torch.float32:
                torch.index_select(src, 0, self.idx, out=dst)
            else:
                dst.copy_(src.index_select(0, self.idx))
        if ds.y is not None:
            ds.y.copy_(full.y.reshape(self.owner.whole.n, -1).index_select(0, self.idx))
        if ds.s is not None:
            ds.s.copy_(full.s.reshape(-1).index_select(0, self.idx))

    def _sequence(self):
        m, ds, own, t, r = self.model, self.ds, self.owner, self.t, self.rows_n
        eng, p, whole = m.engine(), self.plan, self.owner.whole
        cfg = eng.cfg
        self._stage()
        if p is not None:
            # --- evaluation-mode losses of these rows: the fused forward on the structure's plan, the whole set's normalisers
            eng.plan = p
            _feed_x(p, ds.x1, ds.x2 if cfg.has_pert and self.gx else None)
            if cfg.has_pert and not self.gx and p.universal:
                p.XSRC[p.B:].zero_()
            if p.universal:      # the batch-independent plan reads the composition as data: one plan serves every group
                if cfg.has_pert:
                    p.hx_dev.fill_(int(self.gx))
                if cfg.has_y:
                    p.hy_dev.fill_(int(self.gy))
                    p.y_dev.copy_(ds.y.reshape(-1))
                if p.global_counts:
                    p.gcounts_dev.copy_(own.gcounts)
            elif t.cont:
                p.ylab.copy_(ds.y.reshape(r, -1))
            elif cfg.has_y:
                p.set_labels_device(ds.y)
            if t.use_s:
                _feed_s(p, ds.s.to(torch.int32), cfg.L)
            p.retarget_rows(self.idx32)          # every draw is the one its row gets in a plan of the whole set
            eng.training = False
            pending = eng._rng_pending
            eng.draw_noise(bump=False)           # (the counter advances once, behind the last chunk: ``_ChunkedEval.run``)
            eng._rng_pending = pending
            eng.forward()
            whole.slot('loss')[:_N_LOSS].add_(eng.arena.loss[:_N_LOSS])      # float64 sums, in chunk order
        if t.use_s:
            self.blk.feed_s(ds.s.to(torch.int32))
        # this chunk's partials: per-row results to their data-set positions, column moments folded
        whole.collect(self.blk, self.blk.infer(), self.idx, whole.mats(ds.x1, ds.x2 if self.gx else None),
                      lambda tag, s, part: fold_col_blocks(whole.slot('part' + s, 1, 3, whole.X), part))


CACHE_KEYS = _EvalGraph.CACHE_KEYS + (_ChunkedEval.CACHE_KEY,)      # every cache of evaluators a model holds (``DGMMixin``)
