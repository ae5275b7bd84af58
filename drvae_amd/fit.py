"""The ``fit`` protocol of the three models: epoch loop, whole-set evaluation,
rolling-mean early stopping and the snapshot policy of the reference
(src/DrVAE.py:743-877, src/PVAE.py:554-672, src/VFAE.py:523-656), on top of the fused step.

Two ways to feed the epoch loop:
  * a ``drvae_amd.data.DeviceBatcher`` -- the dataset lives in HBM, batches are drawn on the
    device, and every step is ONE hipGraph replay (no host<->device traffic, one host sync
    per epoch for the logged train loss);
  * any iterable of batch tuples (e.g. the reference's ``torch.utils.data.DataLoader``):
    compatibility path, one ``run_on_batch`` per tuple.
"""
import time
import warnings
from collections import OrderedDict

import numpy as np
import torch

from . import engine as E
from . import metrics as MET
from .sparse_rows import CsrRows


class EarlyStopping:
    """The patience / rolling-mean / snapshot controller spelled out inline in the reference's
    ``fit`` (src/DrVAE.py:755-766, 829-868).  One ``update`` per epoch."""

    def __init__(self, epochs, early_stop, patience=50, patience_increase=15, improvement_threshold=0.999,
                 memory_length=3, save_model_after=0):
        self.epochs, self.early_stop = epochs, early_stop
        self.patience, self.patience_increase = patience, patience_increase
        self.improvement_threshold = improvement_threshold
        self.memory_length, self.save_model_after = memory_length, save_model_after
        self.best = -np.inf
        self.rolling = np.array([], dtype=float)
        self.since_improvement = 0
        self.snapshotted = False

    def update(self, epoch, valid_obj):
        """-> dict(snapshot, stop, patience_hit, continuing, rolling_mean, best_before)"""
        self.since_improvement += 1
        self.rolling = np.append(self.rolling, valid_obj)[-self.memory_length:]
        out = dict(best_before=self.best, rolling=self.rolling.copy(), snapshot=False, stop=False,
                   patience_hit=False, continuing=False)
        score = out['rolling_mean'] = self.rolling.mean()
        if score * self.improvement_threshold > self.best:      # False for nan: no improvement
            self.patience = max(self.patience, epoch + self.patience_increase)
            self.best = score
            self.since_improvement = 0
        if (self.early_stop and self.since_improvement == self.save_model_after) or \
                (self.patience <= epoch and not self.snapshotted):
            self.snapshotted = out['snapshot'] = True
        if self.patience <= epoch:
            out['patience_hit'] = True
            if self.early_stop:
                if not self.snapshotted:
                    self.snapshotted = out['snapshot'] = True
                out['stop'] = True
            else:                                               # keep training to the last epoch
                out['continuing'] = True
                self.patience = self.epochs + 1
                self.snapshotted = False
        out['best'] = self.best
        return out

    def on_interrupt(self):
        """KeyboardInterrupt: snapshot unless one was already taken (src/DrVAE.py:869-874)"""
        take = not self.snapshotted
        self.snapshotted = True
        return take


_REC = 'RMSE: {:.3f} R2: {:.3f} Pearson: {:.3f}'
_NAN4 = ('rmse', 'r2', 'pearr', 'll')


class FitMixin:
    """evaluate_performance / fit for ``ELBOModel`` (``self.kind`` selects the model's variant)."""
    fit_patience = 50         # src/DrVAE.py:756, src/PVAE.py:567 (VFAE: 40, src/VFAE.py:536)

    # ------------------------------------------------------------------ metrics
    def eval_y_prediction(self, pred, proba, ylab):
        if getattr(self, 'type_y', 'discrete') != 'discrete':
            return MET.eval_y_regression(pred, ylab)
        return MET.eval_y_prediction(pred, proba, ylab, self.dim_y)

    def _np(self, t):
        return t.detach().cpu().numpy()

    @torch.no_grad()
    def _evaluate(self, x1, x2, s, y, has_x2, has_y, return_full_data=False):
        """one pass of losses + means-only inference + metrics over a row set
        (src/DrVAE.py:640-741, src/PVAE.py:479-552, src/VFAE.py:472-521)"""
        kind = self.kind
        dev = next(self.parameters()).device
        dv = lambda t: None if t is None else t.to(dev)
        x1, x2, y, has_x2, has_y = dv(x1), dv(x2), dv(y), dv(has_x2), dv(has_y)
        perf = OrderedDict()
        kw = dict(x1=x1, s=s)
        if kind != 'vfae':
            kw.update(x2=x2, has_x2=has_x2)
        if kind != 'pvae':
            kw.update(y=y, has_y=has_y)
        try:
            losses = self.run_on_batch(train_mode=False, **kw)
            perf['losses'] = OrderedDict((k, v.clone()) for k, v in losses.items())
        except Exception as e:          # the reference evaluates on regardless (src/DrVAE.py:648-654)
            if kind == 'pvae':
                raise
            print('Warning, computation of losses failed in evaluation!')
            print(e)
            perf['losses'] = None
        res = self.forward(x1, s)
        parts = []
        if kind != 'pvae':
            yidx = torch.nonzero(has_y.reshape(-1)).reshape(-1)
            cont = getattr(self, 'type_y', 'discrete') != 'discrete'
            ylab = y.reshape(y.shape[0], -1)[yidx] if cont else y.reshape(-1)[yidx]
            for k, v in self.eval_y_prediction(res['pred'][yidx], res['proba'][yidx], ylab).items():
                perf['y_' + k] = v
            if cont:
                parts.append('Y: RMSE: {:.3f} R2: {:.3f} Pearson: {:.3f}'.format(perf['y_rmse'], perf['y_r2'],
                                                                                 perf['y_pearr']))
            else:
                parts.append('Y: Accuracy: {:.3f}% AUROC: {:.3f} AUPR: {:.3f}'.format(
                    perf['y_acc'] * 100., perf['y_auroc'], perf['y_aupr']))
        for k, v in self.eval_x_reconstruction(x1, *res['px1']).items():
            perf['x1_' + k] = v
        parts.append('X1: ' + _REC.format(perf['x1_rmse'], perf['x1_r2'], perf['x1_pearr']))
        x2idx = None
        if kind != 'vfae':
            x2idx = torch.nonzero(has_x2.reshape(-1)).reshape(-1)
            if len(x2idx) > 0:
                x2p = x2[x2idx]
                rp = self.eval_x_reconstruction(x2p, *[t_[x2idx] for t_ in res['px2'][:3]])
                for k, v in rp.items():
                    perf['x2_' + k] = v
                parts.append('X2: ' + _REC.format(perf['x2_rmse'], perf['x2_r2'], perf['x2_pearr']))
            else:
                for k in _NAN4:
                    perf['x2_' + k] = np.nan
                parts.append('X2: no x2 data')
        if return_full_data:
            perf['z1'] = self._np(res['z1'])
            if kind != 'vfae':
                perf['z2'] = self._np(res['z2'])
                perf['x2_pert'] = self._np(res['x2_pert'])
            if kind != 'pvae':
                perf['pred'] = self._np(res['pred'])
                perf['proba'] = self._np(res['proba'])
            if kind != 'vfae':
                self._evaluate_identity_pert(perf, res, x1, x2, s, x2idx, yidx if kind == 'drvae' else None,
                                             ylab if kind == 'drvae' else None)
        perf['model_class'] = self.__class__.__name__
        return perf, '\t '.join(parts)

    def _evaluate_identity_pert(self, perf, res, x1, x2, s, x2idx, yidx, ylab):
        """the extra report with the perturbation function set to the identity
        (src/DrVAE.py:696-738, src/PVAE.py:514-549)"""
        res2 = self.forward_w_pert_identity(x1, x2, s)
        if yidx is not None:
            for k, v in self.eval_y_prediction(res2['pred'][yidx], res2['proba'][yidx], ylab).items():
                perf['y_wI_' + k] = v
        if len(x2idx) > 0:
            x2p = x2[x2idx]
            for tag, key in (('x2_wI_', 'px2'), ('x2_rec_', 'px2_rec')):
                rp = self.eval_x_reconstruction(x2p, *[t_[x2idx] for t_ in res2[key][:3]])
                for k, v in rp.items():
                    perf[tag + k] = v
            q1, q2 = res2['z1'][x2idx].double(), res2['z2'][x2idx].double()
            pz = res['z2'][x2idx].double()
            perf['qz1mu_qz2mu_rmse'] = float(torch.sqrt(((q1 - q2) ** 2).mean()))
            perf['pz2Fz1mu_qz2mu_rmse'] = float(torch.sqrt(((pz - q2) ** 2).mean()))
            qz1 = [t[x2idx].contiguous() for t in res2['qz1']]
            qz2 = [t[x2idx].contiguous() for t in res2['qz2']]
            pz2 = [t[x2idx].contiguous() for t in res['pz2']]
            perf['KL_qz2_qz1'] = float(self.encoder_z1.kldivergence_perx(*(qz2 + qz1)).mean())
            perf['KL_qz2_pz2Fz1'] = float(self.encoder_z1.kldivergence_perx(*(qz2 + pz2)).mean())
        else:
            for tag in ('x2_wI_', 'x2_rec_'):
                for k in _NAN4:
                    perf[tag + k] = np.nan
            for k in ('qz1mu_qz2mu_rmse', 'pz2Fz1mu_qz2mu_rmse', 'KL_qz2_qz1', 'KL_qz2_pz2Fz1'):
                perf[k] = np.nan

    def evaluate_performance_on_dataset(self, ds, return_full_data=False, chunk_rows=None):
        """Whole-set evaluation (src/DrVAE.py:797,821 call it on the train and on the validation set every epoch).  For
        an HBM-resident dataset it is ONE hipGraph replay and ONE device->host copy: eval-mode losses, means-only
        inference, reconstruction statistics and the prediction metrics captured once per (model, dataset) -- see
        ``_EvalGraph``.  That includes the regression head (``type_y='cont'``: rmse / R^2 / Pearson r from ``dv_reg_metrics``) and
        models conditioned on the nuisance variable (``use_s``; with ``use_MMD`` for ``kernel_MMD='rbf_fourier' | 'identity'``
        and 2 <= dim_s <= 8, the penalty as its two grouped launches) and the count decoders (``type_rec='binary' | 'poisson' |
        'nb' | 'zinb'``, with ``x_transform`` / ``library_size``: ``dv_recon_rows``' count kinds -- row statistics at the scaled mean
        and the count log-likelihood in one pass; the reported ``ll`` is the negative binomial's for ``'nb'``, the zero-inflated
        log-likelihood for ``'zinb'`` (its statistics are taken at the negative-binomial mean, never at (1 - pi) times it) and
        nan for the other two, as on the step-by-step path).  ``return_full_data`` (arrays for the caller), host datasets and the
        other MMD kernels take the step-by-step path (``'nb'``: ``x1_rec`` / ``x2_pert`` are the means, ``px1`` = (mu, theta);
        ``'zinb'``: the negative-binomial means, ``px1`` = (mu, theta, dropout logit)).

        ``chunk_rows`` (default: ``self.eval_chunk_rows``; None: everything above, unchanged): an integer C >= 1 evaluates the
        set in row chunks of at most C rows -- the same (perf, text), the whole set's numbers, in device memory that holds
        C x dim_x buffers and per-row arrays only; a ``CsrRows`` matrix is never densified beyond a chunk (``_ChunkedEval``).
        Refused, never answered by another path: ``use_MMD`` models and data parallelism (``NotImplementedError``), a
        host-resident set, ``return_full_data=True``, any other value of C (``ValueError``)."""
        if chunk_rows is None:
            chunk_rows = getattr(self, 'eval_chunk_rows', None)
        if chunk_rows is not None:
            chunk_rows = _ChunkedEval.check_chunk_rows(chunk_rows)
            if return_full_data:
                raise ValueError('evaluate_performance_on_dataset: return_full_data=True returns rows x genes arrays; it cannot '
                                 'be combined with a chunk size (chunk_rows / eval_chunk_rows = %d)' % chunk_rows)
            return _ChunkedEval.get(self, ds, chunk_rows).run()
        g = lambda k: getattr(ds, k, None)
        ev = None if return_full_data else _EvalGraph.get(self, ds)
        if ev is not None:
            return ev.run()

        def rows(k):
            # sparse rows (``CsrRows``): the step-by-step path on a TRANSIENT dense copy -- one feed launch (``gather_rows``)
            # writes the whole set; the copy lives for the duration of this evaluation
            x = g(k)
            if not isinstance(x, CsrRows):
                return x
            out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
            return x.gather_rows(out, torch.arange(x.shape[0], dtype=torch.int32, device=x.device))
        return self._evaluate(rows('x1'), rows('x2'), g('s'), g('y'), g('has_x2'), g('has_y'), return_full_data)

    # ------------------------------------------------------------- the objective
    def _valid_objective(self, perf):
        """what early stopping maximises (src/DrVAE.py:822-825, src/PVAE.py:617, src/VFAE.py:600-603)"""
        if self.kind == 'pvae':
            return perf['x1_pearr'] + perf['x2_pearr']
        if getattr(self, 'type_y', 'discrete') != 'discrete':         # src/DrVAE.py:824-825
            v = perf['y_r2'] + perf['y_pearr'] + perf['x1_pearr']
        else:
            v = perf['y_auroc'] + perf['y_aupr'] + perf['x1_pearr']
        return v + perf['x2_pearr'] if self.kind == 'drvae' else v

    def _batch_kwargs(self, batch):
        if self.kind == 'vfae':
            x1, s, y, has_y = batch
            return dict(x1=x1, s=s, y=y, has_y=has_y)
        x1, x2, s, y, has_x2, has_y = batch
        if self.kind == 'pvae':
            return dict(x1=x1, x2=x2, s=s, has_x2=has_x2)
        return dict(x1=x1, x2=x2, s=s, y=y, has_x2=has_x2, has_y=has_y)

    def _train_objective(self, loss):
        v = loss['RECL']
        return v + self.yloss_rate * loss['YL'] if 'YL' in loss else v

    def _log_losses(self, epoch, seen, n_data, frac, loss):
        keys = [k for k in ('CMPL', 'ELBO', 'RECL', 'PERT', 'YL') if k in loss]
        txt = '\t'.join('{}: {:.3f}'.format(k, float(loss[k])) for k in keys)
        self.w2log('training epoch: {} [{}/{} ({:.0f}%)]\t{}'.format(epoch, seen, n_data, 100. * frac, txt))

    # --------------------------------------------------------------- epoch loops
    def _epoch_device(self, batcher, epoch, verbose):
        """one epoch of hipGraph replays fed by the device batcher; returns the mean train objective"""
        eng = self.engine()
        self._assert_arena_aliased()
        batcher.bind(eng, counts=getattr(self, '_global_counts', None), dp=self._dp)
        eng.add_noise = bool(self.add_noise)
        eng.iters = self.finished_training_iters
        # (use_s: the nuisance classes travel with the feed when the batcher carries them; else host-driven gathers: feed())
        resident_feed = not eng.cfg.use_s or bool(getattr(batcher, 'carry_s', False))
        if resident_feed:
            batcher.begin_epoch()           # this epoch's index table; the graph gathers batch b itself
            if getattr(batcher, 'bucketed', False):
                eng.use_capture(eng.plan.key)      # (one captured step per number-of-pairs bucket: this one's, if any)
        else:
            batcher.feed()
        if getattr(eng, '_graph_key', None) != eng.plan.key or getattr(eng, '_graph_noise', None) != eng.add_noise \
                or getattr(eng, '_graph_feed', None) is not eng.plan.live_feed:
            eng.capture(split_for_allreduce=self._allreduce is not None)
            eng._graph_noise = eng.add_noise
            bucketed = getattr(batcher, 'bucketed', False)
            if bucketed:
                eng.stash_capture()         # (under this plan's key: begin_epoch below selects another)
            if self._allreduce is None and not (bucketed and getattr(eng, '_side_cus', None)):
                eng.tune_partition()        # CU split of the two launch chains, by timing (state restored)
            if resident_feed:
                batcher.rebase()            # (the tuning replays advanced the step counter: re-base the table)
        if getattr(batcher, 'bucketed', False):         # a plan per number-of-pairs bucket: capture the missing ones
            def cap(e):
                e.capture(split_for_allreduce=self._allreduce is not None)
                e._graph_noise = e.add_noise
            batcher.prepare_epoch(cap)
        with eng.partition():
            return self._epoch_device_body(eng, batcher, epoch, verbose)

    def _epoch_device_body(self, eng, batcher, epoch, verbose):
        n_b = len(batcher)
        every = max(10, n_b / 10)
        total = torch.zeros((), device=eng.dev)
        # single process: the launch that assembles a step's loss scalars also adds them to ``eng.loss_sum`` -- nothing
        # sits between two replays on the critical chain's stream (three tiny torch launches per step did: 54 steps x
        # ~40 us per epoch at cfg 2).  Under data parallelism the step's scalars are the exchanged ones: summed here
        in_graph = self._allreduce is None
        side = eng.flag_side if getattr(eng, '_side_graph', None) is not None else None
        if in_graph:
            eng.loss_sum.zero_()
            if side is not None:           # (the side chain's stream runs the assembling launch)
                side.wait_stream(torch.cuda.current_stream())
        for b in range(n_b):
            if eng.plan.live_feed is None:
                batcher.feed()
            else:
                batcher.select(b)              # (bucketed sampler feed: this batch's plan; otherwise nothing)
            eng.replay(allreduce=self._allreduce)
            if not in_graph:
                total += self._train_objective(self._loss_tensors(eng))
            if verbose and b % every == 0:
                self._log_losses(epoch, b * batcher.batch_size, len(batcher.dataset), b / n_b, self._loss_tensors(eng))
        self.finished_training_iters = eng.iters
        if eng.plan.live_feed is not None and epoch < self.epochs:
            batcher.draw_ahead()           # (the next epoch's table: queued behind the running steps)
        if in_graph:
            if side is not None:
                torch.cuda.current_stream().wait_stream(side)
            sums = OrderedDict((k, eng.loss_sum[E.LOSS_IDX[k]]) for k in self._loss_tensors(eng))
            total = self._train_objective(sums)
        # the epoch's ONE host sync: the objective and the sticky words of the device-side waits travel in one copy (a second
        # wait left the device idle once more per epoch)
        eng.join_side()
        if eng.dev.type == 'cuda' and torch.is_tensor(total):
            both = torch.stack([total.reshape(()).double(), eng.sync_err[0::2].abs().sum().double()]).cpu().tolist()
            if both[1] != 0:
                eng.check_sync()           # (raises with the wait sites)
            return both[0] / n_b
        mean = float(total) / n_b
        eng.check_sync()
        return mean

    def _graph_step(self, kw):
        """One train step of a tuple-loader batch through ONE captured graph whatever the batch's mix of pairs / labels
        (the reference's own input pipeline yields a different mix every batch, src/run_drvae.py:150-162): the batch goes
        into the buffers of the batch-independent plan (``set_batch``: device-to-device copies + its flags), the
        captured step turns the flags into group masks itself (dv_batch_masks).  The first batch of a size runs
        eagerly (iteration 0 carries beta_pert = 0.01) and the capture follows."""
        eng = self._batch_to_engine(dp=True, **kw)
        eng.add_noise = bool(self.add_noise)
        eng.iters = self.finished_training_iters
        fresh = getattr(eng, '_graph_key', None) != eng.plan.key or getattr(eng, '_graph_noise', None) != eng.add_noise \
            or getattr(eng, '_graph_feed', None) is not eng.plan.live_feed
        if fresh and eng.iters == 0:
            eng.train_step(allreduce=self._allreduce)
        else:
            if fresh:
                eng.capture(split_for_allreduce=self._allreduce is not None)
                eng._graph_noise = eng.add_noise
            with eng.partition():
                eng.replay(allreduce=self._allreduce)
        self.finished_training_iters = eng.iters
        return self._loss_tensors(eng)

    def _epoch_loader(self, loader, epoch, verbose):
        self._assert_arena_aliased()
        n_b = len(loader)
        every = max(10, n_b / 10)
        total = None
        eng = self.engine()
        # tuple loaders: one batch-independent plan + one captured graph for every batch composition (opt out:
        # ``model.universal_plan = False`` -> a plan per structure, eager launches)
        mode = getattr(self, 'universal_plan', True)       # True | False | 'eager' (the universal plan, eager launches)
        graph = bool(mode) and eng.universal_ok() and eng.dev.type == 'cuda' and \
            getattr(self, '_global_counts', None) is None
        if graph:
            eng.universal = True
            graph = mode != 'eager'
        for b, batch in enumerate(loader):
            self.train()
            loss = self._graph_step(self._batch_kwargs(batch)) if graph else \
                self.run_on_batch(train_mode=True, **self._batch_kwargs(batch))
            v = self._train_objective(loss)
            total = v.clone() if total is None else total + v
            if verbose and b % every == 0:
                self._log_losses(epoch, b * len(batch[0]), len(loader.dataset), b / n_b, loss)
        return float(total) / n_b

    def _warn_skipped_steps(self, epoch, before):
        """(``max_grad_norm``) one warning for an epoch in which the non-finite guard skipped steps; returns the running count"""
        now = self.grad_clip_stats()['n_skipped']
        if now > before:
            warnings.warn('epoch %d: %d train step(s) skipped for a non-finite gradient (%d so far); parameters and '
                          'optimiser state were left as they were' % (epoch, now - before, now))
        return now

    def _fit_weights(self):
        """the weights ``fit`` evaluates and snapshots: the parameter average (``averaged_parameters()``) of a model built
        with ``ema_decay`` unless ``self.ema_eval`` is false, else the live ones (a null context: nothing happens)"""
        import contextlib
        if getattr(self, 'ema_decay', None) is not None and getattr(self, 'ema_eval', True):
            return self.averaged_parameters()
        return contextlib.nullcontext()

    def fit(self, train_loader, valid_loader, add_noise=False, verbose=False, early_stop=False,
            model_filename='best_model.pth'):
        """Train for ``self.epochs`` epochs with the reference's validation / early-stopping /
        snapshot protocol (signature and log lines of src/DrVAE.py:743)."""
        from .data import DeviceBatcher, require_counts
        if getattr(self, 'x_transform', None) is not None or getattr(self, 'library_size', False):
            for ld in (train_loader, valid_loader):      # raw-count inputs: x >= 0, checked once, outside the step
                if getattr(ld, 'dataset', None) is not None:
                    require_counts(ld.dataset, 'fit')
        if getattr(self, 'dispersion', 'gene-cell') == 'gene-batch':
            from .data import require_classes
            for ld in (train_loader, valid_loader):      # a theta per nuisance class: 0 <= s < dim_s, checked once as well
                if getattr(ld, 'dataset', None) is not None:
                    require_classes(ld.dataset, int(self.dim_s), 'fit')
        np.set_printoptions(precision=4)
        ctl = EarlyStopping(self.epochs, early_stop, patience=self.fit_patience)
        self.w2log('Starting training at: {}'.format(time.strftime('%c')))
        epoch = 0
        skipped = self.grad_clip_stats()['n_skipped'] if self._max_grad_norm is not None else 0
        try:
            self.add_noise = add_noise
            for epoch in range(1, self.epochs + 1):
                t = time.time()
                if isinstance(train_loader, DeviceBatcher):
                    train_loss = self._epoch_device(train_loader, epoch, verbose)
                else:
                    train_loss = self._epoch_loader(train_loader, epoch, verbose)
                skipped = self._warn_skipped_steps(epoch, skipped) if self._max_grad_norm is not None else 0
                # (``ema_decay``: the two evaluations and the snapshot see the averaged weights unless ``ema_eval`` is off)
                with self._fit_weights():
                    train_perf, train_str = self.evaluate_performance_on_dataset(train_loader.dataset)
                    self.w2log('====> Epoch: {}\tIter: {}'.format(epoch, self.finished_training_iters))
                    self.w2log('Train: sec/epoch: {:.2f}\tAvg train loss: {:9.4f}\t{}'.format(time.time() - t, train_loss,
                                                                                         train_str))
                    t = time.time()
                    valid_perf, perf_str = self.evaluate_performance_on_dataset(valid_loader.dataset)
                    valid_loss = self._valid_objective(valid_perf)
                    self.w2log('Valid: sec/epoch: {:.2f}\tValid set loss: {:9.4f}\t{}'.format(time.time() - t, valid_loss,
                                                                                          perf_str))
                    d = ctl.update(epoch, valid_loss)
                    self.w2log('Valid rolling mem: {}\tmean: {:.4f}\tbest: {:.4f}'.format(d['rolling'], d['rolling_mean'],
                                                                                        d['best_before']))
                    if d['snapshot']:
                        if self.dp_rank == 0:        # (data parallelism: the replicas are identical; one writer)
                            self.save_to_file(model_filename)
                        self.w2log('* Snapshotting at epoch {}'.format(epoch))
                if d['patience_hit']:
                    self.w2log('Early stopping at: {} with train: {:.4f} valid: {:.4f} evaluate_valid_obj: {:.4f} '
                               'best_valid_obj: {:.4f}'.format(epoch, train_loss, valid_loss, d['rolling_mean'],
                                                               d['best']))
                    if d['stop']:
                        break
                    self.w2log('Continuing')
        except KeyboardInterrupt:
            self.w2log('KeyboardInterrupt')
            if ctl.on_interrupt() and self.dp_rank == 0:
                with self._fit_weights():
                    self.save_to_file(model_filename)
                self.w2log('* Snapshotting at epoch {}'.format(epoch))
        self.w2log('Finished training at: {}'.format(time.strftime('%c')))
        self._fit_controller = ctl
        return


class _EvalGraph:
    """The whole-set evaluation of one dataset as a captured launch sequence (round 4).

    What ``_evaluate`` does step by step -- with a host round trip behind nearly every number: index lists from
    ``torch.nonzero``, numpy combinations of the reconstruction partials, ``float()`` of every metric -- is recorded
    here ONCE into a hipGraph over the dataset's own HBM-resident tensors:
      * the evaluation-mode loss scalars of the fused step's forward (Philox draws from the device counter) on a plan of
        the whole set, its inputs gathered device-to-device from the dataset;
      * the means-only inference ``forward`` (block level: the same HIP kernels);
      * ``dv_recon_row_stats`` / ``dv_col_moments`` and their float64 combination, the Gaussian log-likelihood mean; for the
        count decoders (``type_rec='binary' | 'poisson' | 'nb' | 'zinb'``) the decoder's FINISHED heads and ``dv_recon_rows``' count kinds:
        statistics at the mean scaled by x1's size factor (``library_size``; for the x2 targets too), the negative binomial's
        log-likelihood rows (the zero-inflated ones for 'zinb', at the same mean, from the [theta | logit] columns of the heads), the scaled mean stored in place of the mean head for ``dv_col_moments``;
      * accuracy / AUROC / AUPR by sort + scan on the device (``metrics.*_dev``: no compaction, no host decisions); for the
        regression head rmse / R^2 / Pearson r of the means (``dv_reg_metrics``: one launch, two-pass float64 sums);
      * ``use_s``: the whole set's plan carries the nuisance classes on the device (``_Plan.carry_nuisance``) and the sequence
        feeds them from ``ds.s`` (``dv_nuisance_feed``: the loss pass's one-hot columns and class vector, and the one-hot operand
        of the inference's encoder / decoder chains); the MMD penalty's value comes from ``dv_mmd_grouped_fwd`` -- a term with an
        empty side counts 0 there, where ``_evaluate``'s host-list plan compares with one random row;
    every scalar lands in one float64 vector.  ``run()`` = set the annealing coefficient, replay, ONE copy to the host.
    The group index lists (rows with a second profile / a label) are data of the DATASET, taken once; the arrays
    themselves -- inputs, labels, regression targets, nuisance classes -- are read by the replay, so a dataset edited in
    place is evaluated as edited."""

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
        from . import kernels as K
        x1 = getattr(ds, 'x1', None)
        if isinstance(x1, CsrRows) or isinstance(getattr(ds, 'x2', None), CsrRows):
            return None          # (sparse rows: the captured evaluation reads dense matrices in place -- declined)
        if not (torch.is_tensor(x1) and x1.is_cuda):
            return None
        if next(model.parameters()).device != x1.device:
            return None
        # (the decision is a function of the model's configuration and the dataset's tensors alone: every rank of a
        # data-parallel job decides alike)
        use_s = bool(getattr(model, 'use_s', False))
        cont = model.kind != 'pvae' and getattr(model, 'type_y', 'discrete') != 'discrete'
        if use_s and getattr(model, 'use_MMD', False) and not (
                getattr(model, 'kernel_MMD', 'rbf_fourier') in K.MMD_GROUPED_KIND and 2 <= int(model.dim_s) <= K.MMD_MAX_CLASSES):
            return None          # (the penalty's grouped launches cover these; the rest keeps the host-list path)
        need = ('x1',) + (('x2', 'has_x2') if model.kind != 'vfae' else ()) + (('y', 'has_y') if model.kind != 'pvae' else ()) \
            + (('s',) if use_s else ())
        parts = [getattr(ds, k, None) for k in need]
        if not all(torch.is_tensor(t) and t.device == x1.device for t in parts):
            return None          # (a host-resident label / flag array would be a pageable copy under capture)
        if cont and not ds.y.is_floating_point():
            return None
        if use_s and (ds.s.is_floating_point() or ds.s.is_complex() or ds.s.dtype == torch.bool):
            return None
        cache = _EvalGraph.cache(model)
        # the captured launches point into the engine's arena, plan and layer chains: ``.cpu().cuda()`` / ``.to()`` retire
        # the engine (DGMMixin._apply) and a graph of the old one would read freed parameters -- the engine's identity is
        # part of the signature (and ``_apply`` drops the cache)
        eng = model.engine()
        # data parallelism: the ROWS of a whole-set evaluation are sharded over the ranks (every rank holds the dataset; its
        # heavy passes run on rows [n r / W, n (r + 1) / W) only), the partials meet in ONE all-reduce -- see ``_sequence_partial``
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
                import warnings         # so does the step-by-step path, which this dataset now takes
                warnings.warn('drvae_amd: the captured whole-set evaluation could not be built (%s: %s); evaluating step '
                              'by step' % (type(e).__name__, e))
                ev = cache[id(ds)] = _EvalGraph.__new__(_EvalGraph)
                ev.sig, ev.graph = sig, None
        return ev if ev.graph is not None else None

    def __init__(self, model, ds, sig, dp=None):
        self.model, self.sig = model, sig
        self.graph = None
        kind = model.kind
        dev = ds.x1.device
        self.cont = kind != 'pvae' and getattr(model, 'type_y', 'discrete') != 'discrete'
        self.use_s = bool(getattr(model, 'use_s', False))
        # the count decoders ('binary' / 'poisson' / 'nb' / 'zinb'): finished heads, ``dv_recon_rows``' count kinds (``_rows_pass``)
        self.fam = E.REC_FAMILIES[model.type_rec]
        self.rec_kind = None if self.fam.recon_kind == E.RECON_KIND[None] else model.type_rec      # (as ``K.recon_rows`` names it)
        self.dp, self.full = dp, None
        if dp is not None:
            # this rank's rows as VIEWS of the dataset's tensors; the normalisers of the loss pass are the whole set's counts,
            # the Philox draws are keyed by the row's position in the whole set (``row0``): the shards' terms add up to the
            # one-rank evaluation's
            import types
            from . import dist as D
            rank, world = dp
            n_all = int(ds.x1.shape[0])
            self.lo, self.hi = n_all * rank // world, n_all * (rank + 1) // world
            self.full = ds
            hx = getattr(ds, 'has_x2', None) if kind != 'vfae' else None
            hy = getattr(ds, 'has_y', None) if kind != 'pvae' else None
            zer = np.zeros(n_all, np.int64)
            eng0 = model.engine()
            self.counts = D.global_counts(hx.cpu().numpy() if hx is not None else zer, hy.cpu().numpy() if hy is not None else zer,
                                          eng0.cfg.kind, eng0.cfg.semi_supervised, local=True)
            ds = types.SimpleNamespace(**{k: (getattr(ds, k)[self.lo:self.hi] if torch.is_tensor(getattr(ds, k, None)) else None)
                                          for k in ('x1', 'x2', 's', 'y', 'has_x2', 'has_y')})
        self.ds = ds
        g = lambda k: getattr(ds, k, None)
        # rows of the groups (once per dataset: a host sync each)
        self.x2idx = torch.nonzero(g('has_x2').reshape(-1).to(dev)).reshape(-1) if kind != 'vfae' else None
        self.yidx = torch.nonzero(g('has_y').reshape(-1).to(dev)).reshape(-1) if kind != 'pvae' else None
        self.x2idx32 = self.x2idx.to(torch.int32) if self.x2idx is not None else None
        self.yidx32 = self.yidx.to(torch.int32) if self.yidx is not None else None
        # the loss plan of the whole set: built by the ordinary path (host index lists), then reused
        eng = model.engine()
        keep, keep_training, was_training = eng.plan, eng.training, model.training
        keep_counts, keep_row0, keep_carry = model.__dict__.get('_global_counts'), eng.row0, eng.carry_s
        try:
            model.eval()
            # ``use_s``: the whole set's plan carries the nuisance classes on the device (``_Plan.carry_nuisance``): nothing in it
            # depends on the set's composition of classes, ``_sequence`` feeds them from ``ds.s``.  A plan of its own key: the
            # plan a bound ``DeviceBatcher`` replays stays in the cache (``_evict_plans`` never drops a captured step's)
            eng.carry_s = self.use_s
            kw = dict(x1=g('x1'), s=g('s'))
            if kind != 'vfae':
                kw.update(x2=g('x2'), has_x2=g('has_x2'))
            if kind != 'pvae':
                kw.update(y=g('y'), has_y=g('has_y'))
            self.kw = kw
            if dp is not None:
                model._global_counts, model._row0_override = self.counts, self.lo
            model.run_on_batch(train_mode=False, **kw)          # (also the warm-up of every kernel of the sequence)
            self.plan = eng.plan
            n_in = int(ds.x1.shape[0])
            rows = np.asarray(self.plan.rows)
            self.sel = None if (len(rows) == n_in and (rows == np.arange(n_in)).all()) else torch.as_tensor(rows, device=dev)
            if dp is not None:
                self._shard_layout()
            self._sequence()                                    # warm-up of the rest (allocations, code objects)
            torch.cuda.synchronize()
            gph = torch.cuda.CUDAGraph()
            eng.join_side()
            # no garbage collection while a stream is capturing, as in ``FusedStep.capture``: a collected cycle may own the
            # graph of a retired model's evaluation (``_EvalGraph`` <-> model), and destroying a graph during a capture
            # aborts the process
            import gc
            gc.collect()
            gc_was_on = gc.isenabled()
            gc.disable()
            try:
                with torch.cuda.graph(gph):
                    self.names, self.vec, self.loss_keys = self._sequence()
                if dp is not None:
                    self._finalize_full()                           # (warm-up)
                    torch.cuda.synchronize()
                    self.graph_final = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(self.graph_final):
                        self._finalize_full()
            finally:
                if gc_was_on:
                    gc.enable()
            self.graph = gph
        finally:
            eng.plan, eng.training, eng.carry_s = keep, keep_training, keep_carry
            model.train(was_training)
            if dp is not None:
                model.__dict__.pop('_row0_override', None)
                if keep_counts is None:
                    model.__dict__.pop('_global_counts', None)
                else:
                    model._global_counts = keep_counts
                eng.row0 = keep_row0

    def _sequence(self):
        """the launch sequence (eager for the warm-up, then under capture); -> (names, float64 vector, loss keys)"""
        from . import kernels as K
        m, ds, kind = self.model, self.ds, self.model.kind
        eng, p = m.engine(), self.plan
        eng.plan = p
        dev = ds.x1.device
        # --- evaluation-mode losses on the whole set: the fused forward on this plan, inputs from the dataset
        p.feed_active = False
        x1 = ds.x1.to(torch.float32)
        p.XSRC[:p.B].copy_(x1.index_select(0, self.sel) if self.sel is not None else x1)
        if eng.cfg.has_pert:
            x2 = ds.x2.to(torch.float32)
            p.XSRC[p.B:].copy_(x2.index_select(0, self.sel) if self.sel is not None else x2)
        n_in = int(ds.x1.shape[0])
        if self.cont:      # the regression targets of the plan's rows (read by the replay: targets edited in place count)
            y2 = ds.y.reshape(n_in, -1).to(torch.float32)
            p.ylab.copy_(y2.index_select(0, self.sel) if self.sel is not None else y2)
        if self.use_s:
            # the nuisance classes, device to device -- the launch ``_Plan.set_s_device`` makes: one-hot columns of the stacked
            # encoder / decoder rows and the class vector the grouped MMD penalty reads; then the same for the inference
            # below: one_hot(s) of every row of the set, the decoder's stacked rows [z1; z2] use the same classes twice
            s32 = ds.s.reshape(-1).to(torch.int32)
            K.nuisance_feed(p.SOHe, p.SOHd, p.s_cls, (s32.index_select(0, self.sel) if self.sel is not None else s32).contiguous(),
                            pair_rows=p.pair_idx if p.Np else None, L=eng.cfg.L)
            if not hasattr(self, 'soh_d'):
                S, reps = eng.cfg.dim_s, (2 if kind != 'vfae' else 1)
                self.soh_e = torch.zeros(n_in, (S + 3) // 4 * 4, device=dev)[:, :S]
                self.soh_d = torch.zeros(n_in * reps, (S + 3) // 4 * 4, device=dev)[:, :S]
                self.s_all = torch.zeros(n_in, dtype=torch.int32, device=dev)
            K.nuisance_feed(self.soh_e, self.soh_d, self.s_all, s32.contiguous(), L=2 if kind != 'vfae' else 1)
        eng.training = False
        eng.draw_noise()
        eng.forward()
        losses = m._loss_tensors(eng)
        # every scalar of the evaluation lands in ONE float64 vector: [losses | y metrics | x1 metrics | x2 metrics]
        names = ['loss_' + k for k in sorted(E.LOSS_IDX, key=E.LOSS_IDX.get)]      # (all seven; ``run`` picks the model's)
        n_loss = len(names)
        if kind != 'pvae':
            names += ['y_rmse', 'y_r2', 'y_pearr'] if self.cont else ['y_auroc', 'y_aupr', 'y_acc']
        names += ['x1_' + k for k in _NAN4]
        has_x2 = kind != 'vfae' and (len(self.x2idx) > 0 if self.dp is None else self.full_n_x2 > 0)
        if has_x2:
            names += ['x2_' + k for k in _NAN4]
        if not hasattr(self, 'vec'):
            self.vec = torch.zeros(len(names), dtype=torch.float64, device=dev)
        vec = self.vec
        vec[:n_loss].copy_(eng.arena.loss[:n_loss])
        o = n_loss
        # --- means-only inference + metrics (the tail: dv_rank_metrics / dv_recon_finalize, no sort, no host decisions)
        res = self._infer()
        if self.dp is not None:
            self._sequence_partial(res, vec[:n_loss])
            return names, vec, list(losses)
        if kind != 'pvae':
            self._y_metrics(res, vec[o:o + 3])
            o += 3
        self._recon(ds.x1, res['px1'], None, vec[o:o + 4], 'x1', res['px_bias'], res['tail1'])
        o += 4
        if has_x2:
            self._recon(ds.x2, res['px2'], self.x2idx32, vec[o:o + 4], 'x2', res['px_bias'], res['tail2'])
        return names, vec, list(losses)

    # ------------------------------------------------------------ rows sharded over ranks (data parallelism, round 6)
    def _shard_layout(self):
        """ONE flat float64 exchange buffer for the whole evaluation, laid out for the WHOLE set: [loss scalars | proba | pred |
        x1: row statistics, log-likelihood rows, column-moment blocks of every rank | x2: the same].  Every rank writes its
        rows' slots (zeros elsewhere), one sum all-reduce leaves the complete arrays on every rank (float32 / int32 values are
        exact in float64, and x + 0 = x), and the finalising launches -- the same kernels as without sharding -- run on them."""
        from . import kernels as K
        m, full, kind = self.model, self.full, self.model.kind
        dev = full.x1.device
        rank, world = self.dp
        n, X, Y = int(full.x1.shape[0]), int(full.x1.shape[1]), (m.dim_y if kind != 'pvae' else 0)
        self.n_all = n
        bounds = [(n * r // world, n * (r + 1) // world) for r in range(world)]
        self.full_x2idx32 = self.full_yidx32 = None
        self.full_n_x2 = 0
        blk2 = 1
        if kind != 'vfae':
            hx = full.has_x2.reshape(-1).to(dev) != 0
            self.full_x2idx32 = torch.nonzero(hx).reshape(-1).to(torch.int32)
            self.full_n_x2 = int(self.full_x2idx32.numel())
            per = [int(hx[a:b].sum()) for a, b in bounds]
            blk2 = max(K.col_moment_blocks(max(c, 1)) for c in per)
        if kind != 'pvae':
            self.full_yidx32 = torch.nonzero(full.has_y.reshape(-1).to(dev)).reshape(-1).to(torch.int32)
        blk1 = max(K.col_moment_blocks(b - a) for a, b in bounds)
        self.blk = {'x1': blk1, 'x2': blk2}
        self._alloc_full(n, X, Y, world * blk1, world * blk2, dev)

    def _alloc_full(self, n, X, Y, n_part1, n_part2, dev):
        """the flat float64 buffer of the WHOLE set's partials -- ``n_part1`` / ``n_part2`` column-moment blocks for x1 / x2 --
        and the complete per-row arrays the finalising launches read (``_finalize_full``)"""
        o, self.off = 0, {}
        # (regression head: the ``pred`` slot carries the n x Y float means; no class probabilities, no int32 buffers)
        for name, size in (('loss', 8), ('proba', 0 if self.cont else n * Y), ('pred', n * Y if self.cont else (n if Y else 0)),
                           ('rows1', n * 6), ('ll1', n),
                           ('part1', n_part1 * 3 * X), ('rows2', n * 6 if self.full_n_x2 else 0),
                           ('ll2', n if self.full_n_x2 else 0), ('part2', n_part2 * 3 * X if self.full_n_x2 else 0)):
            self.off[name] = (o, size)
            o += size
        self.pack = torch.zeros(o, dtype=torch.float64, device=dev)
        f32 = lambda *shape: torch.zeros(*shape, device=dev)
        self.g_rows = {'x1': f32(n, 6), 'x2': f32(n, 6)}
        self.g_ll = {'x1': f32(n), 'x2': f32(n)}
        if Y and self.cont:
            self.g_pred = f32(n, Y)
        elif Y:
            self.g_proba, self.g_pred32 = f32(n, Y), torch.zeros(n, dtype=torch.int32, device=dev)
            self.g_y32 = torch.zeros(n, dtype=torch.int32, device=dev)

    def _slot(self, name):
        o, size = self.off[name]
        return self.pack[o:o + size]

    def _sequence_partial(self, res, loss_vec):
        """this rank's share of the evaluation's partials into the exchange buffer (captured; no finalising launch)"""
        from . import kernels as K
        m, ds, kind = self.model, self.ds, self.model.kind
        rank, world = self.dp
        lo, hi, X = self.lo, self.hi, int(ds.x1.shape[1])
        self.pack.zero_()
        self._slot('loss')[:loss_vec.numel()].copy_(loss_vec)
        if kind != 'pvae' and self.cont:
            self._slot('pred').view(self.n_all, m.dim_y)[lo:hi].copy_(res['pred'])
        elif kind != 'pvae':
            Y = m.dim_y
            self._slot('proba').view(self.n_all, Y)[lo:hi].copy_(res['proba'])
            self._slot('pred')[lo:hi].copy_(res['pred'].reshape(-1))
        bias = res['px_bias']
        for tag, x, key, sel in (('x1', ds.x1, 'px1', None), ('x2', getattr(ds, 'x2', None), 'px2', self.x2idx32)):
            if tag == 'x2' and (kind == 'vfae' or not self.full_n_x2):
                continue
            x = x.to(torch.float32)
            M = int(x.shape[0])
            n_sel = int(sel.numel()) if sel is not None else M
            buf = self.__dict__.setdefault('_recon_bufs', {})
            if tag not in buf:
                buf[tag] = (torch.empty(M, 6, device=x.device),
                            torch.zeros(self.blk[tag], 3, X, dtype=torch.float64, device=x.device), torch.empty(M, device=x.device))
            rows, part, ll = buf[tag]
            x_rec, ll = self._rows_pass(rows, ll, x, res[key], bias, res['tail' + key[-1]])
            t = '1' if tag == 'x1' else '2'
            self._slot('rows' + t).view(self.n_all, 6)[lo:hi].copy_(rows)
            if ll is not None:      # ('binary' / 'poisson': no reported log-likelihood, the slot stays zero and is not read)
                self._slot('ll' + t)[lo:hi].copy_(ll)
            if n_sel > 0:
                nb = K.col_moment_blocks(n_sel)
                K.col_moments(None, x, x_rec, sel=sel, part=part[:nb], r_bias=bias[0] if bias is not None else None)
                self._slot('part' + t).view(world, self.blk[tag], 3, X)[rank, :nb].copy_(part[:nb])

    def _finalize_full(self):
        """behind the all-reduce: the complete arrays out of the exchange buffer, then the SAME finalising launches as the
        unsharded evaluation (``dv_rank_metrics``, ``dv_recon_finalize``) over the whole set -> ``vec``"""
        from . import kernels as K
        m, kind, full = self.model, self.model.kind, self.full
        vec, n, X = self.vec, self.n_all, int(full.x1.shape[1])
        n_loss = len(E.LOSS_IDX)
        vec[:n_loss].copy_(self._slot('loss')[:n_loss])
        o = n_loss
        if kind != 'pvae' and self.cont:
            # (the targets are read by the replay: a dataset edited in place is evaluated as edited)
            self.g_pred.copy_(self._slot('pred').view(n, m.dim_y))
            K.reg_metrics(vec[o:o + 3], self.g_pred, full.y.reshape(n, -1).to(torch.float32), sel=self.full_yidx32)
            o += 3
        elif kind != 'pvae':
            Y = m.dim_y
            self.g_proba.copy_(self._slot('proba').view(n, Y))
            self.g_pred32.copy_(self._slot('pred'))
            self.g_y32.copy_(full.y.reshape(-1))      # (read by the replay: a dataset edited in place is evaluated as edited)
            self._rank_metrics(self.g_proba, self.g_y32, self.g_pred32, self.full_yidx32, vec[o:o + 3], n)
            o += 3
        for tag, t, sel in (('x1', '1', None), ('x2', '2', self.full_x2idx32)):
            if tag == 'x2' and (kind == 'vfae' or not self.full_n_x2):
                continue
            self.g_rows[tag].copy_(self._slot('rows' + t).view(n, 6))
            self.g_ll[tag].copy_(self._slot('ll' + t))
            part = self._slot('part' + t).view(-1, 3, X)
            K.recon_finalize(vec[o:o + 4], self.g_rows[tag], part, X, sel=sel, n=int(sel.numel()) if sel is not None else n,
                             ll=self.g_ll[tag] if self.fam.eval_ll else None)
            o += 4

    def _rank_metrics(self, proba, y32, pred32, yidx32, out3, n_rows):
        """[auroc, aupr, acc] of the labeled rows ``yidx32`` from the pair-counting kernel (sort + scan beyond its range)"""
        from . import kernels as K
        m = self.model
        n_lab, Y = int(yidx32.numel()), m.dim_y
        if n_lab > K.RANK_MAX_ROWS or n_lab == 0:
            idx = yidx32.long()
            v = MET.eval_y_prediction_dev(pred32.index_select(0, idx), proba.index_select(0, idx), y32.index_select(0, idx).long(), Y)
            out3.copy_(torch.stack([v['auroc'].reshape(()), v['aupr'].reshape(()), v['acc'].reshape(())]))
            return
        if not hasattr(self, 'rank_counts'):
            n_cls = 1 if Y == 2 else Y
            self.rank_counts = torch.zeros(n_cls, n_lab, 4, dtype=torch.int32, device=proba.device)
            self.rank_out = torch.zeros(2 * n_cls + 1, dtype=torch.float64, device=proba.device)
        if Y == 2:
            K.rank_metrics(out3, self.rank_counts, proba, y32, pred32=pred32, sel=yidx32, c0=1, n_cls=1, binary=True)
        else:
            K.rank_metrics(self.rank_out, self.rank_counts, proba, y32, pred32=pred32, sel=yidx32, c0=0, n_cls=Y, binary=False)
            out3[0:1].copy_(self.rank_out[0:2 * Y:2].mean().reshape(1))
            out3[1:2].copy_(self.rank_out[1:2 * Y:2].mean().reshape(1))
            out3[2:3].copy_(self.rank_out[2 * Y:2 * Y + 1])

    def _y_metrics(self, res, out3):
        """accuracy / ROC-AUC / average precision of the labeled rows (src/DGMMixin.py:158-190) -> out3 = [auroc, aupr, acc]"""
        from . import kernels as K
        m, ds = self.model, self.ds
        dev = ds.x1.device
        n_lab, Y = int(self.yidx.numel()), m.dim_y
        if self.cont:      # regression head: out3 = [rmse, r2, pearr] of the means (src/DGMMixin.py:181-188), one launch
            K.reg_metrics(out3, res['pred'], ds.y.reshape(int(ds.x1.shape[0]), -1).to(torch.float32), sel=self.yidx32)
            return
        if n_lab > K.RANK_MAX_ROWS or n_lab == 0:      # (beyond the pair-counting kernel's range: the sort + scan formulation)
            y = ds.y.to(dev)
            ylab = y.reshape(-1).index_select(0, self.yidx)
            v = MET.eval_y_prediction_dev(res['pred'].index_select(0, self.yidx), res['proba'].index_select(0, self.yidx), ylab, Y)
            out3.copy_(torch.stack([v['auroc'].reshape(()), v['aupr'].reshape(()), v['acc'].reshape(())]))
            return
        if not hasattr(self, 'y32'):
            n_cls = 1 if Y == 2 else Y
            self.y32 = torch.zeros(int(ds.x1.shape[0]), dtype=torch.int32, device=dev)
            self.pred32 = torch.zeros_like(self.y32)
            self.rank_counts = torch.zeros(n_cls, n_lab, 4, dtype=torch.int32, device=dev)
            self.rank_out = torch.zeros(2 * n_cls + 1, dtype=torch.float64, device=dev)
        self.y32.copy_(ds.y.reshape(-1))
        self.pred32.copy_(res['pred'].reshape(-1))
        proba = res['proba']
        if Y == 2:
            K.rank_metrics(out3, self.rank_counts, proba, self.y32, pred32=self.pred32, sel=self.yidx32, c0=1, n_cls=1, binary=True)
        else:       # macro average over the one-vs-rest problems (nan as soon as one class's value is: the mean propagates it)
            K.rank_metrics(self.rank_out, self.rank_counts, proba, self.y32, pred32=self.pred32, sel=self.yidx32, c0=0,
                           n_cls=Y, binary=False)
            out3[0:1].copy_(self.rank_out[0:2 * Y:2].mean().reshape(1))
            out3[1:2].copy_(self.rank_out[1:2 * Y:2].mean().reshape(1))
            out3[2:3].copy_(self.rank_out[2 * Y:2 * Y + 1])

    def _infer(self):
        """``forward`` (means-only inference, src/DrVAE.py:253-311) with its two heavy blocks on the fused step's layer
        chains: the encoder's heads as ONE (mu | logvar) product, and the decoder ONCE over the stacked rows [z1; z2]
        with its (mu | std) heads as one product -- 3 launches of 2n rows instead of 6 of n (the block modules compute
        every head with a launch of its own).  The small blocks in between are the model's own modules."""
        from .chain import _Chain
        from . import kernels as K
        m, ds, kind = self.model, self.ds, self.model.kind
        eng = m.engine()
        n, Z, X = int(ds.x1.shape[0]), eng.cfg.dim_z1, eng.cfg.dim_x
        dev = ds.x1.device
        if not hasattr(self, 'c_dec'):
            if self.sel is not None:
                self.c_enc = _Chain(eng.L_enc, n, dev)
            self.c_dec = _Chain(eng.L_decx, n * (2 if kind != 'vfae' else 1), dev)
            self.zd = torch.zeros(n * (2 if kind != 'vfae' else 1), (Z + 3) // 4 * 4, device=dev)[:, :Z]
        if self.sel is None:
            # q(z1|x1) of every row has just been computed by the loss pass (``_sequence`` runs it first): evaluation mode adds
            # no input noise, its encoder input rows [0, n) ARE x1 in dataset order, same layer chain, same kernels -- the
            # first n rows of its heads' buffer are this product (8192 rows: 15 GFLOP not computed twice).  The raw-count
            # switches change nothing here: ``_sequence`` clears ``eng.training`` before the pass, so ``_encoder_forward``
            # takes sigma = 0 and hands the split feed ``noise=None`` -- its encoder rows are T(x1) exactly (log1p(x1) with
            # ``x_transform='log1p'``), what ``forward`` feeds the encoder
            Q = self.plan.c_enc.out[-1][:n]
        else:
            x1 = m._enc_x(ds.x1.to(torch.float32))      # (``x_transform='log1p'``: the encoder reads log1p(x1))
            if X % 4:
                # rows padded to 16 B (zero pads): the first layer's product then runs on the LDS-DMA kernels (``_Chain``)
                if not hasattr(self, 'x1p'):
                    self.x1p = torch.zeros(n, (X + 3) // 4 * 4, device=dev)[:, :X]
                self.x1p.copy_(x1)
                x1 = self.x1p
            Q = self.c_enc.forward([x1] + ([self.soh_e] if self.use_s else []))
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
        raw = bool(self.rec_kind is None and X <= K.RECON_ROWS_MAX_X and self.c_dec.raw_softplus_ok())
        PX = self.c_dec.forward([self.zd] + ([self.soh_d] if self.use_s else []), raw_last=raw)
        res['px_bias'] = (lh.b[:X], lh.b[X:2 * X], lh.shift1) if raw else None
        # (three heads, 'zinb': (mu, theta, logit) as ``forward`` returns it -- columns of the ONE buffer, so [theta | logit] is
        # the contiguous view from column X on that ``_rows_pass`` hands the row pass)
        nh = len(self.fam.heads)
        disp = getattr(m, 'dispersion', 'gene-cell')
        if disp != 'gene-cell':
            # a gene-wise theta: ``dv_recon_rows`` has no broadcast operand, so the finished theta row is written into a theta
            # block once per replay, as one row repeated (M x X words written and read), with the decoder's logit columns copied
            # behind it for 'zinb' -- then the recon kinds run as they are, and the numbers are ``_evaluate``'s key by key
            # (``fam`` is the family of ``type_rec`` as the recon kinds know it -- mean, theta[, logit]; the decoder's own heads
            # buffer is [mean] or [mean | logit])
            rows_all, nt = PX.shape[0], nh - 1
            if not hasattr(self, 'gtail'):
                self.gtail = torch.zeros(rows_all, nt * X, device=PX.device)
            T_ = self.gtail
            if disp == 'gene-batch':
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
        heads behind the mean as ONE view of the heads buffer (``_infer``): theta for 'nb', [theta | logit] for 'zinb', None
        for one head.  'binary' / 'poisson' report no log-likelihood (``_evaluate`` passes no second head: nan), 'nb' the
        negative binomial's, 'zinb' the zero-inflated one (its statistics are taken at the negative-binomial mean)."""
        from . import kernels as K
        from ._lib import GAUSS_SIGMA
        if self.rec_kind is not None:
            ll = ll if self.fam.eval_ll else None
            size = self.ds.x1.to(torch.float32) if getattr(self.model, 'library_size', False) else None
            K.recon_rows(rows, ll, x, px[0], tail, kind=self.rec_kind, size_from=size,
                         rec_out=px[0] if size is not None else None)
            return px[0], ll
        if x.shape[1] <= K.RECON_ROWS_MAX_X:
            K.recon_rows(rows, ll, x, px[0], px[1], bias=bias[:2] if bias is not None else None,
                         sd_shift=bias[2] if bias is not None else 0.0)
        else:
            K.recon_row_stats(rows, x, px[0])
            K.nll_rows_fwd(ll, x, px[0], px[1], mode=GAUSS_SIGMA)
        return px[0], ll

    def _recon(self, x, px, sel, out4, tag, bias=None, tail=None):
        """``eval_x_reconstruction`` (src/DGMMixin.py:128-156) over the rows ``sel`` (all when None): row statistics, column
        moments and log-likelihood rows from the HIP kernels, combined in float64 by ``dv_recon_finalize`` into ``out4`` =
        [rmse, r2, pearr, ll].  The statistics are taken over ALL rows and selected afterwards (no gathered copies of
        the x2 rows and their reconstructions).  Rows of up to 1024 genes: row statistics and log-likelihood rows in ONE pass
        (``dv_recon_rows``); ``bias`` = (bias_mu, bias_sd, shift): the heads are raw products, finished by the passes.
        ``px`` / ``tail``: the heads of these rows (``_rows_pass``: the count decoders' route)."""
        from . import kernels as K
        x = x.to(torch.float32)
        M, X = x.shape
        n = int(sel.numel()) if sel is not None else M
        assert bias is None or X <= K.RECON_ROWS_MAX_X
        buf = self.__dict__.setdefault('_recon_bufs', {})
        if tag not in buf:
            buf[tag] = (torch.empty(M, 6, device=x.device), torch.empty(K.col_moment_blocks(n), 3, X, dtype=torch.float64, device=x.device),
                        torch.empty(M, device=x.device))
        rows, part, ll = buf[tag]
        x_rec, ll = self._rows_pass(rows, ll, x, px, bias, tail)
        K.col_moments(None, x, x_rec, sel=sel, part=part, r_bias=bias[0] if bias is not None else None)
        K.recon_finalize(out4, rows, part, X, sel=sel, n=n, ll=ll)

    def run(self):
        m, kind = self.model, self.model.kind
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
        return self._report(dict(zip(self.names, self.vec.cpu().tolist())))  # THE host sync of the evaluation

    def _report(self, v):
        """(perf, text) of ``evaluate_performance_on_dataset`` from the evaluation's scalars by name"""
        m, kind = self.model, self.model.kind
        perf = OrderedDict()
        perf['losses'] = OrderedDict((k, torch.tensor(v['loss_' + k])) for k in self.loss_keys)
        parts = []
        if kind != 'pvae' and self.cont:
            for k in ('rmse', 'r2', 'pearr'):
                perf['y_' + k] = v['y_' + k]
            parts.append('Y: RMSE: {:.3f} R2: {:.3f} Pearson: {:.3f}'.format(perf['y_rmse'], perf['y_r2'], perf['y_pearr']))
        elif kind != 'pvae':
            for k in ('acc', 'auroc', 'aupr'):
                perf['y_' + k] = v['y_' + k]
            parts.append('Y: Accuracy: {:.3f}% AUROC: {:.3f} AUPR: {:.3f}'.format(perf['y_acc'] * 100., perf['y_auroc'], perf['y_aupr']))
        for k in _NAN4:
            perf['x1_' + k] = v['x1_' + k]
        parts.append('X1: ' + _REC.format(perf['x1_rmse'], perf['x1_r2'], perf['x1_pearr']))
        if kind != 'vfae':
            if 'x2_rmse' in v:
                for k in _NAN4:
                    perf['x2_' + k] = v['x2_' + k]
                parts.append('X2: ' + _REC.format(perf['x2_rmse'], perf['x2_r2'], perf['x2_pearr']))
            else:
                for k in _NAN4:
                    perf['x2_' + k] = np.nan
                parts.append('X2: no x2 data')
        perf['model_class'] = m.__class__.__name__
        return perf, '\t '.join(parts)


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


class _ChunkedEval(_EvalGraph):
    """``_EvalGraph``'s numbers for a data set evaluated ``C`` rows at a time (``evaluate_performance_on_dataset(chunk_rows=C)``,
    ``model.eval_chunk_rows``): a chunk is a rank in time.  The row-sharded evaluation of data parallelism already evaluates a
    row range with the whole set's normalisers and Philox keys and leaves partials that the unsharded finalising launches
    finish (``_finalize_full``); here the partials of every chunk land in ONE buffer of the whole set, one after the other.

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
      * Behind the last chunk the counter advances once -- where a one-replay evaluation leaves it -- and ``_finalize_full``
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
        kind, use_s = model.kind, bool(getattr(model, 'use_s', False))
        need = ('x1',) + (('x2', 'has_x2') if kind != 'vfae' else ()) + (('y', 'has_y') if kind != 'pvae' else ()) + \
            (('s',) if use_s else ())
        dev = next(model.parameters()).device
        for k in need:
            t = getattr(ds, k, None)
            if not ((torch.is_tensor(t) or isinstance(t, CsrRows)) and t.is_cuda and t.device == dev):
                raise ValueError('row-chunked evaluation (eval_chunk_rows) reads the data set on the model\'s device (%s): '
                                 '%r is %s' % (dev, k, 'missing' if t is None else 'host-resident or on another device'))
        if kind != 'pvae' and getattr(model, 'type_y', 'discrete') != 'discrete' and not ds.y.is_floating_point():
            raise ValueError("row-chunked evaluation: type_y='cont' reads floating-point targets")
        if use_s and (ds.s.is_floating_point() or ds.s.is_complex() or ds.s.dtype == torch.bool):
            raise ValueError('row-chunked evaluation: the nuisance classes are integers')
        ptrs = lambda t: (int(t.ptr.data_ptr()), int(t.idx.data_ptr()), int(t.val.data_ptr())) if isinstance(t, CsrRows) \
            else (int(t.data_ptr()),)
        eng = model.engine()
        sig = tuple(p for k in need for p in ptrs(getattr(ds, k))) + \
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
        import gc
        import types
        from . import dist as D
        self.model, self.sig, self.C, self.full = model, sig, C, ds
        kind = model.kind
        eng = model.engine()
        dev = ds.x1.device
        n, X = int(ds.x1.shape[0]), int(ds.x1.shape[1])
        if n < 1:
            raise ValueError('row-chunked evaluation: the data set has no rows')
        self.cont = kind != 'pvae' and getattr(model, 'type_y', 'discrete') != 'discrete'
        self.use_s = bool(getattr(model, 'use_s', False))
        self.fam = E.REC_FAMILIES[model.type_rec]
        self.rec_kind = None if self.fam.recon_kind == E.RECON_KIND[None] else model.type_rec
        self.dp = None
        # the grouping is data of the DATASET, taken once (a host sync per flag array), like ``x2idx`` / ``yidx`` of ``_EvalGraph``
        hx = (ds.has_x2.reshape(-1).cpu().numpy() != 0) if kind != 'vfae' else None
        hy = (ds.has_y.reshape(-1).cpu().numpy() != 0) if kind != 'pvae' else None
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
        # the whole set's partials and complete per-row arrays: ``_shard_layout``'s buffer with ONE column-moment block per matrix
        i32 = lambda rows: torch.as_tensor(np.nonzero(rows)[0], dtype=torch.int32).to(dev)
        self.n_all = n
        self.full_x2idx32 = i32(hx) if hx is not None else None
        self.full_yidx32 = i32(hy) if hy is not None else None
        self.full_n_x2 = int(hx.sum()) if hx is not None else 0
        self._alloc_full(n, X, model.dim_y if kind != 'pvae' else 0, 1, 1, dev)
        # staging rows shared by the structures (they run one after the other): at most C rows of each matrix
        cmax = max(len(r) for _, r in chunks)
        self.stage = types.SimpleNamespace(
            x1=torch.zeros(cmax, X, device=dev), x2=torch.zeros(cmax, X, device=dev) if self.full_n_x2 else None,
            y=torch.zeros(cmax, int(ds.y.numel()) // n, dtype=ds.y.dtype, device=dev) if kind != 'pvae' else None,
            s=torch.zeros(cmax, dtype=ds.s.dtype, device=dev) if self.use_s else None)
        names = ['loss_' + k for k in sorted(E.LOSS_IDX, key=E.LOSS_IDX.get)]
        if kind != 'pvae':
            names += ['y_rmse', 'y_r2', 'y_pearr'] if self.cont else ['y_auroc', 'y_aupr', 'y_acc']
        names += ['x1_' + k for k in _NAN4] + (['x2_' + k for k in _NAN4] if self.full_n_x2 else [])
        self.names, self.vec = names, torch.zeros(len(names), dtype=torch.float64, device=dev)
        self.loss_keys = list(model._loss_tensors(eng))
        keep, keep_training, was_training = eng.plan, eng.training, model.training
        keep_counts, keep_row0, keep_carry = model.__dict__.get('_global_counts'), eng.row0, eng.carry_s
        keep_pending, keep_ctr = eng._rng_pending, eng.rng_ctr.clone()
        # (no garbage collection while a stream is capturing: see ``_EvalGraph.__init__``)
        gc.collect()
        gc_was_on = gc.isenabled()
        gc.disable()
        try:
            model.eval()
            eng.carry_s = self.use_s
            # every chunk's loss pass normalises by the whole set's counts; its plan is built with local rows (``row0`` 0)
            model._global_counts, model._row0_override = self.counts, 0
            self.parts = {}
            for key, a, b in self.spans:
                if key not in self.parts:
                    self.parts[key] = _ChunkPart(self, key, a, b)
            self._finalize_full()                                   # (warm-up)
            torch.cuda.synchronize()
            self.graph_final = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph_final):
                self._finalize_full()
            self.graph = self.graph_final
        finally:
            if gc_was_on:
                gc.enable()
            eng.plan, eng.training, eng.carry_s, eng.row0, eng._rng_pending = keep, keep_training, keep_carry, keep_row0, keep_pending
            model.train(was_training)
            model.__dict__.pop('_row0_override', None)
            if keep_counts is None:
                model.__dict__.pop('_global_counts', None)
            else:
                model._global_counts = keep_counts
            eng.rng_ctr.copy_(keep_ctr)      # (the warm-up passes drew: building leaves the Philox counter where it found it)
            eng._noise_stale = True

    def run(self):
        from . import kernels as K
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
        return self._report(dict(zip(self.names, self.vec.cpu().tolist())))  # THE host sync of the evaluation


class _ChunkPart(_EvalGraph):
    """one STRUCTURE of a row-chunked evaluation: the chunks of ``rows`` rows of one (has_x2, has_y) group -- its loss plan,
    its inference chains and buffers and its captured sequence, which evaluates the rows ``idx`` (data-set positions, device
    data refilled by the host before a replay) and leaves their partials in the owner's buffer of the whole set.  A group
    the loss pass ignores (the supervised-only VFAE's unlabeled rows) has no plan: inference and statistics only."""

    def __init__(self, owner, key, a, b):
        import types
        (gx, gy), r = key
        self.owner, self.model, self.rows_n, self.gx, self.gy = owner, owner.model, r, gx, gy
        m, kind, st = owner.model, owner.model.kind, owner.stage
        eng = m.engine()
        dev = st.x1.device
        self.cont, self.use_s, self.fam, self.rec_kind, self.dp = owner.cont, owner.use_s, owner.fam, owner.rec_kind, None
        self.idx = torch.zeros(r, dtype=torch.int64, device=dev)
        self.idx32 = torch.zeros(r, dtype=torch.int32, device=dev)
        flag = lambda v: torch.full((r,), int(v), dtype=torch.int64, device=dev)
        self.ds = types.SimpleNamespace(
            x1=st.x1[:r], x2=st.x2[:r] if st.x2 is not None else None, s=st.s[:r] if st.s is not None else None,
            y=st.y[:r] if st.y is not None else None, has_x2=flag(gx) if kind != 'vfae' else None,
            has_y=flag(gy) if kind != 'pvae' else None)
        if self.use_s:      # one_hot(s) operands of the inference's encoder / decoder chains, the rows' classes
            S, reps = eng.cfg.dim_s, (2 if kind != 'vfae' else 1)
            self.soh_e = torch.zeros(r, (S + 3) // 4 * 4, device=dev)[:, :S]
            self.soh_d = torch.zeros(r * reps, (S + 3) // 4 * 4, device=dev)[:, :S]
            self.s_all = torch.zeros(r, dtype=torch.int32, device=dev)
        self.idx.copy_(owner.all_idx[a:b])
        self._stage()
        # the loss plan of this structure, built by the ordinary path on the staged rows (also the warm-up of its kernels)
        self.plan, self.sel = None, torch.zeros(0, dtype=torch.int64, device=dev)
        if not (kind == 'vfae' and not eng.cfg.semi_supervised and not gy):
            ds = self.ds
            kw = dict(x1=ds.x1, s=ds.s)
            if kind != 'vfae':
                kw.update(x2=ds.x2, has_x2=ds.has_x2)
            if kind != 'pvae':
                kw.update(y=ds.y, has_y=ds.has_y)
            with warnings.catch_warnings():      # (a homogeneous chunk has empty data groups by construction)
                warnings.simplefilter('ignore')
                m.run_on_batch(train_mode=False, **kw)
            self.plan, self.sel = eng.plan, None
            assert len(self.plan.rows) == r and self.plan.B == r
        self._sequence()                         # warm-up of the rest (allocations, code objects)
        torch.cuda.synchronize()
        eng.join_side()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self._sequence()

    def _stage(self):
        """the rows ``idx`` of the data set into the staging rows: dense rows by one gather, ``CsrRows`` by the feed launch"""
        full, ds, r = self.owner.full, self.ds, self.rows_n
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
            ds.y.copy_(full.y.reshape(self.owner.n_all, -1).index_select(0, self.idx))
        if ds.s is not None:
            ds.s.copy_(full.s.reshape(-1).index_select(0, self.idx))

    def _sequence(self):
        from . import kernels as K
        m, ds, own, r = self.model, self.ds, self.owner, self.rows_n
        eng, p = m.engine(), self.plan
        cfg = eng.cfg
        self._stage()
        if p is not None:
            # --- evaluation-mode losses of these rows: the fused forward on the structure's plan, the whole set's normalisers
            eng.plan = p
            p.feed_active = False
            p.XSRC[:p.B].copy_(ds.x1)
            if cfg.has_pert and self.gx:
                p.XSRC[p.B:].copy_(ds.x2)
            elif cfg.has_pert and p.universal:
                p.XSRC[p.B:].zero_()
            if p.universal:      # the batch-independent plan reads the composition as data: one plan serves every group
                if cfg.has_pert:
                    p.hx_dev.fill_(int(self.gx))
                if cfg.has_y:
                    p.hy_dev.fill_(int(self.gy))
                    p.y_dev.copy_(ds.y.reshape(-1))
                if p.global_counts:
                    p.gcounts_dev.copy_(own.gcounts)
            elif self.cont:
                p.ylab.copy_(ds.y.reshape(r, -1))
            elif cfg.has_y:
                p.set_labels_device(ds.y)
            if self.use_s:
                K.nuisance_feed(p.SOHe, p.SOHd, p.s_cls, ds.s.to(torch.int32).contiguous(),
                                pair_rows=p.pair_idx if p.Np else None, L=cfg.L)
            p.retarget_rows(self.idx32)          # every draw is the one its row gets in a plan of the whole set
            eng.training = False
            pending = eng._rng_pending
            eng.draw_noise(bump=False)           # (the counter advances once, behind the last chunk: ``_ChunkedEval.run``)
            eng._rng_pending = pending
            eng.forward()
            n_loss = len(E.LOSS_IDX)
            own._slot('loss')[:n_loss].add_(eng.arena.loss[:n_loss])      # float64 sums, in chunk order
        if self.use_s:
            K.nuisance_feed(self.soh_e, self.soh_d, self.s_all, ds.s.to(torch.int32).contiguous(), L=2 if m.kind != 'vfae' else 1)
        self._scatter(self._infer())

    def _scatter(self, res):
        """this chunk's partials into the owner's buffer: per-row results to their data-set positions, column moments folded"""
        from . import kernels as K
        m, ds, own, idx, kind = self.model, self.ds, self.owner, self.idx, self.model.kind
        n, X = own.n_all, int(ds.x1.shape[1])
        if kind != 'pvae' and self.cont:
            own._slot('pred').view(n, m.dim_y).index_copy_(0, idx, res['pred'].to(torch.float64))
        elif kind != 'pvae':
            own._slot('proba').view(n, m.dim_y).index_copy_(0, idx, res['proba'].to(torch.float64))
            own._slot('pred').index_copy_(0, idx, res['pred'].reshape(-1).to(torch.float64))
        bias = res['px_bias']
        for tag, t, x in (('x1', '1', ds.x1), ('x2', '2', ds.x2)):
            if tag == 'x2' and not self.gx:
                continue
            buf = self.__dict__.setdefault('_recon_bufs', {})
            if tag not in buf:
                buf[tag] = (torch.empty(self.rows_n, 6, device=x.device),
                            torch.zeros(K.col_moment_blocks(self.rows_n), 3, X, dtype=torch.float64, device=x.device),
                            torch.empty(self.rows_n, device=x.device))
            rows, part, ll = buf[tag]
            x_rec, ll = self._rows_pass(rows, ll, x, res['px' + t], bias, res['tail' + t])
            own._slot('rows' + t).view(n, 6).index_copy_(0, idx, rows.to(torch.float64))
            if ll is not None:      # ('binary' / 'poisson': no reported log-likelihood, the slot stays zero and is not read)
                own._slot('ll' + t).index_copy_(0, idx, ll.to(torch.float64))
            K.col_moments(None, x, x_rec, sel=None, part=part, r_bias=bias[0] if bias is not None else None)
            fold_col_blocks(own._slot('part' + t).view(1, 3, X), part)
