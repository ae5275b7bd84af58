"""The ``fit`` protocol of the three models: epoch loop, whole-set evaluation,
rolling-mean early stopping and the snapshot policy of the reference
(src/DrVAE.py:743-877, src/PVAE.py:554-672, src/VFAE.py:523-656), on top of the fused step.  The step-by-step
evaluation ``_evaluate`` lives here; the captured ones (one replay, row-sharded, row-chunked) in ``drvae_amd.evaluate``.

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
from .evaluate import _NAN4, _ChunkedEval, _EvalGraph, chunk_partition, fold_col_blocks, report_text  # noqa: F401 (re-exported)
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
        cont = getattr(self, 'type_y', 'discrete') != 'discrete'
        if kind != 'pvae':
            yidx = torch.nonzero(has_y.reshape(-1)).reshape(-1)
            ylab = y.reshape(y.shape[0], -1)[yidx] if cont else y.reshape(-1)[yidx]
            for k, v in self.eval_y_prediction(res['pred'][yidx], res['proba'][yidx], ylab).items():
                perf['y_' + k] = v
        for k, v in self.eval_x_reconstruction(x1, *res['px1']).items():
            perf['x1_' + k] = v
        x2idx = None
        if kind != 'vfae':
            x2idx = torch.nonzero(has_x2.reshape(-1)).reshape(-1)
            if len(x2idx) > 0:
                x2p = x2[x2idx]
                rp = self.eval_x_reconstruction(x2p, *[t_[x2idx] for t_ in res['px2'][:3]])
                for k, v in rp.items():
                    perf['x2_' + k] = v
        text = report_text(kind, kind != 'pvae' and cont, perf, x2idx is not None and len(x2idx) > 0)      # (and the nan of a set without x2)
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
        return perf, text

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
