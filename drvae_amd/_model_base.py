"""Shared wiring of the three ELBO models.  The reference spells the same skeleton out
three times (src/DrVAE.py, src/PVAE.py, src/VFAE.py); here one base class owns block
construction, inference ``forward`` and the mapping to the fused train step, and the
three public classes only carry their constructor signatures."""
import warnings
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn

from . import blocks as blk
from . import engine as E
from .DGMMixin import DeepGenerativeModelMixin
from .fit import FitMixin


# the annealing switches every model carries (src/DrVAE.py:92-97) and their defaults; ``anneal_lr_itermax`` is the 3000 the
# reference hard-codes (src/DGMMixin.py:101)
ANNEAL_DEFAULTS = OrderedDict(anneal_kl=False, anneal_kl_itermax=100, anneal_yloss=False, anneal_yloss_itermax=1,
                              anneal_learning_rate=False, anneal_lr_itermax=3000)


class ELBOModel(FitMixin, DeepGenerativeModelMixin, nn.Module):
    kind = None             # 'drvae' | 'pvae' | 'vfae'

    def _init_common(self, args):
        """store every ctor argument as an attribute (the reference does this with inspect,
        src/DrVAE.py:71-74) and set the hyper-parameters it hard-codes (src/DrVAE.py:79-97)."""
        device = args.pop('device', None)
        weight_norm = args.pop('weight_norm', False)
        # 'fp32' | 'bf16x3' | 'bf16x2' | 'bf16x1' (opt-in): the arithmetic of the chip-filling decoder-heads products, see
        # ``StepConfig.matmul`` ('bf16x1' is a bf16 product: label results computed with it as such)
        self._matmul = args.pop('matmul_precision', 'fp32')
        if self._matmul not in E.MATMUL_CHOICES:
            raise ValueError('matmul_precision must be one of %s' % (E.MATMUL_CHOICES,))
        # None | a positive number | inf: global-norm gradient clipping and the non-finite guard of the fused step, see
        # ``StepConfig.max_grad_norm``
        self._max_grad_norm = args.pop('max_grad_norm', None)
        if self._max_grad_norm is not None:
            self._max_grad_norm = float(self._max_grad_norm)
            if not self._max_grad_norm > 0.0:
                raise ValueError('max_grad_norm must be a positive number, inf or None, not %r' % (self._max_grad_norm,))
        # annealing schedules of the fused step (``StepConfig.anneal_*``): constructor arguments here, plain attributes in
        # the reference (src/DrVAE.py:92-97) -- both work until the engine is built (``engine``), a later change raises
        anneal = {k: args.pop(k, d) for k, d in ANNEAL_DEFAULTS.items()}
        # None | a number in (0, 1): the exponential moving average of the parameters kept by the optimiser sweep, see
        # ``StepConfig.ema_decay``; ``ema_eval``: ``fit`` evaluates and snapshots the averaged weights (default) or the live ones
        ema_decay = E.check_ema_decay(args.pop('ema_decay', None))
        # None | an integer >= 1: ``evaluate_performance_on_dataset`` (and so ``fit``) evaluates a device-resident set in row
        # chunks of at most so many rows, in device memory that does not grow with rows x genes (``evaluate._ChunkedEval``)
        eval_chunk_rows = args.pop('eval_chunk_rows', None)
        # raw-count inputs (EXTENSIONS, count decoders only; ``StepConfig.x_transform`` / ``library_size``): the encoder reads
        # log1p(x) while the likelihood keeps the raw counts; every decoder mean is scaled by the row's observed size factor
        x_transform, library_size = args.pop('x_transform', None), args.pop('library_size', False)
        # 'gene-cell' | 'gene' | 'gene-batch': a theta head, one inverse dispersion per gene, or one per (gene, nuisance class) with
        # ``use_s`` ('nb' / 'zinb'; ``StepConfig.dispersion``)
        self.dispersion = E.check_dispersion(args.pop('dispersion', 'gene-cell'), args.get('type_rec'),
                                             use_s=bool(args.get('use_s', False)))
        for k, v in args.items():
            setattr(self, k, v)
        for k, v in anneal.items():
            setattr(self, k, v)
        self.ema_decay, self.ema_eval = ema_decay, True
        self.eval_chunk_rows = eval_chunk_rows
        if eval_chunk_rows is not None:      # (what the configuration alone decides is refused here: ValueError / NotImplementedError)
            from .evaluate import _ChunkedEval
            _ChunkedEval.check_chunk_rows(eval_chunk_rows)
            _ChunkedEval.check_model(self)
        self.x_transform, self.library_size = x_transform, library_size
        self._counts_config()           # (a bad value, or a switch on a decoder that is no count decoder: ValueError)
        if not hasattr(self, 'anneal_yloss_offset'):
            self.anneal_yloss_offset = 0
        self._anneal_config()           # (a switch that is on with itermax <= 0: ValueError)
        self.wn = bool(weight_norm)   # reference: hard-coded False (src/DrVAE.py:79); exposed here
        self.bn = False
        self.prior_mu, self.prior_sg = 0., 1.
        if self.weight_decay is None:
            self.weight_decay = 0.
        self.kl_min = 2.
        self.finished_training_iters = 0
        self.add_noise = False        # set by the caller / fit(add_noise=...) (src/DrVAE.py:769)
        self._check_supported()
        self.nprng = np.random.RandomState(self.random_seed)
        torch.manual_seed(self.random_seed)
        self._build_blocks()
        self._dropout_notes()
        self._create_optimizer()
        if device is None:
            device = 'cuda' if torch.cuda.is_available() else 'cpu'
        self.to(device)

    def _check_supported(self):
        if self.type_rec not in E.REC_FAMILIES:      # src/DrVAE.py:124-131
            names = [repr(k) for k in E.REC_FAMILIES]
            raise ValueError('type_rec must be %s or %s' % (', '.join(names[:-1]), names[-1]))
        # 'binary' / 'poisson' point at blk.BernoulliDecoder / blk.PoissonDecoder, which the reference's blocks.py
        # does not define (its constructor raises AttributeError there): built here as labelled EXTENSIONS; 'nb' (the
        # negative binomial for overdispersed counts, blk.NegativeBinomialDecoder) and 'zinb' (its zero-inflated form,
        # blk.ZeroInflatedNegativeBinomialDecoder) are extensions the reference never names
        bad = []
        # use_s=True is an EXTENSION here: the reference crashes on it (torch.cat([z, s_raw]) of a float and an
        # integer tensor, src/DrVAE.py:438), so it is built from the evident intent -- one_hot(s) appended to the
        # inputs of encoder_z1 and decoder_x, and (use_MMD) the model-level MMD penalty -- and checked against the
        # oracle's restatement of that intent only (no reference output exists)
        if getattr(self, 'use_s', False) and (len(self.dim_h_en_z1) < 1 or len(self.dim_h_de_x) < 1):
            bad.append('use_s=True without hidden layers in encoder_z1 / decoder_x')
        if getattr(self, 'type_y', 'discrete') not in ('discrete', 'cont'):
            raise ValueError('Invalid type_y')
        if getattr(self, 'type_y', 'discrete') == 'cont' and self.kind == 'vfae' and getattr(self, 'semi_supervised', False):
            # the reference's own semi-supervised regression branch crashes (src/VFAE.py:386 passes the
            # 1-tuple returned by sample() on to torch.cat): nothing to be identical to.  Supervised-only
            # (labeled rows, squared-error y-loss, src/VFAE.py:351) runs and is supported
            bad.append("semi-supervised VFAE with type_y='cont'")
        if getattr(self, 'type_y', 'discrete') == 'cont' and not isinstance(getattr(self, 'prior_y', 'uniform'), str):
            bad.append("type_y='cont' with a data prior")
        if getattr(self, 'clf_1sig', False) and self.dim_y != 2:
            raise ValueError('Invalid combination of clf_1sig and dim_y')      # src/DrVAE.py:161
        # input_x_dropout (--x-dropout) is accepted and has NO effect, exactly as in the reference: its MLP
        # computes the dropped inputs and then concatenates the ORIGINAL ones (src/blocks.py:158-161)
        # dropout_rate > 0 (hard-coded 0. by every reference driver) runs in the fused step: ``_dropout_notes``
        if not 0. <= self.dropout_rate < 1.:
            raise ValueError('dropout_rate must lie in [0, 1)')
        pr = getattr(self, 'prior_y', 'uniform')
        if pr is not None and not isinstance(pr, str):       # a class prior given as data (src/DrVAE.py:83-85)
            assert isinstance(pr, np.ndarray) and len(pr) == self.dim_y
        if getattr(self, 'use_c', False) or getattr(self, 'use_m', False):
            bad.append('use_c/use_m')
        if bad:
            raise NotImplementedError('not covered by the fused MI355X step: ' + '; '.join(bad))

    # ------------------------------------------------------------------- blocks
    def _build_blocks(self):
        """same sub-module names and construction order as the reference, so that state_dict
        keys (and the parameter-init RNG stream) line up: src/DrVAE.py:112-183,
        src/PVAE.py:106-153, src/VFAE.py:103-165."""
        hp = dict(nonlin=self.nonlinearity, weight_norm=self.wn, batch_norm=self.bn, dropout_rate=self.dropout_rate)
        pri = dict(prior_mu=self.prior_mu, prior_sg=self.prior_sg)
        Z1 = self.dim_z1
        s_in = [self.dim_s] if getattr(self, 'use_s', False) else []       # src/DrVAE.py:134-135,179-180
        self.encoder_z1 = blk.DiagGaussianModule([self.dim_x] + s_in, self.dim_h_en_z1, Z1,
                                                 input_dropout_rates=[self.input_x_dropout] + [0.] * len(s_in), **pri, **hp)
        if self.kind in ('drvae', 'pvae'):
            self.dim_z2 = Z1
            self.decoder_z2Fz1 = blk.DiagGaussianModuleLinear([Z1], [], Z1, bias_only=False, **pri, **hp)
        if self.kind in ('drvae', 'vfae'):
            clf_in = [Z1, Z1] if (self.kind == 'drvae' and self.clf_z1z2) else [Z1]
            if getattr(self, 'type_y', 'discrete') == 'cont':      # regression head (src/DrVAE.py:166-169)
                self.encoder_y = blk.DiagGaussianModule(clf_in, self.dim_h_clf, self.dim_y, fixed_variance=0.05 ** 2,
                                                        constrain_means=True, **hp)
            else:
                self.encoder_y = blk.CategoricalDecoder(clf_in, self.dim_h_clf,
                                                        1 if getattr(self, 'clf_1sig', False) else self.dim_y, **hp)
            top_h = self.dim_h_en_z3 if self.kind == 'drvae' else self.dim_h_en_z2
            top_z = self.dim_z3 if self.kind == 'drvae' else self.dim_z2
            top = blk.DiagGaussianModule([Z1, self.dim_y], top_h, top_z, **pri, **hp)
            setattr(self, 'encoder_z3' if self.kind == 'drvae' else 'encoder_z2', top)
            self.decoder_z1 = blk.DiagGaussianModule([top_z, self.dim_y], self.dim_h_de_z1, Z1, **hp)
        dec = {'diag_gaussian': blk.DiagGaussianSigmaModule, 'binary': blk.BernoulliDecoder,
               'poisson': blk.PoissonDecoder, 'nb': blk.NegativeBinomialDecoder,
               'zinb': blk.ZeroInflatedNegativeBinomialDecoder}[self.type_rec]      # src/DrVAE.py:124-129
        gene = dict(dispersion=self.dispersion) if self.dispersion != 'gene-cell' else {}       # ('gene-cell': the call as it was)
        self.decoder_x = dec([Z1] + s_in, self.dim_h_de_x, self.dim_x, **hp, **gene)

    def _dropout_notes(self):
        """Hidden-layer dropout in the fused train step (``dropout_rate`` > 0): every hidden activation of every block is
        dropped in front of the layer that reads it -- the reference's ``dropout{i}`` (i > 1) and the ``dropout_mu`` /
        ``dropout_lv`` / ``dropout_sg`` / ``dropout_p`` in front of the heads.  Two LABELLED DIFFERENCES from the block-level
        path (and the reference), named once here in a warning:
          * shared head mask: the two heads of a block are one product over one input, so both read ONE keep mask where the
            reference draws two independent ones -- each head's marginal is the reference's, the joint is not;
          * a block without hidden layers is not dropped at all in the fused step (no hidden activation, no site): always
            ``decoder_z2Fz1``, whose log-variance head alone the reference drops, and any block built with an empty hidden list."""
        if not self.dropout_rate > 0:
            return
        hidden = OrderedDict(encoder_z1=self.dim_h_en_z1)
        if self.kind in ('drvae', 'pvae'):
            hidden['decoder_z2Fz1'] = []
        if self.kind in ('drvae', 'vfae'):
            hidden['encoder_y'] = self.dim_h_clf
            hidden['encoder_z3' if self.kind == 'drvae' else 'encoder_z2'] = \
                self.dim_h_en_z3 if self.kind == 'drvae' else self.dim_h_en_z2
            hidden['decoder_z1'] = self.dim_h_de_z1
        hidden['decoder_x'] = self.dim_h_de_x
        # (one head in the fused step: the classifier -- a regression head's log-variance is fixed, its layer is not in the
        # step's chain (``FusedStep.L_clf``) -- and a Bernoulli / Poisson decoder; the negative binomial has two, its
        # zero-inflated form three: all of them read the one mask)
        x_heads = len(E.rec_family(self.type_rec, self.dispersion).heads)
        two_heads = [n for n, h in hidden.items() if len(h) and n != 'encoder_y' and not (n == 'decoder_x' and x_heads == 1)]
        undropped = [n for n, h in hidden.items() if not len(h)]
        three = ' (all three heads of the zero-inflated decoder_x)' if x_heads == 3 and 'decoder_x' in two_heads else ''
        warnings.warn('dropout_rate=%g in the fused train step differs from the block-level path in two labelled ways: '
                      'both heads share ONE keep mask in %s%s; no dropout at all (no hidden layer) in %s'
                      % (self.dropout_rate, ', '.join(two_heads) or 'no block', three, ', '.join(undropped) or 'no block'))

    def _anneal_config(self):
        """the annealing attributes as they stand now, as ``StepConfig`` keyword arguments (checked: ValueError)"""
        kw = {k: getattr(self, k, d) for k, d in ANNEAL_DEFAULTS.items()}
        kw['anneal_yloss_offset'] = getattr(self, 'anneal_yloss_offset', 0)
        for sw, mx in (('anneal_kl', 'anneal_kl_itermax'), ('anneal_yloss', 'anneal_yloss_itermax'),
                       ('anneal_learning_rate', 'anneal_lr_itermax')):
            if kw[sw] and not int(kw[mx]) > 0:
                raise ValueError('%s is on: %s must be a positive number of iterations, not %r' % (sw, mx, kw[mx]))
        return dict((k, bool(v) if k in ('anneal_kl', 'anneal_yloss', 'anneal_learning_rate') else int(v)) for k, v in kw.items())

    def _counts_config(self):
        """the raw-count switches as they stand now, as ``StepConfig`` keyword arguments (checked: ValueError)"""
        return E.check_counts_config(getattr(self, 'x_transform', None), getattr(self, 'library_size', False), self.type_rec)

    def size_factor(self, x):
        """the observed size factor of every row of ``x``, (rows,): max(sum_g x_g, 1) / dim_x -- what ``library_size=True``
        multiplies the decoder means of a row by (``dv_rec_nll_rows``, the ``_LIB`` kinds)"""
        return torch.clamp(x.sum(dim=1), min=1.0) / float(self.dim_x)

    def _enc_x(self, x):
        """the encoder's view of the rows ``x``: T(x), T = log1p with ``x_transform='log1p'``, log1p(x / s) with
        ``'log1p_norm'`` -- s the rows' own observed size factors (``size_factor``), as the feed launch forms them"""
        tr = getattr(self, 'x_transform', None)
        if tr == 'log1p_norm':
            return torch.log1p(x / self.size_factor(x)[:, None])
        return torch.log1p(x) if tr == 'log1p' else x

    def _scaled(self, px, x, size_factor=None):
        """decoder output ``px`` with its mean multiplied by the size factor of the rows ``x`` (``library_size``; else as it is),
        or by ``size_factor`` where one is given (``_chosen_size``); theta and the dropout logit are never scaled"""
        if not getattr(self, 'library_size', False):
            return px
        sz = self.size_factor(x) if size_factor is None else size_factor
        return (px[0] * sz[:, None],) + tuple(px[1:])

    def _chosen_size(self, size_factor, x):
        """the ``size_factor=`` keyword of inference as a (rows,) tensor next to ``x`` (None stays None: the observed factors);
        ValueError on a model without ``library_size=True``, whose means carry no size factor at all"""
        if size_factor is None:
            return None
        if not getattr(self, 'library_size', False):
            raise ValueError('size_factor= scales the decoder means of a library_size=True model; this model has library_size=False')
        sz = torch.as_tensor(size_factor, dtype=torch.float32, device=x.device)
        if sz.dim() == 0:
            return sz.expand(x.shape[0])
        if tuple(sz.shape) != (x.shape[0],):
            raise ValueError('size_factor must be a number or a (rows,) tensor, not shape %r for %d rows' % (tuple(sz.shape), x.shape[0]))
        return sz

    def _step_config(self):
        top = 'dim_z3' if self.kind == 'drvae' else 'dim_z2'
        return E.StepConfig(
            kind=self.kind, dim_x=self.dim_x, dim_y=getattr(self, 'dim_y', 2), dim_z1=self.dim_z1,
            dim_z3=getattr(self, top, self.dim_z1), h_en_z1=list(self.dim_h_en_z1),
            h_de_z1=list(getattr(self, 'dim_h_de_z1', [])),
            h_en_z3=list(getattr(self, 'dim_h_en_z3' if self.kind == 'drvae' else 'dim_h_en_z2', [])),
            h_de_x=list(self.dim_h_de_x), h_clf=list(getattr(self, 'dim_h_clf', [])), nonlin=self.nonlinearity,
            weight_norm=self.wn, L=self.L, learning_rate=self.learning_rate, weight_decay=self.weight_decay,
            add_noise_var=self.add_noise_var, yloss_rate=getattr(self, 'yloss_rate', 1.),
            kl_qz2pz2_rate=getattr(self, 'kl_qz2pz2_rate', 1.), pertloss_rate=getattr(self, 'pertloss_rate', 0.),
            anneal_perturb_rate_itermax=getattr(self, 'anneal_perturb_rate_itermax', 0),
            anneal_perturb_rate_offset=getattr(self, 'anneal_perturb_rate_offset', 0),
            clf_z1z2=getattr(self, 'clf_z1z2', True), semi_supervised=getattr(self, 'semi_supervised', True),
            kl_min=self.kl_min, optim_alg=self.optim_alg, clf_1sig=bool(getattr(self, 'clf_1sig', False)),
            type_y=getattr(self, 'type_y', 'discrete'), type_rec=self.type_rec,
            use_s=bool(getattr(self, 'use_s', False)), dim_s=int(getattr(self, 'dim_s', 2)),
            use_MMD=bool(getattr(self, 'use_s', False) and getattr(self, 'use_MMD', False)),
            mmd_rate=float(getattr(self, 'mmd_rate', 1.)), kernel_MMD=getattr(self, 'kernel_MMD', 'rbf_fourier'),
            prior_y=None if (getattr(self, 'prior_y', None) is None or isinstance(getattr(self, 'prior_y', None), str))
            else tuple(float(v) for v in self.prior_y), matmul=self._matmul, dropout_rate=float(self.dropout_rate),
            max_grad_norm=self._max_grad_norm, ema_decay=self.ema_decay, **self._counts_config(), **self._anneal_config(),
            **(dict(dispersion=self.dispersion) if self.dispersion != 'gene-cell' else {}))

    # ---------------------------------------------------------------- inference
    @torch.no_grad()
    def forward(self, x1, s=[], size_factor=None):
        """Inference with the posterior MEANS (no sampling): src/DrVAE.py:253-311,
        src/PVAE.py:203-246, src/VFAE.py:178-215.

        Raw-count switches (EXTENSIONS): the encoder reads T(x1) (``x_transform``); with ``library_size`` the means
        ``px1[0]`` / ``x1_rec`` and ``px2[0]`` / ``x2_pert`` are multiplied by the size factor of ``x1`` -- the depth of the
        perturbed profile is unknown at prediction time, so the prediction is made at the depth of the profile it starts from.
        ``size_factor`` (a number or a (rows,) tensor; ``library_size`` models only, ValueError otherwise) scales those means by
        the given value INSTEAD: the decoder's output at a chosen depth -- ``size_factor=1.0`` is the denoised expression at a
        common depth of ``dim_x`` counts per cell.  None: the observed factors.  theta and the dropout logit are never scaled.

        ``type_rec='zinb'``: ``px1`` = (mu, theta, dropout logit); ``x1_rec`` / ``x2_pert`` are the negative-binomial MEAN (scaled
        under ``library_size``) -- the denoised expression, NOT the mixture's mean (1 - pi) mu."""
        self.eval()
        x1 = x1.to(next(self.parameters()).device, torch.float32)
        cond = self._s_inputs(s, x1)
        size = self._chosen_size(size_factor, x1)
        qz1 = self.encoder_z1([self._enc_x(x1)] + cond)
        z1 = qz1[0]
        res = OrderedDict(z1=z1, qz1=qz1)
        if self.kind in ('drvae', 'pvae'):
            pz2 = self.decoder_z2Fz1([z1])
            z2 = pz2[0]
            res.update(z2=z2, pz2=pz2)
        if self.kind in ('drvae', 'vfae'):
            if self.kind == 'drvae':
                clf_in = [z1, z2 - z1] if self.clf_z1z2 else [z2]
            else:
                clf_in = [z1]
            qy = self.encoder_y(clf_in)
            res.update(**self._pred_proba(qy))
        px1 = self._scaled(self.decoder_x([z1] + cond), x1, size)
        res.update(px1=px1, x1_rec=px1[0])
        if self.kind in ('drvae', 'pvae'):
            px2 = self._scaled(self.decoder_x([z2] + cond), x1, size)
            res.update(px2=px2, x2_pert=px2[0])
        return res

    def _s_inputs(self, s, like):
        """[one_hot(s)] when the model conditions on the nuisance variable (src/DrVAE.py:265-268), else []"""
        if not getattr(self, 'use_s', False):
            return []
        return [blk.one_hot(torch.as_tensor(s).to(like.device), self.dim_s)]

    @torch.no_grad()
    def forward_w_pert_identity(self, x1, x2, s=[], size_factor=None):
        """Inference assuming the perturbation function is the identity
        (src/DrVAE.py:185-251, src/PVAE.py:155-201).  ``library_size``: ``px2`` / ``x2_pert`` (predicted from x1) carry x1's
        size factor, ``px2_rec`` / ``x2_rec`` (reconstructed from x2) x2's own; ``size_factor`` (see ``forward``) replaces both."""
        if self.kind == 'vfae':
            raise AttributeError('VFAE has no perturbation path')
        self.eval()
        dev = next(self.parameters()).device
        x1, x2 = x1.to(dev, torch.float32), x2.to(dev, torch.float32)
        cond = self._s_inputs(s, x1)
        size = self._chosen_size(size_factor, x1)
        qz1 = self.encoder_z1([self._enc_x(x1)] + cond)
        z1 = qz1[0]
        res = OrderedDict(z1=z1, qz1=qz1)
        if self.kind == 'drvae':
            qy = self.encoder_y([z1, z1 - z1] if self.clf_z1z2 else [z1])
            res.update(**self._pred_proba(qy))
        px2 = self._scaled(self.decoder_x([z1] + cond), x1, size)
        qz2 = self.encoder_z1([self._enc_x(x2)] + cond)
        px2_rec = self._scaled(self.decoder_x([qz2[0]] + cond), x2, size)
        res.update(px2=px2, x2_pert=px2[0], z2=qz2[0], qz2=qz2, px2_rec=px2_rec, x2_rec=px2_rec[0])
        return res

    # ----------------------------------------------------------- posterior-predictive draws
    @torch.no_grad()
    def sample_x(self, x1, s=[], *, n_samples=1, latent='mean', size_factor=None, seed=None, event=0, row0=0):
        """EXTENSION (no reference counterpart): draws of x from the model, on the device (``drvae_amd.count_sample``; the
        sampler of include/drvae_hip.h) -- ``x1_samp`` (n_samples, rows, dim_x) float32 and, for DrVAE / PVAE, ``x2_samp`` from the
        perturbed latent z2 = F(z1), drawn at x1's size factor as ``x2_pert`` is.  Every ``type_rec``: mu + sd z, [u <= p],
        Poisson(s mu), Gamma-Poisson (theta per cell, per gene or per (gene, class)), and its zero-inflated form.

        ``latent='mean'``: the heads of ``forward()`` exactly -- one decoder pass, observation noise only.  ``'sample'``: the full
        posterior predictive -- per sample z1 ~ q(z1|x1) and z2 ~ p(z2|z1) from the row-keyed normals (draw ids 2k / 2k + 1 of
        sample k under ``seed ^ count_sample.LATENT_SEED_XOR``), one decoder pass per sample; the result then also carries
        ``z1_samp`` / ``z2_samp``.  ``size_factor``: as in ``forward`` (ValueError without ``library_size``).

        An element depends on (seed, event, sample index, GLOBAL row ``row0 + r``, gene) and the heads only, so rows sampled in
        pieces with their ``row0`` equal the rows sampled at once.  ``seed=None``: ``count_sample.default_seed(random_seed)``,
        which the train step's noise cannot share; a seed of your own must not be the train step's (see the header).  ``x2_samp``
        is drawn under ``seed ^ count_sample.X2_SEED_XOR``: it does not repeat x1_samp's random numbers."""
        from . import count_sample as CS
        S = CS.check_sample_args(self, n_samples, latent)
        self.eval()
        x1 = x1.to(next(self.parameters()).device, torch.float32)
        lat = OrderedDict()
        a, b = CS.sample_rows(self, x1, s, n_samples=S, latent=latent, size_factor=size_factor, seed=seed, event=event,
                              row0=int(row0), latents_out=lat)
        res = OrderedDict(x1_samp=a)
        if b is not None:
            res['x2_samp'] = b
        res.update(lat)
        return res

    def posterior_predictive(self, ds, n_samples=1, *, chunk_rows=None, out=None, latent='mean', seed=None, event=0):
        """EXTENSION: ``x1_samp`` of ``sample_x`` for every row of a DEVICE-resident ``DrVAEDataset`` / ``VFAEDataset`` (dense or
        ``CsrRows``), (n_samples, N, dim_x) float32, ``chunk_rows`` rows at a time (None: one chunk).  The global row of a draw is
        the row's position in the set: the result is bit for bit independent of ``chunk_rows`` and of dense versus sparse
        storage; a ``CsrRows`` matrix is gathered one chunk at a time.  ``out``: a float32 tensor of that shape to fill, on the
        device or pinned on the host (default: a new device tensor).  Touches no training state.  ValueError for a host-resident
        set, NotImplementedError under data parallelism."""
        from . import count_sample as CS
        return CS.posterior_predictive(self, ds, n_samples, chunk_rows=chunk_rows, out=out, latent=latent, seed=seed, event=event)

    def perturbation_effect(self, ds, *, n_samples=1, latent='mean', groups=None, n_groups=None, delta=0.25, pseudocount=0.0,
                            chunk_rows=None, seed=None, event=0):
        """EXTENSION (no reference counterpart): which genes the perturbation z2 = F(z1) moves, by how much and how surely, per
        group of cells of a DEVICE-resident ``DrVAEDataset`` (dense or ``CsrRows``) -- DrVAE / PVAE only.  The effect of one
        (sample, cell, gene) is e = log2(b + pseudocount) - log2(a + pseudocount) for the count decoders, a and b the UNSCALED
        mean heads decoded from z1 and z2 (x2_pert is predicted at x1's depth: the size factor cancels), and e = b - a for
        ``'diag_gaussian'`` (pseudocount must be 0).  An element whose e is not finite (a zero mean without a pseudocount)
        counts nowhere.

        ``latent='mean'``: the heads of ``forward()`` (n_samples must be 1).  ``'sample'``: per sample z1 ~ q(z1|x1), z2 ~
        p(z2|z1) -- the latents ``sample_x(latent='sample')`` returns for the same ``seed`` / ``event`` and global row = position
        in the set, so the statistics do not depend on ``chunk_rows`` beyond the order of float64 sums.  ``groups``: None, or an
        (N,) integer tensor with ``n_groups``; a negative entry leaves a cell out, an entry >= n_groups is a ValueError.

        Returns (n_groups, dim_x) float64 device tensors: ``n`` (valid elements), ``lfc_mean``, ``lfc_sd`` (population sd),
        ``p_up`` / ``p_down`` (the share of e > delta / e < -delta, strict), ``mean_base``, ``mean_pert``, and ``raw``, the
        (n_groups, 7, dim_x) sums they come from (``effect.STATS``).  A gene with n == 0 has NaN ratios.  Per chunk and sample:
        two decoder passes, one reduction launch (``drvae_amd.effect``), one fold; nothing of size rows x genes outlives a
        chunk, nothing is copied to the host, training state and the Philox counter are not touched.  ValueError for a
        host-resident set or ``type_rec='binary'``, NotImplementedError under data parallelism."""
        if self.kind == 'vfae':
            raise AttributeError('VFAE has no perturbation path')
        from . import effect
        return effect.perturbation_effect(self, ds, n_samples=n_samples, latent=latent, groups=groups, n_groups=n_groups,
                                          delta=delta, pseudocount=pseudocount, chunk_rows=chunk_rows, seed=seed, event=event)

    def _pred_proba(self, qy):
        """(pred, proba) of src/DrVAE.py:212-220: class + probabilities, or mean + log-variance"""
        if getattr(self, 'type_y', 'discrete') == 'cont':
            return dict(pred=qy[0], proba=qy[1])
        return dict(pred=self.encoder_y.most_probable(*qy), proba=qy[0])

    def predict(self, **kwargs):
        res = self.forward(**kwargs)
        return res['pred'].squeeze().cpu().numpy(), res['proba'].cpu().numpy()

    def reconstruct(self, **kwargs):
        res = self.forward(**kwargs)
        out = [res['x1_rec'].cpu().numpy(), [t.cpu().numpy() for t in res['px1']]]
        if 'px2' in res:
            out += [res['x2_pert'].cpu().numpy(), [t.cpu().numpy() for t in res['px2']]]
        return tuple(out)

    def transform(self, **kwargs):
        res = self.forward(**kwargs)
        if 'z2' in res:
            return res['z1'].cpu().numpy(), res['z2'].cpu().numpy()
        return res['z1'].cpu().numpy()

    # -------------------------------------------------------------- empty groups
    def _warn_empty_groups(self, has_x2, has_y):
        """the reference warns about empty data groups in the minibatch (src/DrVAE.py:588-608)"""
        hx = np.asarray(has_x2.cpu() if torch.is_tensor(has_x2) else has_x2).astype(bool).reshape(-1)
        hy = np.asarray(has_y.cpu() if torch.is_tensor(has_y) else has_y).astype(bool).reshape(-1)
        if self.kind == 'drvae':
            names = {'Labeled Singleton': hy & ~hx, 'Unlabeled Singleton': ~hy & ~hx,
                     'Labeled Paired perturbation': hy & hx, 'Unlabeled Paired perturbation': ~hy & hx}
        elif self.kind == 'pvae':
            names = {'Singleton': ~hx, 'Paired perturbation': hx}
        else:
            names = {'labeled': hy, 'unlabeled': ~hy}
        for n, m in names.items():
            if not m.any():
                warnings.warn('No %s data in the minibatch' % n)
