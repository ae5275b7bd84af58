"""Fused ELBO train step for DrVAE / PVAE / VFAE: hand-written forward AND backward
as one static sequence of HIP kernel launches over pre-allocated buffers (no autograd,
no allocation, no host sync) -> capturable in a hipGraph and replayed per step.

Restructuring relative to the reference (arithmetic identical):
  * the 4 data groups (ls/us/lp/up, src/DrVAE.py:585-608), the L Monte-Carlo samples
    (src/DrVAE.py:421) and the per-class passes for unlabeled rows (src/DrVAE.py:520-524)
    are stacked into the GEMM M dimension: every Linear layer runs ONCE per step;
  * group membership becomes row-index lists; the loss is linear in per-row terms with
    coefficients known before the forward pass (1/(L N), beta_pert ..., src/DrVAE.py:611-624),
    so the backward starts directly from per-row coefficients;
  * both heads of a block are one GEMM with a split epilogue; bias gradients ride on the
    dW GEMM; every scatter-add is a deterministic segment sum (no atomics).

Row layout (B rows, Np pairs, L samples):
  XIN  [B + Np]            noisy x1 rows, then noisy x2 rows of the pairs    (src/DrVAE.py:404-418)
  XT   [B + Np]            (raw-count inputs only) the RAW rows: the reconstruction targets, XIN then holds T(x) + noise
  Q    [B + Np, 2 Z1]      (mu | logvar) of q(z1|x1) and q(z2|x2)            (shared encoder, src/DrVAE.py:418)
  ZDEC [L B + 2 L Np, Z1]  z1 samples | z2 samples (from qz1: src/DrVAE.py:427) | z2Fz1 samples of pairs
  fprop rows               per (l, row): 1 row if labeled else Y rows        (src/DrVAE.py:503-526)
"""
import math
import os
from collections import OrderedDict
from dataclasses import dataclass, field
from typing import List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import gene_batch_rows as GB
from . import gene_rows as G
from . import kernels as K
from . import tuning as T
from ._lib import GAUSS_LOGVAR, GAUSS_SIGMA, REC_KIND, RECON_KIND, RECON_ZINB
from .arena import N_LOSS, ParamArena, span
from .chain import X3_PARTS, _Chain, _Lin, _pad4
from .plan import LOSS_IDX, _Plan
from .schedule import DUAL, EVAL, EVALUATE, FORK_JOIN, LOSS, TRAIN, StepSchedule, StepSync, _Branch, heads_route


# the precision ladder of the decoder-heads products: fp32, then the split-bf16 rungs by falling number of parts
MATMUL_CHOICES = ('fp32',) + tuple(X3_PARTS)
OPTIM_ALGS = ('adam', 'adamax', 'adamw')      # 'adamw': Adam with decoupled weight decay (dv_adam_hyper.decoupled)
assert MATMUL_CHOICES == ('fp32', 'bf16x3', 'bf16x2', 'bf16x1')


@dataclass
class StepConfig:
    """Shapes and hyper-parameters that reach the loss (ctor args of src/DrVAE.py:45-69,
    src/PVAE.py:46-62, src/VFAE.py:42-61 plus the attributes hard-coded in their __init__)."""
    kind: str = 'drvae'
    dim_x: int = 978
    dim_y: int = 2
    dim_z1: int = 100
    dim_z3: int = 100
    h_en_z1: List[int] = field(default_factory=lambda: [800])
    h_de_z1: List[int] = field(default_factory=lambda: [200])
    h_en_z3: List[int] = field(default_factory=lambda: [200])
    h_de_x: List[int] = field(default_factory=lambda: [600])
    h_clf: List[int] = field(default_factory=list)
    nonlin: str = 'elu'
    weight_norm: bool = False
    L: int = 2
    learning_rate: float = 5e-4
    weight_decay: float = 0.05
    add_noise_var: float = 0.01
    yloss_rate: float = 1.0
    kl_qz2pz2_rate: float = 1.0
    pertloss_rate: float = 0.05
    anneal_perturb_rate_itermax: int = 1
    anneal_perturb_rate_offset: int = 0
    clf_z1z2: bool = True
    semi_supervised: bool = True
    kl_min: float = 2.0
    optim_alg: str = 'adam'
    prior_y: Optional[Tuple[float, ...]] = None    # None = 'uniform' (src/DrVAE.py:386-389)
    clf_1sig: bool = False                          # two classes from one sigmoid output (src/DrVAE.py:160-163)
    type_y: str = 'discrete'                        # 'cont': regression head N(sigmoid(.), 0.05^2) (src/DrVAE.py:167-169)
    # EXTENSION (unreachable in the reference, which crashes at src/DrVAE.py:438): one_hot(s) appended
    # to the inputs of encoder_z1 and decoder_x (src/DrVAE.py:134-135,179-180), and with use_MMD the model-level MMD
    # penalty between the nuisance classes' latent samples (src/DrVAE.py:394-398,537-540,616,623-624)
    # type of p(x|z): 'diag_gaussian' (the only one the reference can build) | 'binary' | 'poisson' -- the Bernoulli /
    # Poisson decoders src/DrVAE.py:124-129 names and blocks.py never defines: one Linear head, log-likelihood rows
    # by dv_rec_nll_rows (EXTENSION) | 'nb': the negative binomial for overdispersed counts (EXTENSION, no counterpart in
    # the reference) -- two softplus heads [mu | theta] over one trunk, rows and both heads' gradients by the same launch |
    # 'zinb': the zero-inflated negative binomial (EXTENSION) -- a third head, the dropout logit (identity), behind those two
    type_rec: str = 'diag_gaussian'
    use_s: bool = False
    dim_s: int = 2
    use_MMD: bool = False
    mmd_rate: float = 1.0
    kernel_MMD: str = 'rbf_fourier'
    # OPT-IN arithmetic of the decoder-heads layer where it takes the raw-heads route (the chip-filling products of the wide
    # configuration): 'fp32' = fp32 MFMA like every other product (default) | 'bf16x3' = split-bf16 products, six bf16 MFMA
    # terms per fp32 product with fp32 accumulation (``dv_gemm_x3``) | 'bf16x2' = two bf16 parts per operand, three terms
    # (``dv_gemm_split``; ~2^-16 of sum |a||b|: below fp32, far above bf16) | 'bf16x1' = ONE part, one term: a bf16 product
    # of the rounded operands with fp32 accumulation (~2^-8: a different dtype, NOT held to the fp32 step's tolerances).
    # Decided once, where the plan is built
    matmul: str = 'fp32'
    # hidden-layer dropout (``dropout_rate`` of the models' constructors, src/blocks.py:139-151): every hidden activation of
    # every chain with at least two layers is a dropout SITE of a training pass (``_Chain.add_dropout``); the keep masks are
    # drawn with the step's noise (``kernels.fill_noise_rows``).  0: no sites, the step as it ever was
    dropout_rate: float = 0.0
    # EXTENSION (no counterpart in the reference): global-norm gradient clipping and a non-finite guard inside the step,
    # with the semantics of ``torch.nn.utils.clip_grad_norm_(params, max_grad_norm, norm_type=2)`` in front of the optimiser:
    # the (exchanged) gradient arena is scaled by coef = min(1, max_grad_norm / (norm + 1e-6)) on its way into the sweep, and a
    # step whose gradient holds an inf or a NaN is SKIPPED -- parameters, moments and the bias corrections' step count stay
    # as they are, a device counter counts it (``FusedStep.clip_stats``).  ``inf``: the guard alone.  None: nothing of this
    # exists -- no launch, no buffer, the step as it ever was
    max_grad_norm: Optional[float] = None
    # annealing schedules of the loss and of the learning rate (src/DrVAE.py:549-557,619-622; src/DGMMixin.py:100-104), off
    # by default like the reference's drivers leave them.  With ``it`` the number of finished training iterations:
    #   beta_kl  = anneal_coef(it, anneal_kl_itermax)                              multiplies KLD in ELBO
    #   beta_yr  = anneal_coef(it, anneal_yloss_itermax, anneal_yloss_offset)      multiplies yloss_rate * YL in CMPL
    #   lr_scale = max(0.01, 1 - anneal_coef(it, anneal_lr_itermax))               multiplies learning_rate (EXTENSION: the
    #              reference writes its new rate into a COPY of the optimiser's state, so its own switch does nothing;
    #              built here from the evident intent)
    # Any of them on: the step trains on the batch-independent plans only, and its schedule lives on the DEVICE -- a 16-byte
    # record {beta_pert, beta_kl, beta_yr, lr_scale} ``dv_batch_masks`` evaluates from the step counter at the head of every
    # step (``FusedStep.sched_rec``)
    anneal_kl: bool = False
    anneal_kl_itermax: int = 100
    anneal_yloss: bool = False
    anneal_yloss_itermax: int = 1
    anneal_yloss_offset: int = 0
    anneal_learning_rate: bool = False
    anneal_lr_itermax: int = 3000
    # EXTENSION (no counterpart in the reference): the exponential moving average of the parameters, kept by the optimiser
    # sweep itself -- e += (1 - ema_decay)(p_new - e) on every TAKEN step, one more stream of the sweep's launch
    # (``ParamArena.avg``, ``dv_adam_hyper.avg``).  None: nothing of this exists -- no buffer, no launch
    # argument, the step as it ever was.  ``optim_alg='adamw'`` is Adam with torch.optim.AdamW's decoupled weight decay
    ema_decay: Optional[float] = None
    # EXTENSIONS (no counterpart in the reference) for RAW COUNTS, count decoders ('poisson' / 'nb' / 'zinb') only; x >= 0:
    #   x_transform='log1p': the encoder reads log1p(x) + sigma * eps; the reconstruction target stays the raw row x, no noise
    #   x_transform='log1p_norm': the encoder reads log1p(x / s) + sigma * eps, s the size factor below of that same source
    #                        row (the x2 rows of pairs: x2's own), summed by the feed launch; targets as with 'log1p'
    #   library_size=True  : every decoder mean of a row is multiplied by the observed size factor of its target row,
    #                        s = max(sum_g x_g, 1) / dim_x -- mu = s * (softplus(a_m) + 1e-6); theta and the dropout logit are untouched
    # Either on: SPLIT MODE -- the plan holds the raw target rows in a buffer of their own (``_Plan.XT``), the input launch is
    # ``dv_batch_feed`` in its split form on every path.  Both off: nothing of this exists, the step as it ever was
    x_transform: Optional[str] = None
    library_size: bool = False
    # EXTENSION (no counterpart in the reference), 'nb' / 'zinb' only: where the inverse dispersion theta comes from.
    #   'gene-cell' (default): a decoder head of its own, one theta per (cell, gene) -- the step as it ever was
    #   'gene'               : ONE theta per gene, shared by all cells -- the (dim_x,) parameter ``GENE_THETA`` in the arena,
    #                          theta_g = softplus(raw_theta_g) + 1e-3; the theta head and its three products do not exist, the
    #                          row pass reads the vector (``gene_rows``) and its gradient is a column sum
    #   'gene-batch'         : (``use_s`` only) one theta per (gene, nuisance class) -- the same parameter as a (dim_s, dim_x) table;
    #                          a decoder row reads the row of its class (``gene_batch_rows``: the class is a grid dimension of the
    #                          row pass), the x2 and perturbation rows of a pair the class of their batch row
    dispersion: str = 'gene-cell'

    def __post_init__(self):
        check_counts_config(self.x_transform, self.library_size, self.type_rec, 'StepConfig.')
        check_dispersion(self.dispersion, self.type_rec, 'StepConfig.', use_s=self.use_s)
        self.library_size = bool(self.library_size)
        if self.optim_alg not in OPTIM_ALGS:
            raise ValueError('StepConfig.optim_alg must be one of %s, not %r' % (OPTIM_ALGS, self.optim_alg))
        self.ema_decay = check_ema_decay(self.ema_decay, 'StepConfig.ema_decay')
        for sw, mx in (('anneal_kl', 'anneal_kl_itermax'), ('anneal_yloss', 'anneal_yloss_itermax'),
                       ('anneal_learning_rate', 'anneal_lr_itermax')):
            setattr(self, sw, bool(getattr(self, sw)))
            if getattr(self, sw) and not int(getattr(self, mx)) > 0:
                raise ValueError('StepConfig.%s is on: %s must be a positive number of iterations, not %r'
                                 % (sw, mx, getattr(self, mx)))
        if self.matmul not in MATMUL_CHOICES:
            raise ValueError('StepConfig.matmul must be one of %s, not %r' % (MATMUL_CHOICES, self.matmul))
        if not 0.0 <= self.dropout_rate < 1.0:
            raise ValueError('StepConfig.dropout_rate must lie in [0, 1), not %r' % (self.dropout_rate,))
        if self.max_grad_norm is not None:
            self.max_grad_norm = float(self.max_grad_norm)
            if not self.max_grad_norm > 0.0:          # (NaN fails this too)
                raise ValueError('StepConfig.max_grad_norm must be a positive number, inf or None, not %r'
                                 % (self.max_grad_norm,))

    @property
    def annealed(self):
        """is any schedule beyond the perturbation coefficient on?  (That one alone changes once, on the step from iteration 0
        to 1 with the drivers' settings, and stays a host write: ``_Plan.set_beta``)"""
        return bool(self.anneal_kl or (self.anneal_yloss and self.has_y) or self.anneal_learning_rate)

    @property
    def rec(self):
        """the reconstruction family of ``type_rec`` (``REC_FAMILIES``; ``dispersion='gene'``: ``GENE_FAMILIES``)"""
        return rec_family(self.type_rec, self.dispersion)

    @property
    def split_x(self):
        """are the encoder's rows and the reconstruction targets two buffers?  (raw-count inputs)"""
        return bool(self.x_transform is not None or self.library_size)

    @property
    def cont(self):
        return self.type_y == 'cont'

    @property
    def top_name(self):
        return 'encoder_z2' if self.kind == 'vfae' else 'encoder_z3'

    @property
    def has_pert(self):
        return self.kind in ('drvae', 'pvae')

    @property
    def has_y(self):
        return self.kind in ('drvae', 'vfae')


X_TRANSFORMS = (None, 'log1p', 'log1p_norm')
NB_THETA_SHIFT = 1e-3       # the inverse-dispersion head's shift: the sigma head's (``DV_NB_THETA_SHIFT``)


class RecHead(NamedTuple):
    prefix: str             # state_dict prefix of the head's Linear
    act: str                # its activation and the shift behind it
    shift: float


class RecFamily(NamedTuple):
    """what a ``type_rec`` is, in one place.  'binary' / 'poisson': the Bernoulli / Poisson decoders src/DrVAE.py:124-129 names
    (EXTENSION); 'nb' / 'zinb': the negative binomial and its zero-inflated form (EXTENSIONS, no counterpart in
    the reference; ``blocks.NegativeBinomialDecoder`` / ``ZeroInflatedNegativeBinomialDecoder``)"""
    heads: Tuple[RecHead, ...]          # over one trunk, in arena order: the head columns of ``_Plan.DPX`` and of the row launch;
    #                                     heads[0].shift is the ``shift`` argument of ``dv_rec_nll_rows``
    counts: bool                        # a count decoder: takes ``x_transform`` / ``library_size``
    rows_kind: Optional[int]            # kind of ``dv_rec_nll_rows`` (None: the Gaussian rows have entry points of their own)
    rows_kind_lib: Optional[int]        # its library-scaled kind (None: the family has none)
    recon_kind: int                     # kind of ``dv_recon_rows``: every family has one (``RECON_KIND``; 'zinb': ``RECON_ZINB``)
    eval_ll: bool                       # does that evaluation report a log-likelihood?
    gene: bool = False                  # theta is the gene-wise vector ``GENE_THETA``, not a head (``GENE_FAMILIES``)


# the negative binomial's two heads, mean then inverse dispersion: both softplus + their own shift
_NB_HEADS = (RecHead('decoder_x.decoder_m.linear_m', 'softplus', 1e-6),
             RecHead('decoder_x.decoder_t.linear_t', 'softplus', NB_THETA_SHIFT))
REC_FAMILIES = {
    'diag_gaussian': RecFamily((RecHead('decoder_x.encoder_mu.linear_mu', 'identity', 0.0),
                                RecHead('decoder_x.encoder_sg.linear_sg', 'softplus', 1e-3)),
                               False, None, None, RECON_KIND[None], True),
    'binary': RecFamily((RecHead('decoder_x.decoder_p.linear_p', 'sigmoid', 0.0),), False, REC_KIND['binary'], None,
                        RECON_KIND['binary'], False),
    'poisson': RecFamily((RecHead('decoder_x.decoder_r.linear_r', 'softplus', 1e-6),), True, REC_KIND['poisson'],
                         REC_KIND['poisson_lib'], RECON_KIND['poisson'], False),
    'nb': RecFamily(_NB_HEADS, True, REC_KIND['nb'], REC_KIND['nb_lib'], RECON_KIND['nb'], True),
    # the dropout logit (identity) behind those two, back to back in the arena -- ``_Lin(third=...)``
    'zinb': RecFamily(_NB_HEADS + (RecHead('decoder_x.decoder_d.linear_d', 'identity', 0.0),), True,
                      REC_KIND['zinb'], REC_KIND['zinb_lib'], RECON_ZINB, True),
}


# ``dispersion='gene'``: the families without the theta head -- 'nb' the mean head alone (launched as the Poisson decoder's single
# softplus head is), 'zinb' the pair [mean | dropout logit], back to back in the arena; theta is the (dim_x,) parameter below
# ``dispersion='gene-batch'`` (``use_s`` models only): the same families -- the parameter is a (dim_s, dim_x) table at the same
# place, a row per nuisance class, and the row pass reads the row of a decoder row's class (``gene_batch_rows``)
DISPERSIONS = ('gene-cell', 'gene', 'gene-batch')
GENE_THETA = 'decoder_x.decoder_t.raw_theta'
GENE_FAMILIES = {
    'nb': RecFamily(_NB_HEADS[:1], True, REC_KIND['nb'], REC_KIND['nb_lib'], RECON_KIND['nb'], True, True),
    'zinb': RecFamily((_NB_HEADS[0], REC_FAMILIES['zinb'].heads[2]), True, REC_KIND['zinb'], REC_KIND['zinb_lib'], RECON_ZINB,
                      True, True),
}


def rec_family(type_rec, dispersion='gene-cell'):
    """the ``RecFamily`` of a decoder: ``REC_FAMILIES[type_rec]``, or its gene-wise form"""
    return GENE_FAMILIES[type_rec] if dispersion in ('gene', 'gene-batch') else REC_FAMILIES[type_rec]


def check_dispersion(dispersion, type_rec, prefix='', use_s=False):
    """``dispersion`` as a checked value; ValueError for an unknown one, for 'gene' / 'gene-batch' on a decoder without a theta
    and for 'gene-batch' on a model without nuisance classes (``use_s``)"""
    if dispersion not in DISPERSIONS:
        raise ValueError("%sdispersion must be 'gene-cell' or 'gene' (or 'gene-batch' with use_s=True), not %r"
                         % (prefix, dispersion))
    if dispersion != 'gene-cell' and type_rec not in GENE_FAMILIES:
        raise ValueError("%sdispersion=%r is for the decoders with an inverse dispersion (type_rec=%s), not type_rec=%r"
                         % (prefix, dispersion, ' / '.join(repr(k) for k in GENE_FAMILIES), type_rec))
    if dispersion == 'gene-batch' and not use_s:
        raise ValueError("%sdispersion='gene-batch' is a dispersion per (gene, nuisance class): it needs use_s=True" % prefix)
    return dispersion


def check_counts_config(x_transform, library_size, type_rec, prefix=''):
    """the raw-count switches as ``StepConfig`` keyword arguments; ValueError for an unknown ``x_transform`` and for either
    switch on a decoder that is no count decoder"""
    if x_transform not in X_TRANSFORMS:
        raise ValueError("%sx_transform must be None, 'log1p' or 'log1p_norm', not %r" % (prefix, x_transform))
    on = [n for n, v in (('x_transform', x_transform is not None), ('library_size', bool(library_size))) if v]
    if on and not (type_rec in REC_FAMILIES and REC_FAMILIES[type_rec].counts):
        raise ValueError("%s%s is for the count decoders (type_rec=%s), not type_rec=%r"
                         % (prefix, ' / '.join(on), ' / '.join(repr(k) for k, f in REC_FAMILIES.items() if f.counts), type_rec))
    return dict(x_transform=x_transform, library_size=bool(library_size))


def check_ema_decay(d, what='ema_decay'):
    """None or a float in (0, 1); ValueError otherwise"""
    if d is None:
        return None
    d = float(d)
    if not 0.0 < d < 1.0:               # (NaN fails this too)
        raise ValueError('%s must be None or a number in (0, 1), not %r' % (what, d))
    return d


def anneal_coef(iter_num, iter_max=1000, iter_offset=0):
    """src/DGMMixin.py:77-89."""
    if iter_num - iter_offset > 0:
        return min(1., 0.01 + (iter_num - iter_offset) / (1. * iter_max))
    return 0.01


def param_shapes(cfg):
    """state_dict name -> shape in the reference's construction order (src/DrVAE.py:112-183,
    src/PVAE.py:106-153, src/VFAE.py:103-165)."""
    out = OrderedDict()

    def lin(prefix, n_in, n_out):
        out[prefix + '.weight'] = (n_out, n_in)
        out[prefix + '.bias'] = (n_out,)
        if cfg.weight_norm:
            out[prefix + '.g'] = (n_out,)

    def trunk(prefix, n_in, hidden):
        for i, h in enumerate(hidden, start=1):
            lin('%s.model.linear%d' % (prefix, i), n_in, h)
            n_in = h
        return n_in

    def gauss(prefix, n_in, hidden, n_out, second='lv'):
        n = trunk(prefix + '.nnet', n_in, hidden)
        lin(prefix + '.encoder_mu.linear_mu', n, n_out)
        lin('%s.encoder_%s.linear_%s' % (prefix, second, second), n, n_out)

    X, Y, Z1, Z3 = cfg.dim_x, cfg.dim_y, cfg.dim_z1, cfg.dim_z3
    S = cfg.dim_s if cfg.use_s else 0
    gauss('encoder_z1', X + S, cfg.h_en_z1, Z1)
    if cfg.has_pert:
        out['decoder_z2Fz1.W_mu'] = (Z1, Z1)
        out['decoder_z2Fz1.bias_mu'] = (Z1,)
        out['decoder_z2Fz1.encoder_lv.linear_lv.weight'] = (Z1, Z1)
        out['decoder_z2Fz1.encoder_lv.linear_lv.bias'] = (Z1,)
    if cfg.has_y:
        n_in = 2 * Z1 if (cfg.kind == 'drvae' and cfg.clf_z1z2) else Z1
        if cfg.cont:
            gauss('encoder_y', n_in, cfg.h_clf, Y)
        else:
            n = trunk('encoder_y.nnet', n_in, cfg.h_clf)
            lin('encoder_y.decoder_p.linear_p', n, 1 if cfg.clf_1sig else Y)
        gauss(cfg.top_name, Z1 + Y, cfg.h_en_z3, Z3)
        gauss('decoder_z1', Z3 + Y, cfg.h_de_z1, Z1)
    n = trunk('decoder_x.nnet', Z1 + S, cfg.h_de_x)
    if cfg.rec.gene:
        # in FRONT of the heads: they stay the tail of the arena (the half of the sweep the side chain may take,
        # ``_side_adam_layout``), and the vector lies in the half that follows the whole backward pass
        out[GENE_THETA] = (cfg.dim_s, X) if cfg.dispersion == 'gene-batch' else (X,)
    for h in cfg.rec.heads:
        lin(h.prefix, n, X)
    return out


Y_LOGVAR_CONT = math.log(0.05 ** 2)      # fixed variance of the regression head (src/DrVAE.py:168)


def frozen_params(cfg):
    """parameters that exist in the state_dict but never receive a gradient (torch's Adam then skips
    them entirely -- no weight decay either): the log-variance head of the fixed-variance regression
    classifier (src/blocks.py:297-298)"""
    if cfg.has_y and cfg.cont:
        q = 'encoder_y.encoder_lv.linear_lv'
        return tuple([q + '.weight', q + '.bias'] + ([q + '.g'] if cfg.weight_norm else []))
    return ()


class FusedStep(StepSchedule):
    """Owns the arena views, the per-batch plan (index lists + buffers) and the launch
    sequence.  Typical use::

        eng = FusedStep(cfg, arena)
        eng.set_batch(x1, x2, y, has_x2, has_y)      # device tensors + host flags
        eng.set_noise(noise) | eng.draw_noise()
        eng.forward(); eng.backward(); eng.optimizer_step()
    """

    def __init__(self, cfg, arena, seed=12345, concurrent=True, row0=0):
        self.cfg, self.arena = cfg, arena
        # data parallelism: position of this rank's first row in the GLOBAL minibatch (the Philox draws are keyed
        # by global row); every rank uses the same ``seed``
        self.row0 = int(row0)
        self.dev = arena.device
        self.iters = 0                      # finished_training_iters (src/DGMMixin.py:124)
        # one batch-independent plan (and one captured graph) for ANY composition of pairs / labels in the batch:
        # group membership becomes device-side masks (see ``_Plan.universal``); costs the rows of the worst case
        self.universal = False
        self.universal_pair_slots = None      # (set_batch on the universal plan) only the first so many rows may be pairs
        self.universal_labeled_range = None   # ... and rows [a, b) are labeled for sure (one fprop row each)
        # ``use_s`` models: explicit batches (``set_batch``) go to plans that carry the nuisance classes on the device
        # (``_Plan.carry_nuisance``; ``s`` may then be a device tensor, no host round trip, and the MMD penalty runs as its
        # two grouped launches) -- the plans ``DeviceBatcher(carry_s=True)`` binds.  'masked' (set by
        # ``DeviceBatcher(mode='sampler', carry_s='masked').bind``): the same on the universal plan when ``universal`` is on
        # -- the penalty's data groups are device data too.  Default: the host-list plans
        self.carry_s = False
        self.plan = None
        self._plans = {}                    # plans by batch structure (a handful of signatures in practice)
        self.max_plans = 8
        self.pinned_plans = set()     # keys the cache never drops (a feed's bucket plans: DeviceBatcher)
        self.step_dev = torch.zeros(1, dtype=torch.int32, device=self.dev)       # Adam step (device side)
        self.loss_sum = torch.zeros(8, device=self.dev)      # running sums of the loss scalars over train steps
        self.rng_ctr = torch.zeros(2, dtype=torch.int32, device=self.dev)        # Philox counter (device side)
        # gradient-norm clipping (``StepConfig.max_grad_norm``): the engine's clip state (``kernels.clip_state``), device memory
        # for its life -- the step counter becomes its first word, the record {norm, coef, skip, n_skipped} and the workspace
        # of the norm pass are views of it; None: the feature does not exist
        self.clip_state = self.clip_rec = self.clip_part = None
        if cfg.max_grad_norm is not None:
            self.clip_state = K.clip_state(self.dev, arena.n_live, cfg.max_grad_norm)
            self.step_dev = self.clip_state[0:1]
            self.clip_rec, self.clip_part = K.clip_record(self.clip_state), K.clip_partials(self.clip_state)
        # annealing schedules (``StepConfig.annealed``): the step's record {beta_pert, beta_kl, beta_yr, lr_scale}, 16 bytes of
        # device memory for the engine's life, rewritten at the head of every step by the launch that writes the batch's
        # masks; the sweeps read its last word.  None: no schedule, nothing of this exists
        self.sched_rec = torch.ones(4, device=self.dev) if cfg.annealed else None
        # the parameter average (``StepConfig.ema_decay``): a sibling of the parameter arena, started as a copy of it, moved by
        # every sweep of the step.  ``averaged``: the parameter arena HOLDS the averaged values (``averaged_parameters``: the
        # contents are swapped, never the pointers -- captured graphs have the arena's addresses baked in); no train step then
        if cfg.ema_decay is not None:
            arena.ensure_avg()
        self.averaged = False
        self.seed = seed
        self.training = True
        self.fuse_bwd = False               # set by train_step/capture: forward is followed by backward
        # train-step scheduling of the classifier/fprop side chain (tuning 'sched'): 3 = one graph fork/join per step,
        # 5 (default) = two single-stream graphs (main chain / side chain) launched on two streams per step and ordered
        # ONLY by device flags (dv_flag_publish / dv_flag_wait): no graph edges, no events.  (Also tried and dropped: a
        # fork/join per pass; an extra cross edge, 0.37 ms; the side chain as a second ROOT of one graph with flags,
        # 0.42 ms -- the executor starts it late.)
        self.sched = T.get('sched')
        # the row work that consumes both heads of a block (the reparameterised samples; forward AND backward of
        # the reconstruction log-likelihood) leaves the heads' own GEMM launch (dv_gemm_heads): where, ``heads_route`` says
        self.fuse_heads = bool(T.get('fuse_heads'))
        self._init_schedule_state()
        self.side_ctr = torch.zeros(1, dtype=torch.int32, device=self.dev)   # the side chain's own step count
        self.side_t = torch.ones(1, dtype=torch.int32, device=self.dev)      # ... + 1: the optimiser step it works on
        self.sync = StepSync(self.dev)      # the flags / (error, ticks parked) words of the chains' hand-shake, by name
        self.flags, self.sync_err = self.sync.flags, self.sync.err
        self.add_noise = True               # `fit(add_noise=...)` flag of the reference (src/DrVAE.py:769)
        # classifier/fprop chain || decoder chain.  PVAE's side chain is one tiny KL kernel: a second stream
        # costs it far more than it hides (measured 0.19 ms single-stream vs 0.9 ms forked), so it runs serial
        # (models without a classifier have no second chain: a graph branch for the step's leaf work alone -- two KL row
        # launches, the loss scalars -- was measured: the main chain shrinks by 18 us, the fork/join costs as much;
        # PVAE cfg 1: 0.1742 -> 0.1763 ms)
        # (PVAE: its side chain would be the two KL row launches; as a graph branch next to the decoder they cost more
        # than they hide: cfg 1 0.167 -> 0.175 ms)
        self.branch = _Branch(self.dev, enabled=concurrent and cfg.has_y)
        self.concurrent = bool(concurrent)
        self._build_layers()

    # ------------------------------------------------------------------ layer table
    def _gauss(self, prefix, n_hidden, second, act_second='identity', shift_second=0.0):
        cfg, a = self.cfg, self.arena
        wn = cfg.weight_norm
        layers = []
        for i in range(1, n_hidden + 1):
            p = '%s.nnet.model.linear%d' % (prefix, i)
            layers.append(_Lin(a, p + '.weight', p + '.bias', p + '.g' if wn else None, act=cfg.nonlin))
        m = prefix + '.encoder_mu.linear_mu'
        s = '%s.encoder_%s.linear_%s' % (prefix, second, second)
        layers.append(_Lin(a, m + '.weight', m + '.bias', m + '.g' if wn else None,
                           second=(s + '.weight', s + '.bias', s + '.g' if wn else None),
                           act='identity', act1=act_second, shift1=shift_second))
        return layers

    def _build_layers(self):
        cfg, a = self.cfg, self.arena
        wn = cfg.weight_norm
        self.L_enc = self._gauss('encoder_z1', len(cfg.h_en_z1), 'lv', shift_second=-2.0)
        # the data decoder: trunk + the family's heads as ONE layer (one, a pair, or a pair with a third -- identity -- behind it)
        names = lambda q: (q + '.weight', q + '.bias', q + '.g' if wn else None)
        heads = cfg.rec.heads
        kw = dict(act=heads[0].act, shift0=heads[0].shift)
        if len(heads) > 1:
            kw.update(second=names(heads[1].prefix), act1=heads[1].act, shift1=heads[1].shift)
        if len(heads) > 2:
            assert heads[2].act == 'identity'
            kw.update(third=names(heads[2].prefix))
        self.L_decx = [_Lin(a, *names('decoder_x.nnet.model.linear%d' % i), act=cfg.nonlin)
                       for i in range(1, len(cfg.h_de_x) + 1)] + [_Lin(a, *names(heads[0].prefix), **kw)]
        if cfg.has_pert:
            p = 'decoder_z2Fz1.'
            self.L_z2F = [_Lin(a, p + 'W_mu', p + 'bias_mu', None,
                               second=(p + 'encoder_lv.linear_lv.weight', p + 'encoder_lv.linear_lv.bias', None),
                               act='identity', shift1=-2.0)]
        if cfg.has_y:
            layers = []
            for i in range(1, len(cfg.h_clf) + 1):
                q = 'encoder_y.nnet.model.linear%d' % i
                layers.append(_Lin(a, q + '.weight', q + '.bias', q + '.g' if wn else None, act=cfg.nonlin))
            q = 'encoder_y.encoder_mu.linear_mu' if cfg.cont else 'encoder_y.decoder_p.linear_p'
            layers.append(_Lin(a, q + '.weight', q + '.bias', q + '.g' if wn else None,
                               act='sigmoid' if cfg.cont else 'identity'))
            self.L_clf = layers
            # single Linear with <= 8 classes: dedicated wave-per-row kernels instead of MFMA tiles
            self.clf_small = (not cfg.h_clf) and cfg.dim_y <= 8 and not wn and not cfg.clf_1sig and not cfg.cont
            self.L_top = self._gauss(cfg.top_name, len(cfg.h_en_z3), 'lv', shift_second=-2.0)
            self.L_dz1 = self._gauss('decoder_z1', len(cfg.h_de_z1), 'lv', shift_second=-2.0)

    # ------------------------------------------------------------------------- plan
    def universal_ok(self):
        cfg = self.cfg
        # (``use_s``: only with the nuisance classes AND the penalty's data groups carried as device data --
        # ``DeviceBatcher(mode='sampler', carry_s='masked')``; otherwise such models run on structure plans)
        return not cfg.cont and not (cfg.kind == 'vfae' and not cfg.semi_supervised) and \
            (not cfg.use_s or self.carry_s == 'masked')

    def set_structure_universal(self, n_rows, n_pair_slots=None, labeled_range=None, n_tot=None, carry_s=False):
        """Select (or build) the batch-independent plan for ``n_rows`` rows.  ``n_pair_slots`` < n_rows: only the FIRST
        so many rows of a batch have pair slots (x2 row, z2 / z2Fz1 sample rows) -- for feeds that put a batch's pairs
        first and choose the plan by the batch's number of pairs (``DeviceBatcher(mode='sampler', pair_bucket=...)``):
        the decoder then runs L*B + 2*L*n_pair_slots rows instead of 3*L*B.  ``labeled_range`` = (a, b): the feed
        guarantees that rows [a, b) of every batch are labeled -- they get ONE fprop row (their class, as in a plan
        built for the batch's structure) instead of a row per class.  ``n_tot`` (data parallelism): the
        rows are one rank's slice of a GLOBAL batch of ``n_tot`` rows; N_pairs / N_labeled of every batch then are the
        global counts, handed over as data (``set_batch(counts=...)``, the feed's ``gcounts`` table) instead of being
        counted over this slice by dv_batch_masks.  ``carry_s`` (required for ``use_s`` models, ignored for others): the
        plan carries the nuisance classes on the device (``_Plan.carry_nuisance``); with ``use_MMD`` the penalty reads classes
        AND data groups inside its two launches (``dv_mmd_masked_*``)."""
        cfg = self.cfg
        carry = bool(cfg.use_s and carry_s)
        assert not cfg.cont and not (cfg.kind == 'vfae' and not cfg.semi_supervised), \
            'universal plan: discrete labels, semi-supervised models'
        assert carry or not cfg.use_s, 'universal plan of a use_s model: the nuisance classes are carried on the device (carry_s)'
        nps = n_rows if (n_pair_slots is None or not cfg.has_pert) else int(n_pair_slots)
        assert 0 <= nps <= n_rows
        lab = (0, 0) if (labeled_range is None or not cfg.has_y) else (int(labeled_range[0]), int(labeled_range[1]))
        if lab[1] <= lab[0]:
            lab = (0, 0)
        assert 0 <= lab[0] <= lab[1] <= n_rows
        key = ('universal', n_rows, self.row0)
        if nps != n_rows or lab != (0, 0):
            key = key + (nps,) + (lab if lab != (0, 0) else ())
        if n_tot is not None:
            key = key + (('n_tot', int(n_tot)),)
        if carry:
            key = key + ('carry_s',)
        # nothing narrows the plan: every row may be a pair, labeled or not, counted over this slice
        plain = nps == n_rows and lab == (0, 0) and n_tot is None and not carry
        key = key + self._rate_key()
        if self.plan is None or self.plan.key != key:
            self.plan = self._plans.get(key)
            if self.plan is None:
                ar = np.arange(n_rows)
                ones, zeros = ar < nps, np.zeros(n_rows, bool)
                self.plan = self._plans[key] = _Plan(self, ar, ones if cfg.has_pert else zeros,
                                                      (ar >= lab[0]) & (ar < lab[1]),
                                                      None if n_tot is None else (int(n_tot), 0, 0), key, universal=True)
                self.plan.every_row_anything = plain
                if cfg.has_y:
                    self.plan.set_labels_host(np.zeros(n_rows, np.int64))      # class slots: static
                if carry:
                    self.plan.carry_nuisance()
                self._evict_plans(key)
        return self.plan

    def _rate_key(self):
        """what a plan key carries of the dropout rate: nothing at rate 0 (the keys of such plans stay what they were)"""
        r = self.cfg.dropout_rate
        return (('dropout', float(r)),) if r > 0 else ()

    def _evict_plans(self, keep):
        """keep the plan cache bounded (randomly composed minibatches rarely repeat a structure; whole-set
        evaluations come in a few sizes), never dropping the plan a captured graph points into"""
        for old in list(self._plans):
            if len(self._plans) <= self.max_plans:
                break
            if old != keep and old != self._graph_key and old not in self._captures and old not in self.pinned_plans:
                del self._plans[old]

    def set_structure(self, has_x2, has_y, counts=None, carry_s=None):
        """Select (or build) the plan for a batch STRUCTURE: which rows are pairs / labeled.
        Returns (plan, rows) where ``rows`` are the participating row positions.  ``carry_s`` (``use_s`` models; default:
        ``self.carry_s``): the plan that carries the nuisance classes on the device -- a plan of its own."""
        cfg = self.cfg
        carry = bool(cfg.use_s and (self.carry_s if carry_s is None else carry_s))
        has_x2 = np.asarray(has_x2.cpu() if torch.is_tensor(has_x2) else has_x2).astype(bool).reshape(-1)
        has_y = np.asarray(has_y.cpu() if torch.is_tensor(has_y) else has_y).astype(bool).reshape(-1)
        if not cfg.has_pert:
            has_x2 = np.zeros_like(has_x2)
        if not cfg.has_y:
            has_y = np.zeros_like(has_y)
        rows = np.arange(len(has_y))
        if cfg.kind == 'vfae' and not cfg.semi_supervised:
            rows = rows[has_y]               # supervised-only model ignores unlabeled rows (src/VFAE.py:445-450)
        # the plan (index lists, buffers, captured graph) depends on the group STRUCTURE only; the
        # class labels of the labeled rows are data and are refreshed in place
        key = (len(rows), has_x2[rows].tobytes(), has_y[rows].tobytes(), counts, self.row0)
        if carry:
            key = key + ('carry_s',)
        key = key + self._rate_key()
        if self.plan is None or self.plan.key != key:
            self.plan = self._plans.get(key)
            if self.plan is None:
                self.plan = self._plans[key] = _Plan(self, rows, has_x2[rows], has_y[rows], counts, key)
                if carry:
                    self.plan.carry_nuisance()
                self._evict_plans(key)
        return self.plan, rows

    def set_batch(self, x1, x2, y, has_x2, has_y, counts=None, s=None):
        """x1,x2: (B,X) device fp32; y: (B,) or (B,1) ints (host or device); has_*: host bool/int
        arrays.  ``counts`` = (N_total, N_pairs, N_labeled) GLOBAL normalisers under data
        parallelism; default: this batch's own counts (src/DrVAE.py:611-616).
        ``s``: nuisance classes of the rows (``use_s`` extension)."""
        cfg = self.cfg
        if cfg.use_s:
            assert s is not None, 'use_s: the nuisance classes of the batch are needed'
            p = self._set_batch(x1, x2, y, has_x2, has_y, counts)
            if p.carry_s:       # device to device: the same launch the epoch feed runs, on the batch's own classes
                sd = (s if torch.is_tensor(s) else torch.as_tensor(np.asarray(s))).reshape(-1).to(self.dev)
                if len(p.rows) != sd.numel():
                    sd = sd.index_select(0, torch.as_tensor(p.rows, device=self.dev))
                p.set_s_device(sd)
                return p
            sv = np.asarray(s.cpu() if torch.is_tensor(s) else s).astype(np.int64).reshape(-1)
            p.set_s_host(sv[p.rows])
            return p
        return self._set_batch(x1, x2, y, has_x2, has_y, counts)

    def _require_universal(self, what):
        """an annealed step trains on the batch-independent plans only (their per-row coefficients are rewritten on the device
        at every step: that launch carries the schedule); a configuration that has none is refused, loudly"""
        if self.cfg.annealed and not self.universal_ok():
            cfg = self.cfg
            why = "type_y='cont'" if cfg.cont else 'the supervised-only VFAE' if (cfg.kind == 'vfae' and not cfg.semi_supervised) \
                else "use_s without DeviceBatcher(mode='sampler', carry_s='masked')"
            raise NotImplementedError('%s: annealing schedules (anneal_kl / anneal_yloss / anneal_learning_rate) run on the '
                                      'batch-independent plan, which %s does not have' % (what, why))

    def _set_batch(self, x1, x2, y, has_x2, has_y, counts=None):
        cfg = self.cfg
        self._require_universal('set_batch')
        if (self.universal or cfg.annealed) and self.universal_ok():
            hy = np.asarray(has_y.cpu() if torch.is_tensor(has_y) else has_y).reshape(-1)
            p = self.set_structure_universal(len(hy), self.universal_pair_slots, self.universal_labeled_range,
                                             n_tot=None if counts is None else counts[0], carry_s=cfg.use_s)
            p.feed_active = False
            if counts is not None:       # this rank's slice of a global batch: the GLOBAL (N_pairs, N_labeled) are data
                p.gcounts_dev.copy_(torch.tensor([int(counts[1]), int(counts[2])], dtype=torch.int32))
            p.XSRC[:p.B].copy_(x1)
            i32 = lambda a: torch.as_tensor(np.asarray(a.cpu() if torch.is_tensor(a) else a).reshape(-1).astype(np.int32))
            if cfg.has_pert:
                if x2 is None:      # no second profiles at all (e.g. a whole-set evaluation of singletons)
                    assert has_x2 is None or not np.asarray(has_x2.cpu() if torch.is_tensor(has_x2) else has_x2).any(), \
                        'has_x2 marks pairs but x2 is None'
                    p.XSRC[p.B:].zero_()
                    p.hx_dev.zero_()
                else:
                    assert p.Np == p.B or not np.asarray(i32(has_x2))[p.Np:].any(), 'a pair beyond the plan\'s pair slots'
                    p.XSRC[p.B:].copy_(x2)
                    p.hx_dev.copy_(i32(has_x2))
            if cfg.has_y:
                p.hy_dev.copy_(i32(has_y))
                p.y_dev.copy_(i32(y) if y is not None else torch.zeros(p.B, dtype=torch.int32))
                if p.one_slot is not None:       # rows with one fprop row: their class columns
                    assert np.asarray(i32(has_y))[p._has_y_host.astype(bool)].all(), 'an unlabeled row in the labeled range'
                    p.set_labels_host(np.asarray(i32(y)).astype(np.int64))
            return p
        p, rows = self.set_structure(has_x2, has_y, counts)
        p.feed_active = False       # explicit data supersedes an installed epoch feed (a captured step that
        #                             gathers from the feed then refuses to replay: ``replay`` checks the source)
        n_in = len(np.asarray(has_y.cpu() if torch.is_tensor(has_y) else has_y).reshape(-1))
        sel = torch.as_tensor(rows, device=self.dev) if len(rows) != n_in else None
        p.XSRC[:p.B].copy_(x1.index_select(0, sel) if sel is not None else x1)
        if x2 is not None and cfg.has_pert:
            p.XSRC[p.B:].copy_(x2.index_select(0, sel) if sel is not None else x2)
        if cfg.has_y and cfg.cont:
            yv = np.asarray(y.cpu() if torch.is_tensor(y) else y).astype(np.float32).reshape(n_in, -1) \
                if y is not None else np.zeros((n_in, cfg.dim_y), np.float32)
            p.ylab.copy_(torch.from_numpy(np.ascontiguousarray(yv[rows])))
        elif cfg.has_y:
            yv = np.asarray(y.cpu() if torch.is_tensor(y) else y).astype(np.int64).reshape(-1) if y is not None \
                else np.zeros(n_in, np.int64)
            p.set_labels_host(yv[rows])
        return p

    # ------------------------------------------------------------------------ noise
    def set_noise(self, noise):
        """Inject explicit N(0,1) draws addressed by global row (``oracle.models_ref.make_noise``
        layout: nx1/nx2 (B,X); ez1/ez2/ez2F (L,B,Z1); ez3 (L,Y,B,Z3))."""
        p, cfg = self.plan, self.cfg
        self._noise_stale = True
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32)
        rows, L = p.rows, cfg.L
        p.EX[:p.B].copy_(t(np.asarray(noise['nx1'])[rows]))
        if p.Np:
            pr = rows[p.pair_host]
            p.EX[p.B:].copy_(t(np.asarray(noise['nx2'])[pr]))
            p.E2.copy_(t(np.asarray(noise['ez2'])[:, pr].reshape(L * p.Np, -1)))
        p.E1.copy_(t(np.asarray(noise['ez1'])[:, rows].reshape(L * p.B, -1)))
        if cfg.has_pert:
            p.E2F.copy_(t(np.asarray(noise['ez2F'])[:, rows].reshape(L * p.B, -1)))
        if cfg.has_y and p.Mf:
            ez3 = np.asarray(noise['ez3'])
            slot = p.fp_slot_host
            if p.universal:     # a labeled row's one draw (the reference's, slot 0) belongs to its TRUE class slot
                hy, yv, i = p.hy_dev.cpu().numpy().astype(bool), p.y_dev.cpu().numpy(), p.fp_i_host
                slot = np.where(hy[i] & (slot == yv[i]), 0, slot)
            p.E3.copy_(t(ez3[p.fp_l_host, slot, rows[p.fp_i_host]]))
        if cfg.has_y and cfg.cont:
            p.EY.copy_(t(np.asarray(noise['ey'])[:, rows].reshape(L * p.B, -1)))

    def draw_noise(self, bump=True):
        """Fresh on-device N(0,1) for every draw of the step (Philox, one launch).  ``bump=False``: the
        Philox counter is advanced later, together with the step counter, by ``optimizer_step`` (one
        launch less on the train step's critical path)."""
        n = 1       # the Philox counter counts draw EVENTS (row-keyed draws: see ``_Plan.noise_desc``)
        if self._rec == 'main' and self._tail.noise_ahead:
            self._rng_pending = n         # dual-graph step: the side chain of the PREVIOUS step has drawn them
            return
        lo = 0
        if not (self.training and self.add_noise and self.cfg.add_noise_var > 0):
            # no input noise in this pass (evaluation; ``fit(add_noise=False)``): its rows -- two thirds of the arena at
            # 978 genes -- are not drawn (whole-set evaluation of 8192 rows: 40 -> 15 us); a draw is keyed by (draw id,
            # global row), so the latent draws are the same numbers either way
            lo = self.plan.B + self.plan.Np
        # (an evaluation pass drops nothing: the keep rows at the table's end are not drawn either)
        self._fill_noise(self.plan, lo, keeps=self.training)
        self._noise_stale = True          # (an eager draw: a later replay must draw for its own counter first)
        if bump:
            K.counter_add(self.rng_ctr, n)
        else:
            self._rng_pending = n

    def _fill_noise(self, p, lo=0, keeps=True):
        """the draw launch of plan ``p`` over the rows [lo, end) of its descriptor table: N(0,1) rows and, behind them, the
        keep masks of its dropout sites (``keeps``; a plan without sites: the launch it always was)"""
        if p.drop_sites and keeps:
            K.fill_noise_rows(p.noise, p.noise_table[lo:], self.seed, self.rng_ctr)
            p.masks_injected = False      # (drawn masks replace injected ones)
        else:
            K.fill_normal_rows(p.noise, p.noise_desc[lo:p.n_normal_rows], self.seed, self.rng_ctr)

    @property
    def _drop(self):
        """does the pass being issued drop?  A training pass over a plan with sites; evaluation never does"""
        return bool(self.training and self.plan.drop_sites)

    def dropout_sites(self):
        """the dropout sites of the current plan, in the order of their draws: dicts of ``chain`` (``'c_enc'`` ...), ``layer``
        (the site is the INPUT of that layer, li >= 1), ``M``, ``N`` and ``mask``, the (M, N) keep-mask view in the noise arena"""
        return [dict(s) for s in self.plan.drop_sites]

    def set_dropout_masks(self, masks):
        """Inject explicit keep masks (1.0 / 0.0), next to ``set_noise``: ``masks`` maps a site -- its index in
        ``dropout_sites()`` or its (chain, layer) -- to an (M, N) array; every site must be given.  The masks HOLD: every
        ``train_step(noise=...)`` and every forward / backward on this plan uses them and draws nothing, until something draws
        keep rows again -- a ``train_step()`` without noise, ``draw_noise()`` in training mode, a replay of the captured step --
        which overwrites them and ends the injection (a ``train_step(noise=...)`` after that draws fresh masks)."""
        p = self.plan
        index = {(s['chain'], s['layer']): i for i, s in enumerate(p.drop_sites)}
        given = {(index[k] if not isinstance(k, (int, np.integer)) else int(k)): v for k, v in masks.items()}
        assert sorted(given) == list(range(len(p.drop_sites))), 'set_dropout_masks: a mask for every site'
        for i, v in given.items():
            p.drop_sites[i]['mask'].copy_(torch.as_tensor(np.ascontiguousarray(v), dtype=torch.float32))
        p.masks_injected = True
        self._noise_stale = True

    # ---------------------------------------------------------------------- forward
    def _route(self):      # how the pass being issued runs its heads and its reconstruction rows
        return heads_route(self, self.plan, TRAIN if self.fuse_bwd else LOSS if self.training else EVALUATE)

    def beta_pert(self):
        cfg = self.cfg
        if cfg.anneal_perturb_rate_itermax > 0:
            return anneal_coef(self.iters, cfg.anneal_perturb_rate_itermax, cfg.anneal_perturb_rate_offset)
        return 1.

    def betas(self):
        """(beta_pert, beta_kl, beta_yr) of the current iteration count, as the host evaluates them (src/DrVAE.py:549-562):
        what ``_Plan.set_beta`` writes for the passes whose coefficients are host data (every pass of an engine without
        schedules; evaluation passes over structure plans)"""
        cfg = self.cfg
        kl = anneal_coef(self.iters, cfg.anneal_kl_itermax) if cfg.anneal_kl else 1.
        yr = anneal_coef(self.iters, cfg.anneal_yloss_itermax, cfg.anneal_yloss_offset) if cfg.anneal_yloss else 1.
        return self.beta_pert(), kl, yr

    def schedule_record(self):
        """dict(beta_pert, beta_kl, beta_yr, lr_scale) of the LAST step issued, read back from the device record (one small
        device->host copy, never part of a step)"""
        if self.sched_rec is None:
            raise RuntimeError('schedule_record: the engine was built without an annealing schedule')
        self.join_side()
        return dict(zip(('beta_pert', 'beta_kl', 'beta_yr', 'lr_scale'), self.sched_rec.detach().cpu().tolist()))

    def _anneal_args(self, p):
        """the ``anneal`` argument of ``kernels.batch_masks`` / ``batch_feed(masks=...)`` for plan ``p``"""
        cfg = self.cfg
        return dict(step=self.step_dev, pert=(cfg.anneal_perturb_rate_itermax, cfg.anneal_perturb_rate_offset),
                    kl=cfg.anneal_kl_itermax if cfg.anneal_kl else 0,
                    yl=(cfg.anneal_yloss_itermax if cfg.anneal_yloss else 0, cfg.anneal_yloss_offset),
                    lr=cfg.anneal_lr_itermax if cfg.anneal_learning_rate else 0,
                    mmd_rate=cfg.mmd_rate if (cfg.use_s and cfg.use_MMD) else 0.0, sched=self.sched_rec,
                    w_elbo=p.w_elbo, w_cmpl=p.w_cmpl, c_kld=p.c_kld if cfg.has_y else None,
                    w_klz2=p.w_klz2 if cfg.has_pert else None, w_klp=p.w_klp if cfg.kind == 'pvae' else None)

    def forward(self):
        """The forward pass as a launch sequence; this function only schedules its phases: ``_encoder_forward`` (inputs,
        q(z1|x1), q(z2|x2), perturbation function, samples), then two independent chains -- ``_decoder_forward`` (the big
        GEMMs + NLL) and ``_side_forward`` (fprop / classifier: many small launches).  How the two chains are ordered
        depends on ``_mode()``: DUAL = each chain is recorded into its own graph (``_rec`` says which one is being recorded)
        and device flags order them; FORK_JOIN = one graph, one fork/join per step; EVAL = plain evaluation."""
        cfg, p = self.cfg, self.plan
        if not self.fuse_bwd and self.dev.type == 'cuda' and not torch.cuda.is_current_stream_capturing():
            self.join_side()        # an evaluation forward reads parameters the side chain's tail may still be updating
        if self.fuse_bwd and cfg.annealed and not p.universal:
            raise NotImplementedError('an annealed train step (anneal_kl / anneal_yloss / anneal_learning_rate) runs on the '
                                      "batch-independent plan: set_batch / DeviceBatcher(mode='sampler'), not a structure plan")
        p.set_beta(*self.betas())
        B, Np, L, Z1 = p.B, p.Np, cfg.L, cfg.dim_z1
        rec, r = self._rec, self._route()
        Z1blk = p.ZDEC[:L * B]
        if rec == 'side':           # side-chain graph: the main graph launches these; only the views are needed
            Q = p.c_enc.out[-1]
            Qmu, Qlv = Q[:, :Z1], Q[:, Z1:]
        else:
            Qmu, Qlv = self._encoder_forward(rec, r)
        if p.DZMMD is not None and rec != 'side':
            self._mmd_penalty()
        # ---- two independent chains from here: the classifier / fprop chain (many small launches)
        # runs on a side stream next to the decoder chain (the big GEMMs)
        mode, pub = self._mode(), None
        if mode == DUAL:
            two = cfg.has_pert                      # the decoder's first launch publishes its input final: z2Fz1 samples, else z1
            if rec == 'side' and not cfg.has_y:
                return              # (PVAE: the side chain is the step's tail only, see ``_side_graph_tail``)
            if rec == 'side':
                w0, w2 = self.sync.wait('z1', self.side_ctr), self.sync.wait('z2f', self.side_ctr)
                # the FIRST wait is long by design (the side graph is launched first and sits out the encoder): it
                # stays a one-thread launch -- folded into the 180-workgroup gather behind it, the polling of 180
                # workgroups for ~45 us slowed the main chain by 14 % (0.204 -> 0.233 ms).  The second wait has
                # nothing left to wait for when the side chain reaches it: it rides on the KL row kernel behind it
                K.flag_wait(*w0)
                self._side_forward(Qmu, Qlv, Z1blk, r, (lambda: K.flag_wait(*w2)) if two else None,
                                   mid_park=w2 if (two and not cfg.cont) else None)
                return
            pub = self.sync.pub('z2f' if two else 'z1', self.step_dev)
            if self.L_decx[0].g is not None:             # WeightNorm: the chain's first launch is not the GEMM
                K.flag_publish(*pub)
                pub = None
        elif not self._tail.late_fork:      # (a chip-filling step forks behind the decoder heads' product: ``_decoder_forward``)
            self.branch.fork()
        self._decoder_forward(r, pub)
        if mode == DUAL:
            # (``fold_rows``: no launch on either chain -- ``z2f_post_bwd`` forms the rows)
            klz2 = (self._tail.klz2_on_main or not cfg.has_y) and cfg.has_pert and Np and not self._tail.fold_rows
            P2 = p.c_z2F.out[-1] if klz2 else None
            z2 = ((p.KLZ2, p.KLZ2raw, Qmu, Qlv, P2[:, :Z1], P2[:, Z1:]),
                  dict(qidx=p.qz2_idx, pidx=p.pidx, reps=L, free_bits=True, kl_min=cfg.kl_min)) if klz2 else None
            if cfg.kind == 'pvae':      # (its KL rows against the prior: the main chain's own, the backward reads their raw values)
                zp = ((p.KLP, p.KLPraw, Qmu, Qlv), dict(prior=(0.0, 0.0), free_bits=True, kl_min=cfg.kl_min))
                if klz2:                # ... next to the pairs' rows: one launch for both sets
                    K.kl_rows_fwd_pair(zp, z2)
                    z2 = None
                else:
                    K.kl_rows_fwd(*zp[0], **zp[1])
            if z2 is not None:
                K.kl_rows_fwd(*z2[0], **z2[1])
            return             # main-chain graph: the side chain lives in its own graph on the side stream
        with self.branch:
            self._side_forward(Qmu, Qlv, Z1blk, r)
        if mode == FORK_JOIN:
            return             # train step, single fork/join: the side chain runs on into its backward
        self.branch.join()
        if self.fuse_bwd:
            return             # the loss scalars are assembled on the side chain of backward()
        self._loss_scalars()

    def _encoder_forward(self, rec, r):
        """inputs (explicit batch or the graph-resident feed, + the per-batch masks of a universal plan), q(z1|x1) / q(z2|x2) with
        their samples, the perturbation function q(z2Fz1|z1) with its samples; returns the heads' (mu, logvar) views"""
        cfg, p = self.cfg, self.plan
        B, Np, L, Z1 = p.B, p.Np, cfg.L, cfg.dim_z1
        sigma = cfg.add_noise_var if (self.training and self.add_noise and cfg.add_noise_var > 0) else 0.0
        Z1blk = p.ZDEC[:L * B]
        # ---- inputs (+ training noise N(0,1)*add_noise_var, src/DrVAE.py:404-407,414-417): one gather
        fd = p.live_feed if (self.fuse_bwd and self.training) else None
        # (dual-graph schedule) the step's first launch is where the main chain meets the PREVIOUS step's side chain: its
        # tail (its half of the optimiser sweep, the loss scalars, this step's noise, its counters) must be through --
        # flag ``tail``, published by the tail's last launch.  The optimiser launch used to park on that flag (4.3 us per step
        # at cfg 2, 7.6 us with the sampler feed: the tail is 44-49 us of serial launches against 35 us of main-chain
        # launches behind the join); it only needs the classifier's gradient (flag ``clf_dw``)
        start_park = self.sync.wait('next_step', self.step_dev, add=0) if (rec == 'main' and self._tail.tail_gated) else None
        masks = None
        if p.universal:
            # which rows of THIS batch are pairs / labeled -> coefficient and weight vectors, on the device (with
            # the graph-resident feed: by one more workgroup of the feed's launch)
            gc = None
            if p.global_counts:      # data parallelism: the normalisers are the global batch's counts (table data / set_batch)
                gc = getattr(fd, 'gcounts', None) if fd is not None else p.gcounts_dev
                assert gc is not None, 'this plan normalises by global counts: the feed carries none (DeviceBatcher.bind(dp=...))'
            masks = dict(n_tot=p.n_tot, gcounts=gc, kl_rate=cfg.kl_qz2pz2_rate, pert_rate=cfg.pertloss_rate,
                         yl_rate=cfg.yloss_rate, beta=p.beta_dev, c_nll=p.c_nll, w_recl=p.w_recl,
                         hx=(fd.hx32 if fd is not None else p.hx_dev) if cfg.has_pert else None,
                         hy=(fd.hy32 if fd is not None else p.hy_dev) if cfg.has_y else None,
                         y=(fd.y32 if fd is not None else p.y_dev) if cfg.has_y else None,
                         c_klz2=p.c_klz2 if cfg.has_pert else None, c_yl=p.c_yl, w_pert=p.w_pert, w_yl=p.w_yl,
                         label=p.label_r if cfg.has_y else None, c_klp=p.c_klp if cfg.kind == 'pvae' else None,
                         Np=Np if cfg.has_pert else 0, one_slot=p.one_slot)
            if p.annealed:      # ... and the step's schedule record, its betas folded into the coefficients, the ELBO / CMPL weights
                masks['anneal'] = self._anneal_args(p)
            if fd is None:
                K.batch_masks(B, L, **masks)
        if fd is not None:
            # batch (optimiser step - epoch base) of the epoch's index table, straight from the
            # HBM-resident dataset; also refreshes the label-dependent index buffers
            # (universal plan: dv_batch_masks has the labels; its rows with ONE fprop row get their class columns here)
            lab = cfg.has_y and not cfg.cont and (not p.universal or p.one_slot is not None)
            K.batch_feed(p.XIN, fd.x1, fd.x2, fd.y32, fd.table, fd.n_batches, self.step_dev, fd.base, park=start_park,
                         **self._split_args(p),
                         pair_rows=p.pair_idx if Np else None, noise=p.EX if sigma else None, sigma=sigma,
                         has_y=p.has_y_i32 if (lab and not p.universal) else None, L=L,
                         label_r=p.label_r if (lab and not p.universal) else None,
                         fp_i=p.fp_q if lab else None, fp_lab=p.fp_lab_i32 if lab else None,
                         fp_slot=p.fp_slot_dev if lab else None, fp_cls=p.fp_cls if (lab and p.Mf) else None,
                         onehot=p.Z3IN[:, cfg.dim_z3:] if (lab and p.Mf) else None, n_classes=cfg.dim_y,
                         onehot2=p.FPIN[:, Z1:] if (lab and p.Mf) else None,
                         yf=fd.yf if (cfg.has_y and cfg.cont) else None,
                         ylab=p.ylab if (cfg.has_y and cfg.cont) else None, masks=masks)
            if cfg.use_s:
                # the nuisance classes of the same batch of the table: one-hot columns of the stacked encoder / decoder
                # rows and the class vector the MMD penalty reads (a launch of its own: the feed's descriptor stays as it is)
                assert p.carry_s and getattr(fd, 's32', None) is not None, 'use_s: this feed does not carry the nuisance classes'
                K.nuisance_feed(p.SOHe, p.SOHd, p.s_cls, fd.s32, table=fd.table, n_batches=fd.n_batches, ctr=self.step_dev,
                                base=fd.base, pair_rows=p.pair_idx if Np else None, L=L)
        elif cfg.split_x:
            # raw-count inputs, explicit batch: the SAME launch as the graph-resident feed (targets to XT, encoder rows to XIN)
            # over the plan's own one-batch identity table and zero counters -- x1 = XSRC[:B], x2 = XSRC[B:]; no label
            # outputs, the masks stay with ``dv_batch_masks`` above.  Host-fed and feed steps agree bit for bit
            K.batch_feed(p.XIN, p.XSRC[:B], p.XSRC[B:], None, p.id_table, 1, p.id_zero, p.id_zero, park=start_park,
                         pair_rows=p.pair_idx if Np else None, noise=p.EX if sigma else None, sigma=sigma, L=L,
                         **self._split_args(p))
        else:
            K.rows_gather(p.XIN, p.XSRC, p.xin_idx, noise=p.EX if sigma else None, sigma=sigma, park=start_park)
        # ---- q(z1|x1), q(z2|x2): one pass of the shared encoder; the samples (src/blocks.py:170-174) -- z1
        # for every row and z2 for the pairs, drawn from q(z1|x1), not q(z2|x2) (quirk 1, src/DrVAE.py:427) --
        # leave the heads' launch itself (``fuse_heads``) or one launch of their own
        if r.sample_epi:
            # (... and every z1 sample is copied into the z1 columns of its fprop rows on the way out: the side
            # chain's gather is gone; the class columns are written when the labels are: ``_Plan._refresh_onehot`` /
            # ``dv_batch_feed``)
            Q = p.c_enc.forward(p.enc_in, heads=dict(sample=dict(
                eps=p.E12, out=p.ZDEC[:p.o3], n_src=B, seg_ptr=p.zseg_ptr, seg_rows=p.zseg_rows,
                out4=p.FPIN[:, :Z1] if r.fprop_from_heads else None, out4_ptr=p.fp_ptr_ext if r.fprop_from_heads else None)),
                drop=self._drop)
            Qmu, Qlv = Q[:, :Z1], Q[:, Z1:]
        else:
            Q = p.c_enc.forward(p.enc_in, drop=self._drop)
            Qmu, Qlv = Q[:, :Z1], Q[:, Z1:]
            K.reparam_fwd(p.ZDEC[:p.o3], Qmu, Qlv, p.E12, src_idx=p.z_src_idx)
        if cfg.has_pert:
            # (dual-graph schedule) entry of this launch = the z1 samples are final: lets the side
            # chain's fprop start before the perturbation function has run
            pub1 = self.sync.pub('z1', self.step_dev) if rec == 'main' else None
            if r.sample_epi:
                # z2Fz1 sample, the classifier input z2Fz1 - z1, and the decoder's copy for the pairs
                p.c_z2F.forward([Z1blk], resid=Z1blk, publish=pub1, heads=dict(sample=dict(
                    eps=p.E2F, out=p.Z2F, n_src=L * B, sub=Z1blk, out2=p.D, out3=p.ZDEC if Np else None,
                    out3_idx=p.pert_out_idx if Np else None)), drop=self._drop)
            else:
                P2 = p.c_z2F.forward([Z1blk], resid=Z1blk, publish=pub1, drop=self._drop)
                K.reparam_fwd(p.Z2F, P2[:, :Z1], P2[:, Z1:], p.E2F, sub=Z1blk, out2=p.D,
                              out3=p.ZDEC if Np else None, out3_idx=p.pert_out_idx if Np else None)
        return Qmu, Qlv

    def _lib_kw(self):
        """``library=True`` for the reconstruction rows of a ``library_size`` model; no keyword otherwise (the call as it was)"""
        return dict(library=True) if self.cfg.library_size else {}

    def _split_args(self, p):
        """the split-form keywords of ``kernels.batch_feed`` for plan ``p`` (raw-count inputs); none with both switches off"""
        return dict(xt=p.XT, transform=self.cfg.x_transform) if self.cfg.split_x else {}

    def _decoder_forward(self, r, pub=None):
        """p(x|z): the decoder over all stacked sample rows, then the NLL over genes by the launch ``r.nll`` names (``heads_route``:
        in a latency-bound train step the heads' launch itself, ``dv_gemm_heads``); ``pub``: published on entry of the first launch"""
        cfg, p = self.cfg, self.plan
        X, train = cfg.dim_x, self.fuse_bwd
        if r.nll == 'heads':   # train step: the heads' launch emits d/d(mu, pre-softplus) and the row sums' partials
            p.c_decx.forward(p.dec_in, publish=pub, heads=dict(out=p.DPX, nll=dict(
                x=p.XIN, xidx=p.tgt, coef=p.c_nll, part=p.NLLP)), drop=self._drop)
            return
        # ``raw_last``, chip-filling heads in a train step: the product runs with the plain epilogue, the NLL row pass behind it
        # adds the bias and applies softplus + shift on its way (wide configuration: 10.87 -> 9.97 ms for the launch)
        # ... and an EVALUATION pass over many rows (whole-set evaluation, round 5): the heads are needed for the row terms only
        # -- plain product, finished inside the row pass (32768 x 1956 x 600: 737 -> 589 us for the product, and no
        # 256 MB of finished heads written and read back)
        PX = p.c_decx.forward(p.dec_in, publish=pub, raw_last=r.raw_last, x3=r.x3, drop=self._drop)
        if self._tail.late_fork:      # (chip-filling step: the side chain starts HERE, next to the row pass below)
            self.branch.fork()
        lh = p.c_decx.layers[-1]
        if r.nll == 'gene':    # gene-wise theta: the heads are [mean] or [mean | dropout logit], theta is read from its vector
            self._gene_rows(PX, train)
        elif r.nll == 'rec':   # Bernoulli / Poisson / (zero-inflated) negative-binomial rows (+ the gradient w.r.t. the head's pre-activation in a train step)
            K.rec_nll_rows(p.NLL, p.XT if cfg.split_x else p.XIN, PX, kind=cfg.type_rec, shift=cfg.rec.heads[0].shift,
                           xidx=p.tgt, coef=p.c_nll if train else None, dpre=p.DPX if train else None, **self._lib_kw())
        elif r.nll in ('raw_cs', 'raw_cs_eval'):
            # the row terms from the raw heads (bias + softplus + shift applied by the pass); train step: and the gradients,
            # the heads' bias gradient with them (column sums of the gradients this pass writes: no second pass over them)
            grads = (p.DPX[:, :X], p.DPX[:, X:], p.NLLWS, p.c_nll) if train else (None,) * 4
            K.nll_rows_raw_cs(p.NLLC, *grads, p.XIN, PX[:, :X], PX[:, X:], (lh.b[:X], lh.b[X:]), xidx=p.tgt, sd_shift=lh.shift1)
            if train:
                K.colsum(lh.db, p.NLLWS)
        elif r.nll == 'fwdbwd':        # train step: d/d(mu, pre-softplus) emitted in the same row pass
            K.nll_rows_fwdbwd(p.NLL, p.DPX[:, :X], p.DPX[:, X:], p.c_nll, p.XIN, PX[:, :X], PX[:, X:], mode=GAUSS_SIGMA,
                              xidx=p.tgt, sd_act='softplus', sd_shift=lh.shift1 if r.raw_last else 1e-3,
                              bias=(lh.b[:X], lh.b[X:]) if r.raw_last else None)
        else:                          # 'fwd' | 'raw_eval' (gene counts that are no multiple of 4 -- 978: the wave-per-row pass)
            raw = dict(bias=(lh.b[:X], lh.b[X:]), sd_shift=lh.shift1) if r.raw_last else {}
            K.nll_rows_fwd(p.NLL, p.XIN, PX[:, :X], PX[:, X:], mode=GAUSS_SIGMA, xidx=p.tgt, **raw)

    def _gene_rows(self, PX, grads):
        """the reconstruction rows of a ``dispersion='gene'`` model (``gene_rows.gene_rows``): per-chunk row partials into
        ``NLLG``; ``grads``: and the heads' gradients into ``DPX``, the per-block column sums of theta's into ``GWS`` -- summed
        into the vector's gradient by ``_gene_theta_grad``, behind the decoder's backward products.  ``'gene-batch'``: the same
        through ``gene_batch_rows`` with the plan's class operands; ``GWS`` then holds a segment of X columns per class"""
        cfg, p, X = self.cfg, self.plan, self.cfg.dim_x
        zi = cfg.type_rec == 'zinb'
        gk = dict(coef=p.c_nll, dmu=p.DPX[:, :X], dlogit=p.DPX[:, X:] if zi else None, ws=p.GWS) if grads else \
            dict(row_blocks=p.GWS.shape[0])
        kw = dict(kind=cfg.type_rec, shift=cfg.rec.heads[0].shift, logit=PX[:, X:] if zi else None, xidx=p.tgt,
                  library=cfg.library_size, size=p.GSIZE, **gk)
        if cfg.dispersion == 'gene-batch':     # a theta per (class, gene): the classes of the decoder rows are the plan's
            cls, cls_src = p.gene_cls()
            GB.gene_batch_rows(p.NLLG, p.XT if cfg.split_x else p.XIN, PX[:, :X], self.arena.p(GENE_THETA), cls,
                               cls_src=cls_src, **kw)
            return
        G.gene_rows(p.NLLG, p.XT if cfg.split_x else p.XIN, PX[:, :X], self.arena.p(GENE_THETA), **kw)

    def _gene_theta_grad(self):
        """d loss / d raw_theta = the column sum of ``GWS`` over the row blocks.  Only the optimiser sweep (and a gradient
        exchange) reads it, so it is no launch in front of the decoder's data gradient: it follows the decoder's backward
        products, in front of the point where the decoder's gradients count as final"""
        g = self.arena.g(GENE_THETA)           # ((dim_s, dim_x) table: the classes' segments of ``GWS`` back to back)
        K.colsum(g.view(-1), self.plan.GWS[:, :g.numel()])

    def _side_forward(self, Qmu, Qlv, Z1blk, r, mid=None, mid_park=None):
        """fprop first: it only needs the z1 samples, so (dual-graph schedule) it can start before
        the perturbation function has run; ``mid`` then waits for the z2Fz1 samples.  ``mid_park``
        (dual-graph schedule): that wait rides on the launch that follows it where that is a row kernel
        with a small grid (one launch less); else ``mid``, a wait launch of its own."""
        cfg, p = self.cfg, self.plan
        B, Np, L, Z1 = p.B, p.Np, cfg.L, cfg.dim_z1
        if cfg.kind == 'pvae':
            K.kl_rows_fwd(p.KLP, p.KLPraw, Qmu, Qlv, prior=(0.0, 0.0), free_bits=True, kl_min=cfg.kl_min)
        if cfg.has_y and cfg.cont:
            # regression head (src/DrVAE.py:159-169,503-530): q(y|.) first -- the fprop of an unlabeled
            # row conditions on a SAMPLE of it -- then one fprop row per classifier row
            if mid is not None:
                mid()
            if cfg.has_pert and Np:
                P2 = p.c_z2F.out[-1]
                K.kl_rows_fwd(p.KLZ2, p.KLZ2raw, Qmu, Qlv, P2[:, :Z1], P2[:, Z1:], qidx=p.qz2_idx, pidx=p.pidx,
                              reps=L, free_bits=True, kl_min=cfg.kl_min)
            Z3, Y = cfg.dim_z3, cfg.dim_y
            if cfg.kind == 'drvae':
                clf_in = [Z1blk, p.D] if cfg.clf_z1z2 else [p.Z2F]
            else:
                clf_in = [Z1blk]
            QYm = p.c_clf.forward(clf_in, drop=self._drop)                         # sigmoid-constrained means
            K.rows_gather(p.FPIN[:, :Z1], Z1blk, p.fp_src)
            K.ycont_fwd(p.YLrow, p.FPIN[:, Z1:], p.Z3IN[:, Z3:], QYm, p.ylab, p.has_y_i32, p.EY, Y_LOGVAR_CONT, B,
                        sqerr=cfg.kind == 'vfae')       # VFAE scores by squared error (src/VFAE.py:351)
            Q3 = p.c_top.forward([p.FPIN], drop=self._drop)
            K.kl_rows_fwd(p.KL3, p.KL3raw, Q3[:, :Z3], Q3[:, Z3:], prior=(0.0, 0.0), free_bits=True,
                          kl_min=cfg.kl_min, eps=p.E3, zout=p.Z3IN[:, :Z3])
            PZ1 = p.c_dz1.forward([p.Z3IN], drop=self._drop)
            K.kl_rows_fwd(p.KLDrow, p.KL1raw, Qmu, Qlv, PZ1[:, :Z1], PZ1[:, Z1:], qidx=p.fp_q, free_bits=True,
                          kl_min=cfg.kl_min, add=p.KL3)
            return
        # ---- fprop over (labeled: true class | unlabeled: every class)
        if cfg.has_y:
            if p.Mf:
                Z3, Y = cfg.dim_z3, cfg.dim_y
                if not r.fprop_from_heads:
                    K.rows_gather(p.FPIN, Z1blk, p.fp_src, onehot_cls=p.fp_cls, n_classes=Y)
                # (evaluation passes over many fprop rows -- whole-set evaluation: 24576 -- take the plain product + row pass:
                # the 32 x (16 + 16) paired-heads tiles are the latency-bound sizes' kernel; 3.33 -> 3.27 ms per pair)
                if r.z3_in_heads:
                    # the z3 sample leaves the heads' launch of q(z3|z1,y); its KL term against N(0,I) (with its
                    # own free bits) is evaluated next to the z1 term below: one launch less
                    Q3 = p.c_top.forward([p.FPIN], heads=dict(sample=dict(eps=p.E3, out=p.Z3IN[:, :Z3], n_src=p.Mf)), drop=self._drop)
                    PZ1 = p.c_dz1.forward([p.Z3IN], drop=self._drop)
                    # KLFP = max(KL(q(z1|x)||p(z1|z3,y)), kl_min) + max(KL(q(z3|.)||N(0,I)), kl_min)  (src/DrVAE.py:347,358)
                    # -- in the train step inside the classifier-head launch below (``fprop_tail``)
                    if not r.fprop_tail:
                        K.kl_rows_fwd(p.KLFP, p.KL1raw, Qmu, Qlv, PZ1[:, :Z1], PZ1[:, Z1:], qidx=p.fp_q,
                                      free_bits=True, kl_min=cfg.kl_min, prior=(0.0, 0.0),
                                      second=(Q3[:, :Z3], Q3[:, Z3:], p.KL3raw))
                else:
                    Q3 = p.c_top.forward([p.FPIN], drop=self._drop)
                    # KL(q(z3|z1,y)||N(0,I)) with free bits + the z3 sample, one row pass
                    K.kl_rows_fwd(p.KL3, p.KL3raw, Q3[:, :Z3], Q3[:, Z3:], prior=(0.0, 0.0), free_bits=True,
                                  kl_min=cfg.kl_min, eps=p.E3, zout=p.Z3IN[:, :Z3])
                    PZ1 = p.c_dz1.forward([p.Z3IN], drop=self._drop)
                    # KLFP = max(KL(q(z1|x)||p(z1|z3,y)), kl_min) + the z3 term   (src/DrVAE.py:347,358)
                    K.kl_rows_fwd(p.KLFP, p.KL1raw, Qmu, Qlv, PZ1[:, :Z1], PZ1[:, Z1:], qidx=p.fp_q, free_bits=True,
                                  kl_min=cfg.kl_min, add=p.KL3)
        # KL(q(z2|x2)||p(z2|z1)) of the pairs: both arguments come from the main chain and its consumers are the
        # main chain's z2Fz1 backward and the loss scalars -- in the dual-graph train step the MAIN chain computes
        # it (it has time to spare in front of the join, the side chain has not); then the wait for the z2Fz1
        # samples rides on the classifier launch
        klz2_here = cfg.has_pert and Np and not self._tail.klz2_on_main and not self._tail.fold_rows
        # (a parked launch polls from every workgroup: small grids only -- the C side refuses more than 512)
        clf_park = (mid_park is not None and not klz2_here and cfg.has_y and self.clf_small
                    and (L * B + 3) // 4 <= 256)
        fold_mid = mid_park is not None and klz2_here and (L * Np + 3) // 4 <= 256
        if mid is not None and not fold_mid and not clf_park:
            mid()
        if klz2_here:
            P2 = p.c_z2F.out[-1]
            K.kl_rows_fwd(p.KLZ2, p.KLZ2raw, Qmu, Qlv, P2[:, :Z1], P2[:, Z1:], qidx=p.qz2_idx, pidx=p.pidx,
                          reps=L, free_bits=True, kl_min=cfg.kl_min, park=mid_park if fold_mid else None)
        # ---- q(y|.)
        if cfg.has_y:
            if cfg.kind == 'drvae':
                clf_in = [Z1blk, p.D] if cfg.clf_z1z2 else [p.Z2F]
            else:
                clf_in = [Z1blk]
            ym = (p.YLrow, p.KLDrow, p.CFP, p.DQY, p.label_r, p.fp_ptr, p.KLFP, p.log_prior, p.c_kld, p.c_yl)
            if self.clf_small:
                lc = self.L_clf[0]
                # train step: the y-marginalisation (forward and backward) rides on the classifier's launch
                fk = None
                if r.fprop_tail:
                    # the fprop rows' KL terms in front of the y-marginalisation and the backward of the z1 term
                    # (with the coefficients it has just produced) behind it: same launch
                    fk = dict(Q=p.c_enc.out[-1], qidx=p.fp_q, P=p.c_dz1.out[-1], Q3=p.c_top.out[-1], Z1=Z1,
                              Z3=cfg.dim_z3, kl_min=cfg.kl_min, raw1=p.KL1raw, raw3=p.KL3raw, dq=p.DQFP, dp=p.DPZ1)
                # ``fold_rows``: ... and so does the classifier's data gradient, from the DQY the launch has just stored: d/dz2F
                # whole, of d/dz1 the W[:, :Z1] part (``z2f_post_bwd`` adds the fprop rows' sum and -d/dz2F, as
                # ``smalln_bwd_data`` did: same bits)
                fold = dict(dgrad=[(p.DZ1C, 0, 1.0, 0.0), (p.DZ2F, Z1, 1.0, 0.0)]) if self._tail.fold_rows else {}
                K.smalln_fwd(p.QY, None, clf_in[0], lc.W, lc.b, clf_in[1] if len(clf_in) > 1 else None,
                             ymarg=ym if self.fuse_bwd else None, park=mid_park if clf_park else None, fprop_kl=fk, **fold)
            else:
                K.softmax_clamp_fwd(p.QY, p.c_clf.forward(clf_in, drop=self._drop), sigmoid1=cfg.clf_1sig)
            if not self.fuse_bwd:
                K.ymarg_fwd(p.YLrow, p.KLDrow, p.QY, p.label_r, p.fp_ptr, p.KLFP, p.log_prior)
            elif not self.clf_small:    # train step: CFP / DQY of the backward pass come out of the same launch (clf_small: ``ymarg`` above)
                K.ymarg_fwdbwd(p.YLrow, p.KLDrow, p.CFP, p.DQY, p.QY, p.label_r, p.fp_ptr, p.KLFP, p.log_prior,
                               p.c_kld, p.c_yl)

    def join_side(self):
        """Order the CURRENT stream behind everything the side chain has been given so far.  After a ``replay()`` of the
        dual-graph step the side chain's tail (its half of the optimiser sweep, the loss scalars, the next step's noise) is
        awaited only by the NEXT captured step (tail gating), so whatever else touches parameters, moments or loss scalars
        on the current stream -- ``losses()``, an eager ``train_step``, an evaluation forward, ``capture()``, a checkpoint
        -- goes through here first (one event record + wait; no host sync)."""
        if self._side_graph is not None and self.dev.type == 'cuda':
            torch.cuda.current_stream().wait_stream(self.flag_side)

    def _dual_capable(self, on_gpu=None):
        """may this model's train step run as two flag-ordered graphs?  With a classifier the side chain is the fprop /
        classifier chain and the step's tail; PVAE (no classifier) has only the tail to give it -- the decoder heads' half of
        the optimiser sweep, the loss scalars, the next step's noise (cfg 1: 20 serial launches -> 16 + a 4-launch tail)"""
        # (``on_gpu``: see ``_step_tail``)
        cfg = self.cfg
        if cfg.has_y:
            return self.branch.on if on_gpu is None else bool(self.concurrent and on_gpu)
        return bool(cfg.kind == 'pvae' and self.concurrent and cfg.optim_alg in ('adam', 'adamw'))

    def _side_adam_layout(self):
        """(may the side chain sweep the decoder heads' half of the arena?, first element of that half)"""
        heads = self.L_decx[-1]
        g0 = self.arena.grad.storage_offset()
        hs = min(heads.dW.storage_offset(), heads.db.storage_offset()) - g0
        ok = bool(len(self.L_decx) > 1 and heads.g is None and hs % 4 == 0 and self.arena.n_live == self.arena.n_params
                  and max(heads.dW.storage_offset() + span(heads.dW),
                          heads.db.storage_offset() + heads.db.numel()) - g0 >= self.arena.n_live - 3)
        return ok, hs

    def sync_side_counters(self):
        """the side chain's counters and its tail flag follow the step counter (after it was set from outside: a
        restored checkpoint, a capture)"""
        self.side_ctr.copy_(self.step_dev)
        self.side_t.copy_(self.step_dev + 1)
        self.sync.flag('tail').copy_(self.step_dev)

    def _mmd_penalty(self):
        """Model-level MMD penalty of the ``use_s`` extension (src/DrVAE.py:394-398,537-540): minus the MMD between
        the latent samples of each nuisance class and the rest, per data group and Monte-Carlo sample, on z1 and
        (pairs) z2.  A cross-row term: evaluated with the block-level MMD operators (``blocks.mmd_criterion`` -> the
        HIP MMD kernels, forward and backward) on the sample rows of the stacked decoder input; value -> the loss
        tail, gradient -> ``DZMMD``, added to d/dz behind the decoder's backward pass.  Capturable: the row lists of
        every category are plan data (``_Plan.set_s_host``), the random Fourier features come from torch's
        graph-safe device generator; a captured step is valid for the composition of nuisance classes it was
        captured with (``replay`` checks)."""
        cfg, p = self.cfg, self.plan
        if p.mmd_masked is not None:
            # ... on a universal plan: the batch's data groups are read inside the launches too, from the flags dv_batch_masks
            # reads (the live feed's, through its table, or the explicit batch's).  Same two draws, same two launches
            g = p.mmd_masked
            if g['W'] is not None:
                g['W'].normal_()
                g['b'].uniform_()
            fd = p.live_feed if (self.fuse_bwd and self.training) else None
            if fd is not None:
                g = dict(g, hx=fd.hx32 if cfg.has_pert else None, hy=fd.hy32 if cfg.has_y else None, table=fd.table,
                         n_batches=fd.n_batches, ctr=self.step_dev, base=fd.base)
            else:
                g = dict(g, hx=p.hx_dev if cfg.has_pert else None, hy=p.hy_dev if cfg.has_y else None)
            K.mmd_masked_fwd(g)
            K.mmd_masked_bwd(g)
            return
        if p.mmd_grouped is not None:
            # device-carried nuisance classes: ALL terms in one launch per direction, membership read from ``s_cls``; fresh
            # random features for every term from torch's graph-safe device generator (two launches), kept readable in the
            # stacked buffers.  An empty side of a term and a zero difference are defined as value 0, gradient 0
            g = p.mmd_grouped
            if g['W'] is not None:
                g['W'].normal_()
                g['b'].uniform_()
            K.mmd_grouped_fwd(g)
            K.mmd_grouped_bwd(g)
            return
        if cfg.kernel_MMD in ('rbf_fourier', 'identity') and getattr(p, 'mmd_items', None) and T.get('mmd_explicit'):
            return self._mmd_penalty_launches()
        from . import blocks as blk
        with torch.enable_grad():
            z = p.ZDEC[:p.o3].detach().clone().requires_grad_(True)
            total = z.new_zeros(())
            for rows, sind, pairs in p.mmd_calls:
                total = total + blk.mmd_criterion(z.index_select(0, rows), sind, cfg.kernel_MMD, pairs=pairs) / cfg.L
            total.backward()
        p.MMDval.copy_(total.detach().reshape(1))
        # CMPL = ... - mmd_rate * MMD_sum / N_total  (src/DrVAE.py:616,623-624)
        p.DZMMD.copy_(z.grad * (-cfg.mmd_rate / p.n_tot))

    def _mmd_penalty_launches(self):
        """the same penalty WITHOUT autograd (round 6): per call and category pair an explicit launch list -- gather both sides'
        sample rows, [random Fourier features: draw W ~ N(0,1), b ~ U(0,1) in the block's order; ONE projection product over both
        sides with the scale / bias epilogue; cos / column means / difference (``dv_mmd_rff_fwd``)] or [the difference of the
        column means (``dv_mmd_identity_fwd``)], value -w sqrt(mmd^2) into ``MMDval``, the gradient of that -- times the
        penalty's factor in CMPL -- back through the same kernels and added to the rows' slots of ``DZMMD``: 13 launches per
        term instead of ~38 (cfg 4 with the penalty: 0.543 -> 0.379 ms per step, same box).  Same draws in the same order as
        the block-level path, same kernels: the two agree to rounding (``tests/test_gpu_models.py``)."""
        cfg, p = self.cfg, self.plan
        Z, rff = cfg.dim_z1, cfg.kernel_MMD == 'rbf_fourier'
        R = 500                                                  # dim_r of blocks.mmd_fourier (src/blocks.py:40)
        a, c = math.sqrt(2. / 2.) / math.sqrt(Z), math.sqrt(2. / R)     # bandwidth 2 (blocks.mmd_objective)
        z = p.ZDEC[:p.o3]
        dev = z.device
        bufs = p.__dict__.get('_mmd_bufs')
        if bufs is None:
            f = lambda *shape: torch.zeros(*shape, device=dev)
            nmax = max(it['n0'] + it['n1'] for it in p.mmd_items)
            bufs = p._mmd_bufs = dict(zz=f(nmax, _pad4(Z))[:, :Z], dz=f(nmax, _pad4(Z))[:, :Z], diff=f(R if rff else Z), m2=f(1),
                                      rs=f(1), g=f(1))
            if rff:
                bufs.update(th=f(nmax, R), G=f(nmax, R), W=f(Z, R), b=f(R), bias=f(R), scale=torch.full((R,), a, device=dev))
        B_ = bufs
        p.DZMMD.zero_()
        p.MMDval.zero_()
        fac = -cfg.mmd_rate / p.n_tot                            # CMPL = ... - mmd_rate * MMD_sum / N_total
        for it in p.mmd_items:
            n0, n1 = it['n0'], it['n1']
            n = n0 + n1
            zz, dz = B_['zz'][:n], B_['dz'][:n]
            K.rows_gather(zz, z, it['idx32'])
            if rff:
                th, G = B_['th'][:n], B_['G'][:n]
                B_['W'].normal_()
                B_['b'].uniform_()
                torch.mul(B_['b'], 2 * math.pi, out=B_['bias'])
                K.gemm(th, zz, B_['W'], True, False, epi=K.EPI_FWD, scale=B_['scale'], bias=B_['bias'])
                K.mmd_rff_fwd(B_['diff'], B_['m2'], th[:n0], th[n0:], c)
            else:
                K.mmd_identity_fwd(B_['diff'], B_['m2'], zz[:n0], zz[n0:])
            torch.rsqrt(B_['m2'], out=B_['rs'])
            p.MMDval.addcmul_(B_['m2'], B_['rs'], value=-it['w'])         # - w sqrt(mmd^2)
            torch.mul(B_['rs'], -0.5 * it['w'] * fac, out=B_['g'])         # d(that, times the CMPL factor) / d(mmd^2)
            if rff:
                K.mmd_rff_bwd(G[:n0], th[:n0], B_['diff'], B_['g'], 2.0 * c / n0)
                K.mmd_rff_bwd(G[n0:], th[n0:], B_['diff'], B_['g'], -2.0 * c / n1)
                K.gemm(dz, G, B_['W'], True, True, alpha=a)
            else:
                K.mmd_identity_bwd(dz[:n0], B_['diff'], B_['g'], 2.0 / n0)
                K.mmd_identity_bwd(dz[n0:], B_['diff'], B_['g'], -2.0 / n1)
            p.DZMMD.index_add_(0, it['idx'], dz)

    def _loss_scalars(self, after=None, terms_elsewhere=False, bump_counters=False):
        """RECL, KLD, PERT, YL, ELBO, CMPL (src/DrVAE.py:611-624) as device scalars.  ``terms_elsewhere``
        (with ``after``): this launch only parks on the flag and advances the counters; the caller has another
        chain assemble the scalars (they are a leaf of the step: only the host reads them)."""
        cfg, p = self.cfg, self.plan
        L = cfg.L
        nll = getattr(p, self._route().rows)     # the buffer this pass's row launch writes
        # (per-tile / per-chunk partials: a row's sum is its term)
        rl = nll.shape[1] if nll.dim() == 2 else 1
        if p.universal:      # normalisers and group masks are per-row weights written by dv_batch_masks
            terms = [(nll[:p.o3], p.w_recl[:p.o3], 1.0, 0, rl)]
            if cfg.has_pert:
                terms.append((nll[p.o3:], p.w_pert[:L * p.Np], 1.0, 2, rl))
                # (annealed plan: c_klz2 carries beta_kl -- the reported KLD is weighted by its copy without)
                terms.append((p.KLZ2, p.w_klz2 if p.annealed else p.c_klz2, 1.0, 1))
        else:
            terms = [(nll[:p.o3], None, 1.0 / (L * p.n_tot), 0)]
            if cfg.has_pert and p.Np:
                terms.append((nll[p.o3:], None, 1.0 / (L * max(1., p.n_pairs)), 2))
                terms.append((p.KLZ2, p.c_klz2, 1.0, 1))           # beta_pert*rate/(L N) lives on the device
        if cfg.kind == 'pvae':
            terms.append((p.KLP, p.w_klp if p.annealed else p.c_klp, 1.0, 1) if p.universal else (p.KLP, None, 1.0 / p.n_tot, 1))
        if cfg.has_y:
            terms.append((p.KLDrow, None, 1.0 / (L * p.n_tot), 1))
            terms.append((p.YLrow, p.w_yl, 1.0, 3) if p.universal else
                         (p.YLrow, None, 1.0 / (L * max(1., p.n_lab)), 3))
        if p.DZMMD is not None:
            terms.append((p.MMDval, None, 1.0 / p.n_tot, 4))
        bump = ()
        if after is not None or bump_counters:     # this launch also advances the step / Philox counters
            bump = [(self.step_dev, 1)] + ([(self.rng_ctr, self._rng_pending)] if self._rng_pending else [])
            self._rng_pending = 0
            self._ctr_bumped = True
        # (train steps also add their scalars to ``loss_sum``: a ``fit`` epoch reads the sums once, at its end)
        K.loss_assemble(self.arena.loss, [] if terms_elsewhere else terms, p.w_elbo, p.w_cmpl, after=after, bump=bump,
                        halt=self.sync_err, accum=self.loss_sum if self.fuse_bwd else None)

    # --------------------------------------------------------------------- backward
    def backward(self):
        """The hand-written backward pass, scheduled like ``forward``: the side chain's share (``_side_backward``; in the
        dual-graph schedule followed by ``_side_graph_tail``) next to the main chain -- decoder, perturbation function,
        samples, encoder -- which joins the side chain's d/dz contributions where it first needs them."""
        cfg, p = self.cfg, self.plan
        B, Np, L, Z1, X = p.B, p.Np, cfg.L, cfg.dim_z1, cfg.dim_x
        Q = p.c_enc.out[-1]
        Qmu, Qlv = Q[:, :Z1], Q[:, Z1:]
        DQ = p.DQ
        Z1blk, DZ1 = p.ZDEC[:L * B], p.DZDEC[:L * B]
        # ---- side chain: y-marginalisation, fprop, classifier -> DZ1B (its share of d/dz1), DZ2F
        # (dual-graph schedule: what the side chain carries behind the join is decided in ``_step_tail``)
        mode, t, r = self._mode(), self._tail, self._route()
        late, leaf = t.late, []

        # ---- main chain: reconstruction terms, d/d(mu, pre-softplus) straight from the per-row
        # coefficients, then back through the decoder (the three big GEMMs)
        PX = p.c_decx.out[-1]
        if not self.fuse_bwd and cfg.rec.gene:
            self._gene_rows(PX, True)
        elif not self.fuse_bwd and cfg.type_rec != 'diag_gaussian':
            K.rec_nll_rows(p.NLL, p.XT if cfg.split_x else p.XIN, PX, kind=cfg.type_rec, shift=cfg.rec.heads[0].shift,
                           xidx=p.tgt, coef=p.c_nll, dpre=p.DPX, **self._lib_kw())
        elif not self.fuse_bwd:
            K.nll_rows_bwd(p.DPX[:, :X], p.DPX[:, X:], p.c_nll, p.XIN, PX[:, :X], PX[:, X:], mode=GAUSS_SIGMA,
                           xidx=p.tgt, sd_act='softplus', sd_shift=1e-3)
        if mode == DUAL and self._rec == 'side':
            self._side_backward(Qmu, Qlv, Z1blk, r, late, leaf)
            self._side_graph_tail(leaf)
            return
        if mode == EVAL:
            self.branch.fork()
        elif mode == FORK_JOIN:
            self.branch._forked = True       # one fork/join per step: the side chain simply continues
        p.c_decx.backward(p.DPX, p.dec_in, [[(p.DZDEC, 1.0, 0.0)]] + [None] * (len(p.dec_in) - 1),
                          publish_after_last=self.sync.pub('rows', self.step_dev) if t.side_loss else None,
                          db_last_done=r.db_done, x3_last=r.x3, drop=self._drop)
        if cfg.rec.gene:
            self._gene_theta_grad()
        if p.DZMMD is not None:
            # model-level MMD penalty (use_s extension): its gradient w.r.t. the z1 / z2 samples was computed in
            # forward() through the block-level MMD kernels (see ``_mmd_penalty``)
            p.DZDEC[:p.o3].add_(p.DZMMD)
        if self._after_decoder_bwd is not None:
            self._after_decoder_bwd()        # decoder_x gradients are final: graph split point of the overlapped exchange
        if mode != DUAL:
            with self.branch:
                self._side_backward(Qmu, Qlv, Z1blk, r, late, leaf)
            self.branch.join()
        park = bump = None
        if t.fold_join:
            # no launch of its own for the join: the first consumer of the side chain's gradients (below) parks on
            # the flag itself, and the counters ride on the sample-backward launch
            park = self.sync.wait('join', self.step_dev)
            bump = [(self.step_dev, 1)] + ([(self.rng_ctr, self._rng_pending)] if self._rng_pending else [])
            self._rng_pending = 0
            self._ctr_bumped = True
        elif mode == DUAL:    # the launch that assembles the loss scalars also parks on the side chain's flag
            self._loss_scalars(after=self.sync.wait('join', self.step_dev), terms_elsewhere=t.side_loss)
        elif mode == FORK_JOIN:         # (the step / Philox counters ride on this launch: two launches less in front of the optimiser)
            self._loss_scalars(bump_counters=True)
        if cfg.has_pert:
            P2 = p.c_z2F.out[-1]
            # everything that hangs on the z2Fz1 samples, one launch: scatter-back of the decoded
            # copies, reparam backward, KL(q(z2|x2)||p(z2|z1)) with free bits (src/DrVAE.py:466,482-487)
            # wrt both arguments, the residual path, and the side chain's share of d/dz1
            # (``fold_rows``: ... and the forward of those KL rows -> KLZ2 / KLZ2raw, and the side chain's share of d/dz1 from its
            # parts: DZ1C + the fprop rows' sum - DZ2F)
            fold = dict(kl_out=p.KLZ2 if Np else None, seg=(p.DFPIN, p.fp_ptr, 1.0) if p.Mf else None, z1_dz2f=-1.0) \
                if t.fold_rows else {}
            K.z2f_post_bwd(p.DP2, DZ1, DQ[B:] if Np else None, p.DZ2F if cfg.has_y else None,     # (no classifier: no gradient into the z2Fz1 samples but the decoder's)
                           p.DZDEC[p.o3:] if Np else None, p.pair_slot,
                           p.E2F, P2, Q[B:] if Np else None, p.c_klz2, p.KLZ2raw, cfg.kl_min,
                           (p.DZ1C if t.fold_rows else p.DZ1B) if cfg.has_y else None, L, B, Np, park=park,
                           prior=(p.c_klp[B:], p.KLPraw[B:]) if (cfg.kind == 'pvae' and Np) else None, **fold)
            # perturbation function: mu = z1 + z1 W^T + b, logvar head
            p.c_z2F.backward(p.DP2, [Z1blk], [[(DZ1, 1.0, 1.0)]], drop=self._drop)
        # (VFAE: the side chain's share of d/dz1 is a second source of the sample backward below, no summing launch of
        # its own.  The join stays the one-workgroup launch above: VFAE's side chain is the longer one, and 59 parked
        # workgroups polling for it slow the very chain they wait for -- cfg 4 0.164 -> 0.170 ms)
        add1 = p.DZ1B if (cfg.has_y and not cfg.has_pert) else None
        # ---- back through the samples into q(z1|x1): L z1-samples (+ L z2-samples for pairs) per row,
        # plus the row-aligned KL(q(z1|x)||p(z1|z3,y)) gradients of the row's fprop rows
        fp = cfg.has_y and p.Mf
        K.reparam_bwd_seg(DQ[:B, :Z1], DQ[:B, Z1:], p.DZDEC, p.E12, Qlv, p.zseg_ptr, p.zseg_rows,
                          extra=p.DQFP if fp else None, ex_ptr=p.q_ptr if fp else None,
                          ex_rows=p.q_rows if fp else None, bump=bump, dz_add=add1,
                          # PVAE's prior term KL(q || N(0,I)) (src/PVAE.py): its gradient rides on the two launches that
                          # write q's gradient rows (here: rows [0, B); ``z2f_post_bwd``: the pairs' q(z2|x2) rows) instead
                          # of a dv_kl_rows_bwd launch behind them (cfg 1: one launch less on the critical chain)
                          prior=(p.c_klp, p.KLPraw, cfg.kl_min, Qmu) if cfg.kind == 'pvae' else None)
        p.c_enc.backward(DQ, p.enc_in, None,
                         publish_first=self.sync.pub('noise', self.step_dev, 0) if t.noise_ahead else None, drop=self._drop)

    def _side_backward(self, Qmu, Qlv, Z1blk, r, late, leaf):
        """the side chain's share of the backward pass: y-marginalisation, fprop blocks, classifier -> ``DZ1B`` (its share
        of d/dz1) and ``DZ2F``.  ``late``: the classifier's weight gradient is deferred (appended to ``leaf``: a leaf of the step
        -- only the optimiser reads it -- that runs behind the side chain's publish)"""
        cfg, p = self.cfg, self.plan
        B, Np, L, Z1 = p.B, p.Np, cfg.L, cfg.dim_z1

        def wgrad_clf(*args):
            ws = getattr(p, 'SNWS', None)       # (row-split workspace: plans with >= 1024 classifier rows)
            if late:
                # (its entry also tells the main chain that the side chain's data gradients are final: see below)
                leaf.append(lambda pub=None: K.smalln_bwd_weight(*args, publish=pub, ws=ws))
            else:
                K.smalln_bwd_weight(*args, ws=ws)

        if cfg.has_y and cfg.cont:
            Y, Z3 = cfg.dim_y, cfg.dim_z3
            PZ1, Q3, QYm = p.c_dz1.out[-1], p.c_top.out[-1], p.c_clf.out[-1]
            K.ycont_bwd(None, p.CFP, QYm, p.ylab, p.has_y_i32, Y_LOGVAR_CONT, p.c_yl, p.c_kld, p.DFPIN[:, Z1:],
                        p.DZ3IN[:, Z3:], B, sqerr=cfg.kind == 'vfae')     # cfp[r] = c_kld[r]: one fprop row per row
            K.kl_rows_bwd(p.DQFP[:, :Z1], p.DQFP[:, Z1:], p.DPZ1[:, :Z1], p.DPZ1[:, Z1:], p.CFP, p.KL1raw,
                          Qmu, Qlv, PZ1[:, :Z1], PZ1[:, Z1:], qidx=p.fp_q, free_bits=True, kl_min=cfg.kl_min)
            p.c_dz1.backward(p.DPZ1, [p.Z3IN], [[(p.DZ3IN, 1.0, 0.0)]], drop=self._drop)
            K.kl_rows_bwd(p.DQ3[:, :Z3], p.DQ3[:, Z3:], None, None, p.CFP, p.KL3raw, Q3[:, :Z3], Q3[:, Z3:],
                          prior=(0.0, 0.0), free_bits=True, kl_min=cfg.kl_min, dz=p.DZ3IN[:, :Z3], eps=p.E3)
            p.c_top.backward(p.DQ3, [p.FPIN], [[(p.DFPIN, 1.0, 0.0)]], drop=self._drop)
            K.rows_segment_sum(p.DZ1B, p.DFPIN, seg_ptr=p.fp_ptr, beta=0.0, width=Z1)
            # the y columns of both fprop inputs carry d/d(y sample); labeled rows: the log-likelihood
            K.ycont_bwd(p.DLOG, None, QYm, p.ylab, p.has_y_i32, Y_LOGVAR_CONT, p.c_yl, p.c_kld, p.DFPIN[:, Z1:],
                        p.DZ3IN[:, Z3:], B, sqerr=cfg.kind == 'vfae')
            if cfg.kind == 'drvae' and cfg.clf_z1z2:
                p.c_clf.backward(p.DLOG, [Z1blk, p.D], [[(p.DZ1B, 1.0, 1.0)], [(p.DZ2F, 1.0, 0.0), (p.DZ1B, -1.0, 1.0)]],
                                 drop=self._drop)
            elif cfg.kind == 'drvae':
                p.c_clf.backward(p.DLOG, [p.Z2F], [[(p.DZ2F, 1.0, 0.0)]], drop=self._drop)
            else:
                p.c_clf.backward(p.DLOG, [Z1blk], [[(p.DZ1B, 1.0, 1.0)]], drop=self._drop)
        elif cfg.has_y:
            Y = cfg.dim_y
            if not self.fuse_bwd:
                K.ymarg_bwd(p.CFP, p.DQY, p.QY, p.label_r, p.fp_ptr, p.KLFP, p.log_prior, p.c_kld, p.c_yl)
            if p.Mf:
                Z3 = cfg.dim_z3
                PZ1, Q3 = p.c_dz1.out[-1], p.c_top.out[-1]
                # KL(q(z1|x) || p(z1|z3,y)): gradient to p (decoder_z1 heads) and, row-aligned, to q
                if not r.fprop_tail:       # (else: left the classifier-head launch of the forward pass)
                    K.kl_rows_bwd(p.DQFP[:, :Z1], p.DQFP[:, Z1:], p.DPZ1[:, :Z1], p.DPZ1[:, Z1:], p.CFP, p.KL1raw,
                                  Qmu, Qlv, PZ1[:, :Z1], PZ1[:, Z1:], qidx=p.fp_q, free_bits=True,
                                  kl_min=cfg.kl_min)
                # KL(q(z3|z1,y) || N(0,I)) + the sample path: in the epilogue of the data-gradient product that produces
                # d/dz3 (``DV_EPI_KLQ``: the side chain in front of the join is a chain of dependent launches -- one less),
                # else a row pass behind it
                klq = dict(out=p.DQ3, q=Q3, eps=p.E3, coef=p.CFP, raw=p.KL3raw, kl_min=cfg.kl_min, Z=Z3) \
                    if self.fuse_bwd else None
                if not p.c_dz1.backward(p.DPZ1, [p.Z3IN], [[(p.DZ3IN, 1.0, 0.0)]], klq=klq, drop=self._drop):
                    K.kl_rows_bwd(p.DQ3[:, :Z3], p.DQ3[:, Z3:], None, None, p.CFP, p.KL3raw, Q3[:, :Z3], Q3[:, Z3:],
                                  prior=(0.0, 0.0), free_bits=True, kl_min=cfg.kl_min, dz=p.DZ3IN[:, :Z3], eps=p.E3)
                p.c_top.backward(p.DQ3, [p.FPIN], [[(p.DFPIN, 1.0, 0.0)]], drop=self._drop)
                # z1 feeds one (labeled) or Y (unlabeled) fprop rows: their d/dz1 is summed per z1 row -- inside
                # the classifier's data-gradient launch where that launch writes DZ1B anyway, else on its own
                seg_in_clf = self.clf_small and not (cfg.kind == 'drvae' and not cfg.clf_z1z2)
                if not seg_in_clf:
                    K.rows_segment_sum(p.DZ1B, p.DFPIN, seg_ptr=p.fp_ptr, beta=0.0, width=Z1)
            # classifier
            b1 = 1.0 if p.Mf else 0.0
            seg = (p.DFPIN, p.fp_ptr) if p.Mf else None
            two = cfg.kind == 'drvae' and cfg.clf_z1z2
            if self.clf_small:
                lc = self.L_clf[0]
                if two:      # input [z1, z2F - z1]: d/dz1 gets W1 - W2, d/dz2F gets W2
                    if not self._tail.fold_rows:      # (else: left the classifier's forward launch, summed by ``z2f_post_bwd``)
                        K.smalln_bwd_data([(p.DZ1B, 0, 1.0, b1, Z1, -1.0), (p.DZ2F, Z1, 1.0, 0.0)], p.DQY, p.QY, lc.W,
                                          seg=seg)
                    wgrad_clf(lc.dW, lc.db, p.DQY, p.QY, Z1blk, p.D)
                elif cfg.kind == 'drvae':
                    K.smalln_bwd_data([(p.DZ2F, 0, 1.0, 0.0)], p.DQY, p.QY, lc.W)
                    wgrad_clf(lc.dW, lc.db, p.DQY, p.QY, p.Z2F)
                    if not p.Mf:
                        p.DZ1B.zero_()
                else:
                    K.smalln_bwd_data([(p.DZ1B, 0, 1.0, b1)], p.DQY, p.QY, lc.W, seg=seg)
                    wgrad_clf(lc.dW, lc.db, p.DQY, p.QY, Z1blk)
            else:
                K.softmax_clamp_bwd(p.DLOG, p.DQY, p.QY, sigmoid1=cfg.clf_1sig)
                if two:
                    p.c_clf.backward(p.DLOG, [Z1blk, p.D],
                                     [[(p.DZ1B, 1.0, b1)], [(p.DZ2F, 1.0, 0.0), (p.DZ1B, -1.0, 1.0)]], drop=self._drop)
                elif cfg.kind == 'drvae':
                    p.c_clf.backward(p.DLOG, [p.Z2F], [[(p.DZ2F, 1.0, 0.0)]], drop=self._drop)
                    if not p.Mf:
                        p.DZ1B.zero_()
                else:
                    p.c_clf.backward(p.DLOG, [Z1blk], [[(p.DZ1B, 1.0, b1)]], drop=self._drop)

    def _side_graph_tail(self, leaf):
        """(dual-graph schedule) what the side chain's graph runs behind its backward pass: publish its data gradients, the
        deferred leaf launches, the decoder heads' half of the optimiser sweep, the loss scalars, the NEXT step's noise, its
        own counters"""
        p, t, sync, ctr = self.plan, self._tail, self.sync, self.side_ctr
        # DZ1B / DZ2F / every side gradient is final (the join): published on entry of the first leaf launch behind them
        # (the classifier's weight gradient) where there is one, else by a launch of its own
        if leaf:
            leaf[0](pub=sync.pub('join', ctr))
            for fn in leaf[1:]:
                fn()
        else:
            K.flag_publish(*sync.pub('join', ctr))
        if t.side_loss:
            # (entry of this launch = the deferred leaf launches, i.e. the classifier's weight gradient, are through:
            # flag ``clf_dw``, what the main chain's optimiser launch gates its classifier slice on)
            K.flag_wait(*sync.wait('rows', ctr), publish=sync.pub('clf_dw', ctr) if t.tail_gated else None)
            if t.side_adam:
                self._sweep(t.hs, self.arena.n_live, step=self.side_t)
            if not t.fold_rows:
                self._loss_scalars()   # a leaf too; the wait above also covers the main chain's NLL rows
        if t.noise_ahead:
            # the next step's N(0,1) draws: every reader of this step's is through once the encoder
            # backward has started (the main chain publishes that), and the Philox counter has advanced.
            # (A park of the draw launch itself instead of the wait launch was measured slower: 356
            # workgroups polling one flag, +10 us/step)
            K.flag_wait(*sync.wait('noise', ctr))
            if t.fold_rows:
                # the pairs' KL rows are written by ``z2f_post_bwd``, behind the join: the loss scalars follow the wait for
                # flag ``noise``, published behind that launch on the main chain
                self._loss_scalars()
            self._fill_noise(p)
        # ... and now the side chain's late work is final: published by the counter launch on entry
        K.counters_add2(ctr, 1, self.side_t, 1, publish=sync.pub('tail', ctr) if (t.late or t.cap_fork) else None)

    # -------------------------------------------------------------------- optimiser
    def optimizer_step(self, gscale=1.0):
        """torch.optim.Adam with coupled L2 on EVERY parameter (src/DGMMixin.py:36)."""
        cfg, a = self.cfg, self.arena
        if self._ctr_bumped:
            self._ctr_bumped = False          # the loss-scalar launch of this step already advanced them
        elif self._rng_pending:
            K.counters_add2(self.step_dev, 1, self.rng_ctr, self._rng_pending)
            self._rng_pending = 0
        else:
            K.counter_add(self.step_dev, 1)
        if self._rec == 'both' and self.sched == 5 and self._dual_capable():
            # eager step: the side chain's counters follow, and so does the "side chain's tail is through" flag that the
            # NEXT captured step's first launch waits for (published on entry: counter + 1 = the advanced value)
            K.counters_add2(self.side_ctr, 1, self.side_t, 1, publish=self.sync.pub('tail', self.side_ctr))
        if self.averaged:
            raise RuntimeError('the parameter arena holds the AVERAGED parameters (averaged_parameters()): no optimiser step '
                               'inside that context')
        n = a.n_live                      # parameters without gradients sit behind it (untouched, like torch)
        t, gate = (self._tail if self._rec == 'main' else None), None
        if self.clip_rec is not None:
            # clipped step: every gradient is final here (``_step_tail`` records no leaf work behind the join and no
            # side-chain half of the sweep for it), behind the exchange in every exchange form.  The norm over the whole live
            # slice -- the pad elements between parameters are zero, always (``ParamArena``) --, the record, the sweep
            assert not (t and (t.adam_gated or t.cap_fork or t.side_adam)), 'a clipped sweep has no gated form'
            K.clip_norm(a.grad[:n], self.clip_state, gscale=gscale)
            self._sweep(0, n, gscale=gscale)
            return
        if t and t.adam_gated:   # dual-graph step: the classifier's dW may still be in flight on the side chain
            # (the optimiser's gate waits with counter + 0: the step counter is advanced before it)
            if cfg.has_y:
                lc, g0 = self.L_clf[0], a.grad.storage_offset()
                lo = min(lc.dW.storage_offset(), lc.db.storage_offset()) - g0
                hi = max(lc.dW.storage_offset() + span(lc.dW), lc.db.storage_offset() + lc.db.numel()) - g0
            else:       # (no classifier, no leaf gradient in flight: the first workgroup's elements stand in for the slice --
                lo, hi = 0, 4       # the gate is what orders the NEXT step behind the side chain's tail, see ``_step_tail``)
            gate = self.sync.gate('clf_dw' if t.tail_gated else 'tail', self.step_dev, lo, hi)
            n = t.hs if t.side_adam else n      # ... and the side chain sweeps the rest (the decoder heads)
        if t and t.cap_fork:
            # (the sweep's first workgroup also parks on the side chain's "tail through" flag: what orders the NEXT step --
            # its first launch reads the noise the side chain has drawn -- behind it)
            gate = self.sync.gate('tail', self.step_dev, 0, 4)
        self._sweep(0, n, gscale=gscale, gate=gate)

    def _sweep(self, lo, hi, *, gscale=None, gate=None, step=None):
        """the optimiser sweep over the elements [lo, hi) of the arena -- every sweep of the step, the gated one, the capped
        fork's and the side chain's half included: Adam or Adamax by ``cfg.optim_alg`` (exp_avg_sq doubles as Adamax's exp_inf),
        the clipped form where the engine clips (it counts by the clip state's first word), else by ``step`` (default: the
        step counter; the side chain has its own).  What is switched off is no argument at all, the call as it ever was:
        the rate's annealing coefficient from the step's schedule record, AdamW's decoupled switch, the slice of the
        parameter average that belongs to the elements, the gate, the gradient's scale (the side chain's half runs only in
        steps without an exchange: it has none)"""
        cfg, a = self.cfg, self.arena
        name = ('adamax_l2' if cfg.optim_alg == 'adamax' else 'adam_l2') + ('_clip' if self.clip_rec is not None else '')
        if self.clip_rec is not None:
            step = self.clip_state
        elif step is None:
            step = self.step_dev
        kw = {}
        if gscale is not None:
            kw['gscale'] = gscale
        if gate is not None:
            kw['gate'] = gate
        if cfg.anneal_learning_rate:
            kw['lr_scale'] = self.sched_rec[3:4]
        if cfg.optim_alg == 'adamw':
            kw['decoupled'] = True
        if cfg.ema_decay is not None:
            kw.update(avg=a.avg[lo:hi], avg_decay=cfg.ema_decay)
        getattr(K, name)(a.param[lo:hi], a.grad[lo:hi], a.exp_avg[lo:hi], a.exp_avg_sq[lo:hi], step, lr=cfg.learning_rate,
                         weight_decay=cfg.weight_decay, halt=self.sync_err, **kw)

    def _refuse_averaged(self, what):
        if self.averaged:
            raise RuntimeError('%s inside averaged_parameters(): the parameter arena holds the averaged values, a train '
                               'step would train them' % what)

    def swap_average(self):
        """exchange the CONTENTS of the parameter arena and of the average (the whole arena: pads and the frozen tail are
        equal in both), through the gradient arena -- dead between steps -- as scratch.  Three copies on the current stream,
        behind the side chain; twice is the identity, bit for bit"""
        a = self.arena
        if not hasattr(a, 'avg'):
            raise RuntimeError('the engine was built without ema_decay: there is no parameter average')
        self.join_side()
        with torch.no_grad():
            a.grad.copy_(a.param)
            a.param.copy_(a.avg)
            a.avg.copy_(a.grad)
        self.averaged = not self.averaged

    def clip_stats(self):
        """dict(norm, coef, skipped_last, n_skipped) of the last clipped optimiser step as python numbers: the gradient's
        global 2-norm (times |gscale|), the coefficient the sweep scaled it by, whether that step was skipped for a
        non-finite gradient, and how many steps have been skipped so far.  One small device->host copy, never part of a step."""
        if self.clip_rec is None:
            raise RuntimeError('clip_stats: the engine was built without max_grad_norm')
        self.join_side()
        return K.clip_record_values(self.clip_rec)

    def train_step(self, noise=None, allreduce=None):
        """forward + backward (+ gradient all-reduce) + Adam + iteration count: the body of
        ``run_on_batch(train_mode=True)`` (src/DGMMixin.py:91-126)."""
        self._refuse_averaged('train_step')
        self.training = True
        self.join_side()
        if noise is not None:
            self.set_noise(noise)
            if self.plan.drop_sites and not self.plan.masks_injected:
                # injected noise, no injected masks: the keep rows alone are drawn (their own draw event)
                p = self.plan
                K.fill_noise_rows(p.noise, p.noise_table[p.n_normal_rows:], self.seed, self.rng_ctr)
                self._rng_pending = 1
        else:
            self.draw_noise(bump=False)
        self._launch_sequence(allreduce=allreduce, draw=False)
        self.iters += 1

    def losses(self):
        """OrderedDict of python floats (one device->host copy; the only sync of a step)."""
        self.join_side()         # (the loss scalars are assembled by the side chain's tail: see join_side)
        v = self.arena.loss.detach().cpu().tolist()
        if self._side_graph is not None:
            self.check_sync()
        keys = ['RECL', 'KLD', 'PERT', 'YL', 'MMD', 'ELBO', 'CMPL']
        if self.cfg.kind == 'pvae':
            keys.remove('YL')
        if self.cfg.kind == 'vfae':
            keys.remove('PERT')
        return OrderedDict((k, v[LOSS_IDX[k]]) for k in keys)
