"""Drug Perturbation VAE -- counterpart of reference ``src/PVAE.py`` (class ``PVAE``)."""
from ._model_base import ELBOModel


class PVAE(ELBOModel):
    """p(x1,x2,z1,z2) = p(z1)p(z2|z1)p(x1|z1)p(x2|z2); q(z1|x1), q(z2|x2) share one encoder.

    ``dropout_rate`` > 0 drops every hidden activation in front of the layer that reads it, inside the fused train step (keep
    masks drawn on the device with the step's noise; evaluation and inference drop nothing).  Two labelled differences from
    the block-level path and the reference, named by one warning at construction: the two heads of a block share ONE keep
    mask (each head's marginal is the reference's, the joint is not), and a block without a hidden layer -- always
    ``decoder_z2Fz1``, whose log-variance head alone the reference drops -- is not dropped at all.
    ``dropout_rate`` >= 1 raises ``ValueError``.
    ``max_grad_norm`` (default None: off) clips the global 2-norm of the gradient inside the fused step, with the semantics of
    ``torch.nn.utils.clip_grad_norm_`` in front of the optimiser, and guards it: a step whose gradient holds an inf or a NaN
    is skipped -- parameters and optimiser state stay as they are, ``grad_clip_stats()['n_skipped']`` counts it, ``fit`` warns
    once per epoch in which it happened.  ``float('inf')`` keeps the guard and clips nothing.  A clipped step gives up the
    side chain's share of the optimiser sweep.  0, a negative number or NaN raise ``ValueError``.
    ``anneal_kl`` / ``anneal_yloss`` / ``anneal_learning_rate`` (default off, as the reference's drivers leave them) ramp the
    weight of ``KLD`` in the ELBO, of ``yloss_rate * YL`` in the compound loss and the learning rate over ``anneal_kl_itermax``
    / ``anneal_yloss_itermax`` (+ ``anneal_yloss_offset``) / ``anneal_lr_itermax`` iterations inside the fused step; the
    schedule is evaluated on the device from the step counter.  They may also be set as attributes until the first step
    builds the engine (a later change raises).  Annealed training runs on the batch-independent plans: configurations
    without one, and the stratified ``DeviceBatcher``, raise ``NotImplementedError``.  A switch that is on with an
    ``itermax`` <= 0 raises ``ValueError``.  The learning-rate schedule is a labelled extension.
    ``ema_decay`` (default None: off; a number in (0, 1), else ``ValueError``) keeps an exponential moving average of the
    parameters inside the optimiser sweep: ``averaged_parameters()`` evaluates with it, ``averaged_state_dict()`` returns it,
    ``fit`` evaluates and snapshots it unless ``model.ema_eval = False``.  ``optim_alg='adamw'`` is Adam with decoupled weight
    decay (``torch.optim.AdamW``).  Both are labelled extensions.
    ``x_transform`` (default None | 'log1p' | 'log1p_norm') and ``library_size`` (default False) are the raw-count inputs of the count decoders
    (``type_rec='poisson'`` / ``'nb'`` / ``'zinb'``; anything else, or another ``x_transform``, raises ``ValueError``; x >= 0, checked once
    per dataset by ``fit`` / ``DeviceBatcher.bind``): the encoder reads log1p(x) (``'log1p_norm'``: the depth-normalised
    log1p(x / s), s the row's own size factor below) while the likelihood keeps the raw counts
    without training noise, and every decoder mean of a row is multiplied by the row's observed size factor
    max(sum_g x_g, 1) / dim_x.  Attributes until the engine is built, like the schedules.  Labelled extensions.
    ``dispersion`` (default 'gene-cell' | 'gene'; ``type_rec='nb'`` / ``'zinb'`` only, anything else raises ``ValueError``): 'gene' replaces the
    theta head by ONE inverse dispersion per gene, the parameter ``decoder_x.decoder_t.raw_theta`` (theta = softplus + 1e-3, started at
    0); ``px1`` / ``px2`` keep their shape, theta expanded to (rows, dim_x).  'gene-batch' (``use_s=True`` only, else
    ``ValueError``): one inverse dispersion per (gene, nuisance class) -- the same parameter as a (dim_s, dim_x) table, a row of class k
    reads row k (the x2 rows of a pair: the class of their batch row).  Labelled extension.
    ``eval_chunk_rows`` (default None; an integer >= 1, also a plain attribute): ``evaluate_performance_on_dataset`` -- and so ``fit`` --
    evaluates a device-resident set in row chunks of at most so many rows: the whole set's numbers in device memory that
    holds ``eval_chunk_rows`` x dim_x buffers and per-row arrays only; a ``CsrRows`` set is never densified beyond a chunk.
    ``use_MMD`` models and data parallelism raise ``NotImplementedError``, anything but None or such an integer ``ValueError``."""
    kind = 'pvae'
    prior_y = None          # read by the reference ctor (src/PVAE.py:77) although PVAE has no y

    def __init__(self, dim_x, dim_s, dim_y, dim_c=1, dim_m=1, dim_h_en_z1=(50, 50), dim_h_en_z2Fz1=(50),
                 dim_h_de_x=(50, 50), dim_z1=50, type_rec='binary', epochs=500, batch_size=100,
                 nonlinearity='softplus', learning_rate=0.001, optim_alg='adam', L=1, weight_decay=None,
                 dropout_rate=0., input_x_dropout=0., add_noise_var=0., use_MMD=True, kernel_MMD='rbf_fourier',
                 mmd_rate=1., kl_qz2pz2_rate=1., pertloss_rate=0.1, anneal_perturb_rate_itermax=1,
                 anneal_perturb_rate_offset=0, use_s=False, use_c=False, use_m=False, random_seed=12345,
                 log_txt=None, weight_norm=False, device=None, matmul_precision='fp32',
                 max_grad_norm=None, anneal_kl=False, anneal_kl_itermax=100, anneal_yloss=False, anneal_yloss_itermax=1,
                 anneal_learning_rate=False, anneal_lr_itermax=3000, ema_decay=None,
                 x_transform=None, library_size=False, dispersion='gene-cell', eval_chunk_rows=None):
        super().__init__()
        args = dict(locals())
        args.pop('self')
        args.pop('__class__', None)
        self._init_common(args)

    def loss_function(self, x1, x2, s, has_x2, noise=None):
        self._warn_empty_groups(has_x2, has_x2 * 0)
        return super().loss_function(noise=noise, x1=x1, x2=x2, s=s, has_x2=has_x2)

    def evaluate_performance(self, x1, x2, s, has_x2, return_full_data=False):
        """(perf dict, summary string) of src/PVAE.py:479-552"""
        return self._evaluate(x1, x2, s, None, has_x2, None, return_full_data)
