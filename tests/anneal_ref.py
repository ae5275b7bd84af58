"""The float64 reference of the annealing schedules (src/DrVAE.py:549-562,619-622; src/DGMMixin.py:77-104): the four
coefficients of an iteration as python floats, the annealed ELBO / CMPL recombined from the differentiable pieces the oracle
returns, and a trainer that steps torch's optimiser at the annealed learning rate.  Test-only; imports the oracle and does not
edit it.

    it = number of finished training iterations at the start of the step
    beta_pert = coef(it, anneal_perturb_rate_itermax, anneal_perturb_rate_offset)     (1 when itermax <= 0)
    beta_kl   = coef(it, anneal_kl_itermax)                          if anneal_kl            else 1
    beta_yr   = coef(it, anneal_yloss_itermax, anneal_yloss_offset)  if anneal_yloss         else 1
    lr_scale  = max(0.01, 1 - coef(it, anneal_lr_itermax))           if anneal_learning_rate else 1
    ELBO = RECL + beta_pert pertloss_rate PERT - beta_kl KLD      (VFAE: RECL - beta_kl KLD)
    CMPL = -ELBO - beta_yr yloss_rate YL - mmd_rate MMD
"""
from collections import OrderedDict

import numpy as np

from oracle import blocks_ref as B
from oracle import models_ref as M

# the schedule's own settings and their defaults (the models' constructor arguments of the same names)
DEFAULTS = OrderedDict(anneal_kl=False, anneal_kl_itermax=100, anneal_yloss=False, anneal_yloss_itermax=1,
                       anneal_yloss_offset=0, anneal_learning_rate=False, anneal_lr_itermax=3000)
RECORD = ('beta_pert', 'beta_kl', 'beta_yr', 'lr_scale')


def settings(**kw):
    out = OrderedDict(DEFAULTS)
    assert set(kw) <= set(out), kw
    out.update(kw)
    return out


def coef(it, iter_max=1000, iter_offset=0):
    """src/DGMMixin.py:77-89, written out (``oracle.blocks_ref.anneal_coef`` is the same expression: asserted below)"""
    if it - iter_offset > 0:
        return min(1., 0.01 + (it - iter_offset) / (1. * iter_max))
    return 0.01


def coefficients(it, sched, pert_itermax=1, pert_offset=0):
    """OrderedDict(beta_pert, beta_kl, beta_yr, lr_scale) of iteration count ``it``, python floats (float64)"""
    out = OrderedDict()
    out['beta_pert'] = coef(it, pert_itermax, pert_offset) if pert_itermax > 0 else 1.
    out['beta_kl'] = coef(it, sched['anneal_kl_itermax']) if sched['anneal_kl'] else 1.
    out['beta_yr'] = coef(it, sched['anneal_yloss_itermax'], sched['anneal_yloss_offset']) if sched['anneal_yloss'] else 1.
    out['lr_scale'] = max(0.01, 1. - coef(it, sched['anneal_lr_itermax'])) if sched['anneal_learning_rate'] else 1.
    for args in ((it, 3, 2), (it, 100, 0)):
        assert coef(*args) == B.anneal_coef(*args)
    return out


def record32(it, sched, pert_itermax=1, pert_offset=0):
    """the device record of the step: np.float32 of every coefficient, ONE rounding each -- (4,) float32"""
    return np.array([np.float32(v) for v in coefficients(it, sched, pert_itermax, pert_offset).values()], np.float32)


def spec_coefficients(spec, it, sched):
    return coefficients(it, sched, spec.anneal_perturb_rate_itermax, spec.anneal_perturb_rate_offset)


def recombine(spec, sched, losses, it):
    """the oracle's losses with ELBO / CMPL replaced by the annealed combinations of its (unscaled, differentiable) pieces"""
    c = spec_coefficients(spec, it, sched)
    out = OrderedDict(losses)
    if spec.kind == 'vfae':
        out['ELBO'] = out['RECL'] - c['beta_kl'] * out['KLD']
    else:
        out['ELBO'] = out['RECL'] + c['beta_pert'] * spec.pertloss_rate * out['PERT'] - c['beta_kl'] * out['KLD']
    out['CMPL'] = -out['ELBO']
    if spec.kind != 'pvae':
        out['CMPL'] = out['CMPL'] - c['beta_yr'] * spec.yloss_rate * out['YL']
    if spec.use_s and spec.use_MMD:
        out['CMPL'] = out['CMPL'] - spec.mmd_rate * out['MMD']
    return out


def loss_function(spec, sched, params, batch, noise, iters=0, training=True, counts=None):
    losses, rows = M.loss_function(spec, params, batch, noise, iters, training, counts)
    return recombine(spec, sched, losses, iters), rows


class AnnealTrainer(M.RefTrainer):
    """``oracle.models_ref.RefTrainer`` with the schedules: the annealed CMPL is what is differentiated, and the optimiser's
    rate is set to lr_scale * learning_rate before each ``step()`` (the evident intent of src/DGMMixin.py:100-104)"""

    def __init__(self, spec, params, sched):
        super().__init__(spec, params)
        self.sched = sched

    def loss(self, batch, noise, training=True, counts=None):
        return loss_function(self.spec, self.sched, self.params, batch, noise, self.iters, training, counts)

    def step(self, batch, noise, counts=None):
        self.opt.zero_grad()
        losses, rows = self.loss(batch, noise, True, counts)
        losses['CMPL'].backward()
        self.opt.param_groups[0]['lr'] = spec_coefficients(self.spec, self.iters, self.sched)['lr_scale'] * self.spec.learning_rate
        self.opt.step()
        self.iters += 1
        return losses, rows


# ---------------------------------------------------------------------------------------------------- the test model
def small_spec(kind, **over):
    """the smallest shapes that exercise every group: 24 genes, 4 latent dimensions, one hidden layer of 16, 3 classes, L = 2"""
    kw = dict(kind=kind, dim_x=24, dim_y=3, dim_z1=4, dim_z3=4, h_en_z1=[16], h_de_z1=[16], h_en_z3=[16], h_de_x=[16],
              h_clf=[], L=2, learning_rate=5e-3, weight_decay=0.01)
    kw.update(over)
    return M.ModelSpec(**kw)


def small_batch(spec, n=12, seed=3):
    """``n`` rows in the oracle's group rotation: all four DrVAE data groups (PVAE / VFAE: both of theirs) are present"""
    batch = M.make_batch(spec, n, seed=seed)
    if spec.kind == 'drvae':
        hy, hx = batch['has_y'].astype(bool), batch['has_x2'].astype(bool)
        assert all(m.any() for m in (hy & ~hx, ~hy & ~hx, hy & hx, ~hy & hx))
    return batch
