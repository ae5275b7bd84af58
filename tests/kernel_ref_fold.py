"""Plain-PyTorch stand-ins of the two launchers in their FOLDED forms (``Tail.fold_rows``): ``z2f_post_bwd`` that forms the
pairs' KL rows itself and sums the fprop rows' d/dz1, ``smalln_fwd`` that also emits the classifier's data gradient.  Same
names, same signatures as ``drvae_amd.kernels``, written as the unfolded sequences of ``tests/kernel_ref.py`` they replace --
the companion of that file for these two, installed on top of it (as ``tests/kernel_ref_dropout.py`` is), test-only.  They
carry the ``fold_rows`` attribute ``schedule._step_tail`` looks for; the stand-ins of ``kernel_ref`` do not."""
import torch

from tests import kernel_ref

CALLS = {'z2f_post_bwd': 0, 'smalln_fwd': 0, 'folded_kl': 0, 'folded_dgrad': 0}


def pair_rows(pair_slot, L, B, Np):
    """p row l*B + i of every KL row l*Np + jp (pair_slot[i] == jp): the ``pidx`` of the separate launch"""
    slot = pair_slot.long()
    i_of = torch.empty(Np, dtype=torch.long, device=slot.device)
    i_of[slot[slot >= 0]] = torch.arange(B, device=slot.device)[slot >= 0]
    return (torch.arange(L, device=slot.device)[:, None] * B + i_of[None, :]).reshape(-1)


def z2f_post_bwd(dp2, dz1, dq2, dz2f, dzdec_pert, pair_slot, eps, p2, q2, coef, raw, kl_min, dz1b, L, B, Np,
                 park=None, prior=None, kl_out=None, seg=None, z1_dz2f=0.0):
    CALLS['z2f_post_bwd'] += 1
    if park is not None:
        kernel_ref.flag_wait(park[0], park[1], park[2], park[3] if len(park) > 3 else 1)
    Z = dp2.shape[1] // 2
    if kl_out is not None and Np:
        CALLS['folded_kl'] += 1
        kernel_ref.kl_rows_fwd(kl_out, raw, q2[:, :Z], q2[:, Z:2 * Z], p2[:, :Z], p2[:, Z:2 * Z],
                               pidx=pair_rows(pair_slot, L, B, Np), reps=L, free_bits=True, kl_min=kl_min)
    share = dz1b
    if seg is not None:
        s = torch.zeros(L * B, Z, device=dp2.device)
        kernel_ref.rows_segment_sum(s, seg[0], seg_ptr=seg[1], beta=0.0, width=Z)
        s = s * (seg[2] if len(seg) > 2 else 1.0)
        share = s if share is None else share + s
    if z1_dz2f != 0.0 and dz2f is not None:
        share = z1_dz2f * dz2f if share is None else share + z1_dz2f * dz2f
    kernel_ref.z2f_post_bwd(dp2, dz1, dq2, dz2f, dzdec_pert, pair_slot, eps, p2, q2, coef, raw, kl_min, share, L, B, Np,
                            prior=prior)


def smalln_fwd(probs, logits, a1, W, bias=None, a2=None, ymarg=None, park=None, fprop_kl=None, dgrad=None):
    CALLS['smalln_fwd'] += 1
    kernel_ref.smalln_fwd(probs, logits, a1, W, bias, a2, ymarg=ymarg, park=park, fprop_kl=fprop_kl)
    if dgrad:
        CALLS['folded_dgrad'] += 1
        assert ymarg is not None and len(dgrad) <= 2
        kernel_ref.smalln_bwd_data(list(dgrad), ymarg[3], probs, W)


z2f_post_bwd.fold_rows = True
smalln_fwd.fold_rows = True

FUNCTIONS = ['z2f_post_bwd', 'smalln_fwd']


def install(monkeypatch):
    """``kernel_ref.install`` plus the folded forms of this module, for one CPU test (pytest monkeypatch); resets the counts"""
    import drvae_amd.kernels as K
    kernel_ref.install(monkeypatch)
    me = globals()
    for name in FUNCTIONS:
        monkeypatch.setattr(K, name, me[name])
    for k in CALLS:
        CALLS[k] = 0
