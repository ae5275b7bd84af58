"""Plain-PyTorch fp32 stand-ins of the launchers that carry the nuisance variable on the device
(``drvae_amd.kernels.nuisance_feed`` / ``mmd_grouped_fwd`` / ``mmd_grouped_bwd``): same names, same signatures, same output
tensors -- the companion of ``tests/kernel_ref.py`` for these three, test-only, CPU or GPU tensors."""
import math

import torch
import torch.nn.functional as F

from tests import kernel_ref


def nuisance_feed(sohe, sohd, cls, s32, *, table=None, n_batches=0, ctr=None, base=None, pair_rows=None, L=1):
    B, S = cls.numel(), sohe.shape[1]
    if table is not None:
        b = min(max(int(ctr[0]) - int(base[0]), 0), n_batches - 1)
        c = s32[table[b].long()]
    else:
        c = s32.reshape(-1)
    c = c.to(torch.int32)
    cp = c[pair_rows.long()] if (pair_rows is not None and pair_rows.numel()) else c[:0]
    cls.copy_(c)
    sohe.copy_(F.one_hot(torch.cat([c, cp]).long(), S).to(sohe.dtype))
    sohd.copy_(F.one_hot(torch.cat([c.repeat(L), cp.repeat(L), cp.repeat(L)]).long(), S).to(sohd.dtype))


def _terms(g):
    """(t, k, entries slice, rows of z, class of every entry, n0, n1) of every term"""
    S = g['S']
    Kc = 1 if S == 2 else S
    ptr = g['grp_ptr'].tolist()
    for tg in range(len(ptr) - 1):
        e = slice(ptr[tg], ptr[tg + 1])
        rows = g['rows'][e].long()
        c = g['cls'][g['src'][e].long()]
        for k in range(Kc):
            n0 = int((c == k).sum())
            yield tg * Kc + k, k, tg, e, rows, c, n0, (ptr[tg + 1] - ptr[tg]) - n0


def mmd_grouped_fwd(g):
    z, rff, E = g['z'], g['kind'] == 'rbf_fourier', g['rows'].numel()
    for t, k, tg, e, rows, c, n0, n1 in _terms(g):
        g['cnt'][tg, k] = n0
        if g['S'] == 2:
            g['cnt'][tg, 1] = n1
        if n0 == 0 or n1 == 0:
            g['diff'][t].zero_()
            if rff:
                g['theta'][k * E + e.start:k * E + e.stop].zero_()
            continue
        u = torch.where(c == k, torch.full_like(c, 1, dtype=z.dtype) / n0, torch.full_like(c, -1, dtype=z.dtype) / n1)
        if rff:
            th = g['a'] * (z[rows] @ g['W'][t]) + 2 * math.pi * g['b'][t]
            g['theta'][k * E + e.start:k * E + e.stop] = th
            g['diff'][t] = g['c'] * (u[:, None] * torch.cos(th)).sum(0)
        else:
            g['diff'][t] = (u[:, None] * z[rows]).sum(0)


def mmd_grouped_bwd(g):
    z, rff, E = g['z'], g['kind'] == 'rbf_fourier', g['rows'].numel()
    dz = torch.zeros_like(g['dz'])
    val = z.new_zeros(())
    for t, k, tg, e, rows, c, n0, n1 in _terms(g):
        diff = g['diff'][t]
        m2 = (diff * diff).sum()
        g['m2'][t] = m2
        if float(m2) <= 0.0 or n0 == 0 or n1 == 0:
            continue
        val = val - g['w'] * torch.sqrt(m2)
        coef = -g['fac'] * g['w'] / torch.sqrt(m2)
        u = torch.where(c == k, torch.full_like(c, 1, dtype=z.dtype) / n0, torch.full_like(c, -1, dtype=z.dtype) / n1)
        if rff:
            th = g['theta'][k * E + e.start:k * E + e.stop]
            G = -diff[None, :] * torch.sin(th)
            dz[rows] += (coef * g['c'] * g['a']) * u[:, None] * (G @ g['W'][t].t())
        else:
            dz[rows] += coef * u[:, None] * diff[None, :]
    g['dz'].copy_(dz)
    g['value'].copy_(val.reshape(1))


FUNCTIONS = ['nuisance_feed', 'mmd_grouped_fwd', 'mmd_grouped_bwd']


def install(monkeypatch):
    """``kernel_ref.install`` plus the three launchers of this module, for one CPU test (pytest monkeypatch)"""
    import drvae_amd.kernels as K
    kernel_ref.install(monkeypatch)
    me = globals()
    for name in FUNCTIONS:
        monkeypatch.setattr(K, name, me[name])
