"""Plain-PyTorch fp32 stand-ins of ``drvae_amd.kernels.mmd_masked_fwd`` / ``mmd_masked_bwd`` (the MMD penalty of a
batch-independent plan: data groups and classes read as data): same names, same operands by name, same output tensors --
the companion of ``tests/kernel_ref_nuisance.py`` for these two, test-only, CPU or GPU tensors."""
import math

import torch

from tests import kernel_ref_nuisance as KN

_G = {'drvae': 4, 'pvae': 2, 'vfae': 2}


def _term_groups(g):
    """(tg, rows of z, batch rows) of every term group of this batch"""
    cls = g['cls']
    B, Np, L, model = cls.numel(), g['Np'], g['L'], g['model']
    table = g.get('table')
    if table is not None:
        b = min(max(int(g['ctr'][0]) - int(g['base'][0]), 0), g['n_batches'] - 1)
        r = table[b].long()
    else:
        r = torch.arange(B, device=cls.device)
    zero = torch.zeros(B, dtype=torch.bool, device=cls.device)
    hx = g['hx'][r] != 0 if g.get('hx') is not None else zero
    hy = g['hy'][r] != 0 if g.get('hy') is not None else zero
    if model == 'drvae':
        grp = torch.where(hx, torch.where(hy, 2, 3), torch.where(hy, 0, 1))
    elif model == 'pvae':
        grp = hx.long()
    else:
        grp = 1 - hy.long()
    G = _G[model]
    lists = [(l * B, B, False) for l in range(L)] + ([(L * B + l * Np, Np, True) for l in range(L)] if Np else [])
    for q, (z0, n, z2) in enumerate(lists):
        for gi in range(G):
            m = grp[:n] == gi
            if z2:
                m = m & hx[:n]
            mem = torch.nonzero(m).reshape(-1)
            yield q * G + gi, z0 + mem, mem


def mmd_masked_fwd(g):
    z, rff, S = g['z'], g['kind'] == 'rbf_fourier', g['S']
    Kc, n_z = (1 if S == 2 else S), g['z'].shape[0]
    g['cnt'].zero_()
    for tg, rows, mem in _term_groups(g):
        c = g['cls'][mem]
        g['members'][tg, :mem.numel()] = mem.to(torch.int32)
        for k in range(S):
            g['cnt'][tg, k] = int((c == k).sum())
        g['cnt'][tg, S] = mem.numel()
        for k in range(Kc):
            t = tg * Kc + k
            n0 = int((c == k).sum())
            n1 = mem.numel() - n0
            if n0 == 0 or n1 == 0:
                g['diff'][t].zero_()
                continue
            u = torch.where(c == k, torch.full_like(c, 1, dtype=z.dtype) / n0, torch.full_like(c, -1, dtype=z.dtype) / n1)
            if rff:
                th = g['a'] * (z[rows] @ g['W'][t]) + 2 * math.pi * g['b'][t]
                g['theta'][k * n_z + rows] = th
                g['diff'][t] = g['c'] * (u[:, None] * torch.cos(th)).sum(0)
            else:
                g['diff'][t] = (u[:, None] * z[rows]).sum(0)


def mmd_masked_bwd(g):
    z, rff, S = g['z'], g['kind'] == 'rbf_fourier', g['S']
    Kc, n_z = (1 if S == 2 else S), g['z'].shape[0]
    dz = torch.zeros_like(g['dz'])
    val = z.new_zeros(())
    for tg, rows, mem in _term_groups(g):
        c = g['cls'][mem]
        for k in range(Kc):
            t = tg * Kc + k
            diff = g['diff'][t]
            m2 = (diff * diff).sum()
            g['m2'][t] = m2
            n0 = int((c == k).sum())
            n1 = mem.numel() - n0
            if float(m2) <= 0.0 or n0 == 0 or n1 == 0:
                continue
            val = val - g['w'] * torch.sqrt(m2)
            coef = -g['fac'] * g['w'] / torch.sqrt(m2)
            u = torch.where(c == k, torch.full_like(c, 1, dtype=z.dtype) / n0, torch.full_like(c, -1, dtype=z.dtype) / n1)
            if rff:
                th = g['theta'][k * n_z + rows]
                Gm = -diff[None, :] * torch.sin(th)
                dz[rows] += (coef * g['c'] * g['a']) * u[:, None] * (Gm @ g['W'][t].t())
            else:
                dz[rows] += coef * u[:, None] * diff[None, :]
    g['dz'].copy_(dz)
    g['value'].copy_(val.reshape(1))


FUNCTIONS = ['mmd_masked_fwd', 'mmd_masked_bwd']


def install(monkeypatch):
    """``kernel_ref_nuisance.install`` plus the two launchers of this module, for one CPU test (pytest monkeypatch)"""
    import drvae_amd.kernels as K
    KN.install(monkeypatch)
    me = globals()
    for name in FUNCTIONS:
        monkeypatch.setattr(K, name, me[name])
