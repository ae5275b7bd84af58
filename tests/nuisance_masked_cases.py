"""Shared by the tests of the nuisance variable on sampler-mode device batches (tests/test_nuisance_sampler_cpu.py,
tests/test_gpu_nuisance_sampler.py): an fp64 numpy reference written from the specification of ``dv_mmd_masked_*`` in
include/drvae_hip.h, its translation to the structure tables of tests/nuisance_cases.py, and constructed epoch tables."""
import math

import numpy as np

from tests import nuisance_cases as NC

GROUPS = {'drvae': 4, 'pvae': 2, 'vfae': 2}


# ------------------------------------------------------------------------------------------- numpy reference
def batch_flags(hx, hy, table, b, B):
    """(hx, hy) of the batch's B rows as bool arrays; ``table`` None: the flags are batch-local; ``b`` = ctr - base, clamped"""
    if table is None:
        r = np.arange(B)
    else:
        r = np.asarray(table)[min(max(int(b), 0), len(table) - 1)]
    fx = np.zeros(B, bool) if hx is None else np.asarray(hx)[r] != 0
    fy = np.zeros(B, bool) if hy is None else np.asarray(hy)[r] != 0
    return fx, fy


def data_groups(model, fx, fy):
    """data group of every batch row, the reference's order"""
    if model == 'drvae':
        return np.where(fx, np.where(fy, 2, 3), np.where(fy, 0, 1))
    if model == 'pvae':
        return np.where(fx, 1, 0)
    return np.where(fy, 0, 1)


def lists(B, Np, L):
    """(first row of z, rows, is a z2 list) of every row list"""
    out = [(l * B, B, False) for l in range(L)]
    if Np:
        out += [(L * B + l * Np, Np, True) for l in range(L)]
    return out


def masked_ref(z, cls, fx, fy, model, Np, L, S, kind, w, fac, W=None, b=None, a=None, c=None):
    """fp64: dict(diff (T, D), m2 (T), value, dz like z, theta (K n_z, R) | None, cnt (n_lists G, S + 1), members: a list per
    term group) of the masked MMD penalty for ONE batch whose flags are ``fx`` / ``fy``"""
    z = np.asarray(z, np.float64)
    cls = np.asarray(cls)
    B, G, Kc = len(cls), GROUPS[model], (1 if S == 2 else S)
    n_z = L * (B + Np)
    assert z.shape[0] == n_z and Np <= B
    grp = data_groups(model, fx, fy)
    rff = kind == 'rbf_fourier'
    ls = lists(B, Np, L)
    T = len(ls) * G * Kc
    D = W.shape[2] if rff else z.shape[1]
    diff, m2 = np.zeros((T, D)), np.zeros(T)
    theta = np.zeros((Kc * n_z, D)) if rff else None
    cnt = np.zeros((len(ls) * G, S + 1), np.int32)
    dz, value, members = np.zeros_like(z), 0.0, []
    for q, (z0, n, is_z2) in enumerate(ls):
        for g in range(G):
            tg = q * G + g
            i = np.arange(n)
            mem = i[(grp[:n] == g) & (fx[:n] if is_z2 else np.ones(n, bool))]
            members.append(mem)
            cj, r = cls[mem], z0 + mem
            cnt[tg, :S] = np.bincount(cj[(cj >= 0) & (cj < S)], minlength=S)[:S]
            cnt[tg, S] = len(mem)
            for k in range(Kc):
                t = tg * Kc + k
                n0, n1 = int((cj == k).sum()), int((cj != k).sum())
                if n0 == 0 or n1 == 0:
                    continue
                u = np.where(cj == k, 1.0 / n0, -1.0 / n1)
                if rff:
                    th = a * (z[r] @ np.asarray(W[t], np.float64)) + 2 * math.pi * np.asarray(b[t], np.float64)
                    theta[k * n_z + r] = th
                    diff[t] = c * (u[:, None] * np.cos(th)).sum(0)
                else:
                    diff[t] = (u[:, None] * z[r]).sum(0)
                m2[t] = (diff[t] ** 2).sum()
                if m2[t] <= 0:
                    continue
                value += -w * math.sqrt(m2[t])
                coef = -fac * w / math.sqrt(m2[t])
                if rff:
                    Gm = -diff[t][None, :] * np.sin(th)
                    dz[r] += coef * c * a * u[:, None] * (Gm @ np.asarray(W[t], np.float64).T)
                else:
                    dz[r] += coef * u[:, None] * diff[t][None, :]
    return dict(diff=diff, m2=m2, value=value, dz=dz, theta=theta, cnt=cnt, members=members)


def as_structure(model, fx, fy, Np, L, z, W=None, b=None, S=2):
    """the same batch as a problem of ``nuisance_cases.mmd_ref``: the structure table ``term_groups`` builds from the batch's
    ACTUAL flags (pair slots numbered over the batch's pairs), the sample rows re-stacked for it, and W / b of its terms taken
    from the masked layout's slots.  -> (grp_ptr, rows, src, z, W, b)"""
    B, G, Kc = len(fx), GROUPS[model], (1 if S == 2 else S)
    hx = fx if model != 'vfae' else np.zeros(B, bool)
    hy = fy if model != 'pvae' else np.zeros(B, bool)
    ptr, rows, src, masks = NC.term_groups(model, hx, hy, L)
    pairs = np.nonzero(hx)[0]
    assert len(pairs) == 0 or pairs.max() < Np
    z = np.asarray(z)
    zc = np.concatenate([z[:L * B]] + [z[L * B + l * Np + pairs] for l in range(L)])
    # term group of the structure table -> term group of the masked layout
    tgs = []
    for g, m in enumerate(masks):
        if not m.any():
            continue
        for l in range(L):
            tgs.append(l * G + g)
            if hx[np.nonzero(m)[0][0]]:
                tgs.append((L + l) * G + g)
    assert len(tgs) == len(ptr) - 1
    sel = np.concatenate([np.arange(tg * Kc, (tg + 1) * Kc) for tg in tgs])
    return ptr, rows, src, zc, (None if W is None else np.asarray(W)[sel]), (None if b is None else np.asarray(b)[sel])


# --------------------------------------------------------------------------------------- constructed epoch tables
def model_groups(kind, big):
    """data group (of the MODEL ``kind``) of every dataset row"""
    hx = big['has_x2'].reshape(-1).astype(bool) if kind != 'vfae' else np.zeros(len(big['s'].reshape(-1)), bool)
    hy = big['has_y'].reshape(-1).astype(bool) if kind != 'pvae' else np.zeros(len(big['s'].reshape(-1)), bool)
    return data_groups(kind, hx, hy)


def varied_table(kind, big, dim_s, n_batches, batch=24, seed=0):
    """(n_batches, batch) dataset rows, constructed: the number of rows per data group differs from batch to batch, every
    (data group, class) cell of every batch holds a row, the rows of a batch are shuffled (members of a group are scattered)"""
    s, grp, G = big['s'].reshape(-1), model_groups(kind, big), GROUPS[kind]
    rs = np.random.RandomState(seed)
    extra = batch - G * dim_s
    assert extra >= n_batches
    nxt, tab = {}, np.zeros((n_batches, batch), np.int64)
    for b in range(n_batches):
        e = np.zeros(G, np.int64)
        e[0] = b
        rest = extra - b
        e[1:] = rest // (G - 1)
        e[G - 1] += rest - (rest // (G - 1)) * (G - 1)
        rows = []
        for g in range(G):
            ks = list(range(dim_s)) + [int(rs.randint(dim_s)) for _ in range(int(e[g]))]
            for k in ks:
                pool = np.nonzero((grp == g) & (s == k))[0]
                assert len(pool) >= 4, (kind, g, k)
                i = nxt.get((g, k), 0)
                nxt[(g, k)] = i + 1
                rows.append(pool[i % len(pool)])
        assert len(rows) == batch
        tab[b] = np.asarray(rows)[rs.permutation(batch)]
    return tab


def assert_cells_filled_and_counts_differ(kind, big, tab, dim_s):
    """every (data group, class) cell of every batch holds a row (so no group is one class only, no side of a term is empty:
    only then the host-list path and the device path define the same number) and no two batches have the same group counts"""
    s, grp, G = big['s'].reshape(-1), model_groups(kind, big), GROUPS[kind]
    seen = set()
    for b in range(tab.shape[0]):
        cells = np.zeros((G, dim_s), np.int64)
        np.add.at(cells, (grp[tab[b]], s[tab[b]]), 1)
        assert (cells > 0).all(), (b, cells)
        seen.add(tuple(cells.sum(1)))
    assert len(seen) == tab.shape[0], seen


# ------------------------------------------------------------------------------------------ the noise of a step
def step_noise(p, cfg, hy, y):
    """the N(0,1) draws sitting in the noise arena of the batch-independent plan ``p``, in the layout ``FusedStep.set_noise``
    takes (``oracle.models_ref.make_noise``): a second engine that runs the same batch on a plan of its own structure is
    handed the SAME draws -- its own would be other numbers for the labeled rows, whose one z3 draw sits in the slot of
    their class on this plan and in slot 0 on a structure plan.  ``hy`` / ``y``: the batch's label flags and labels."""
    L, B, Np = cfg.L, p.B, p.Np
    n = lambda t: t.detach().cpu().numpy().astype(np.float32)
    X, Z1 = p.EX.shape[1], p.E1.shape[1]
    out = dict(nx1=n(p.EX[:B]), nx2=np.zeros((B, X), np.float32), ez1=n(p.E1).reshape(L, B, Z1),
               ez2=np.zeros((L, B, Z1), np.float32))
    if Np:
        out['nx2'][:Np] = n(p.EX[B:])
        out['ez2'][:, :Np] = n(p.E2).reshape(L, Np, Z1)
    if cfg.has_pert:
        out['ez2F'] = n(p.E2F).reshape(L, B, Z1)
    if cfg.has_y and p.Mf:
        hy, y = np.asarray(hy).astype(bool).reshape(-1), np.asarray(y).astype(np.int64).reshape(-1)
        E3 = n(p.E3)
        ez3 = np.zeros((L, cfg.dim_y, B, E3.shape[1]), np.float32)
        l, i, slot = p.fp_l_host, p.fp_i_host, p.fp_slot_host
        one = p._has_y_host.astype(bool)[i]                  # rows the plan itself holds as labeled: one fprop row
        lab = hy[i]
        keep = ~lab | one | (slot == y[i])                   # a labeled row: the draw of its class slot, to slot 0
        dst = np.where(lab, 0, slot)
        ez3[l[keep], dst[keep], i[keep]] = E3[keep]
        out['ez3'] = ez3
    return out
