"""Shared by the tests of the device-carried nuisance variable (tests/test_nuisance_cpu.py, tests/test_gpu_nuisance.py):
fp64 numpy references written from the formulas of include/drvae_hip.h (``dv_nuisance_feed``, ``dv_mmd_grouped_*``), and
the datasets / epoch tables the engine-level tests run on."""
import math

import numpy as np
import torch

from oracle import models_ref as M
from tests.golden import cases as C

GROUPS = ((1, 0), (0, 0), (1, 1), (0, 1))      # (has_y, has_x2): the batcher's order of data groups


# ------------------------------------------------------------------------------------------- numpy references
def feed_ref(s, table, b, pair_rows, B, L, S):
    """(sohe, sohd, cls) of batch ``b`` of ``table`` (None: ``s`` is the batch's own class vector)"""
    n_b = 1 if table is None else table.shape[0]
    b = min(max(b, 0), n_b - 1)
    c = np.asarray(s if table is None else s[table[b]], np.int64)
    cp = c[pair_rows] if len(pair_rows) else c[:0]
    eye = np.eye(S, dtype=np.float32)
    return eye[np.concatenate([c, cp])], eye[np.concatenate([np.tile(c, L), np.tile(cp, L), np.tile(cp, L)])], c.astype(np.int32)


def mmd_ref(z, cls, grp_ptr, rows, src, S, kind, w, fac, W=None, b=None, a=None, c=None):
    """fp64: (diff (T, D), m2 (T), value, dz like z, theta (K E, R) | None, cnt (n_groups, S)) of the grouped MMD penalty;
    an empty side or m2 == 0 gives value 0 and gradient 0 for that term"""
    z = np.asarray(z, np.float64)
    Kc = 1 if S == 2 else S
    n_groups, E = len(grp_ptr) - 1, int(grp_ptr[-1])
    rff = kind == 'rbf_fourier'
    D = W.shape[2] if rff else z.shape[1]
    diff, m2 = np.zeros((n_groups * Kc, D)), np.zeros(n_groups * Kc)
    theta = np.zeros((Kc * E, D)) if rff else None
    cnt = np.zeros((n_groups, S), np.int32)
    dz, value = np.zeros_like(z), 0.0
    for g in range(n_groups):
        e0, e1 = int(grp_ptr[g]), int(grp_ptr[g + 1])
        r, cj = np.asarray(rows[e0:e1]), np.asarray(cls)[np.asarray(src[e0:e1])]
        cnt[g] = np.bincount(cj, minlength=S)[:S]
        for k in range(Kc):
            t = g * Kc + k
            n0, n1 = int((cj == k).sum()), int((cj != k).sum())
            if n0 == 0 or n1 == 0:
                continue
            u = np.where(cj == k, 1.0 / n0, -1.0 / n1)
            if rff:
                th = a * (z[r] @ np.asarray(W[t], np.float64)) + 2 * math.pi * np.asarray(b[t], np.float64)
                theta[k * E + e0:k * E + e1] = th
                diff[t] = c * (u[:, None] * np.cos(th)).sum(0)
            else:
                diff[t] = (u[:, None] * z[r]).sum(0)
            m2[t] = (diff[t] ** 2).sum()
            if m2[t] <= 0:
                continue
            value += -w * math.sqrt(m2[t])
            coef = -fac * w / math.sqrt(m2[t])            # d(fac * -w sqrt(m2)) / d diff = coef * diff
            if rff:
                G = -diff[t][None, :] * np.sin(th)
                dz[r] += coef * c * a * u[:, None] * (G @ np.asarray(W[t], np.float64).T)
            else:
                dz[r] += coef * u[:, None] * diff[t][None, :]
    return diff, m2, value, dz, theta, cnt


def term_groups(kind, has_x2, has_y, L):
    """(grp_ptr, rows, src) of a batch structure, written from the reference's definition of the penalty (per data
    group and Monte-Carlo sample, on z1 and -- groups of pairs -- z2; src/DrVAE.py:537-540,585-608)"""
    hx, hy = np.asarray(has_x2).astype(bool).reshape(-1), np.asarray(has_y).astype(bool).reshape(-1)
    if kind == 'vfae':
        hx = np.zeros_like(hx)
    if kind == 'pvae':
        hy = np.zeros_like(hy)
    B = len(hx)
    pairs = np.nonzero(hx)[0]
    Np = len(pairs)
    slot = np.full(B, -1)
    slot[pairs] = np.arange(Np)
    masks = {'drvae': [hy & ~hx, ~hy & ~hx, hy & hx, ~hy & hx], 'pvae': [~hx, hx], 'vfae': [hy, ~hy]}[kind]
    ptr, rows, src = [0], [], []
    for m in masks:
        idx = np.nonzero(m)[0]
        if not len(idx):
            continue
        for l in range(L):
            lists = [l * B + idx]
            if hx[idx[0]]:
                lists.append(L * B + l * Np + slot[idx])
            for r in lists:
                rows.append(r)
                src.append(idx)
                ptr.append(ptr[-1] + len(idx))
    return np.asarray(ptr), np.concatenate(rows), np.concatenate(src), masks


# --------------------------------------------------------------------------------------- engine-level fixtures
def dataset(kind, dim_s, dev, n=400, **over):
    """the neighbouring tests' fixture: 400 rows, every class in every data group at least 24 times"""
    from drvae_amd import data as D
    spec = C.tiny_spec(kind, use_s=True, dim_s=dim_s, **over)
    big = M.make_batch(spec, n, seed=9)
    t = lambda k: torch.from_numpy(big[k].copy())
    ds = D.DrVAEDataset(t('x1'), t('x2'), t('s'), t('y'), t('has_x2'), t('has_y')).to(dev)
    return spec, big, ds


def group_counts(big, batch=24):
    """rows per data group of a batch: the same number from every group the dataset has rows of (4 groups: 6 each)"""
    hy, hx = big['has_y'].reshape(-1).astype(bool), big['has_x2'].reshape(-1).astype(bool)
    have = [bool(((hy == bool(gy)) & (hx == bool(gx))).any()) for gy, gx in GROUPS]
    assert batch % sum(have) == 0
    return [batch // sum(have) if h else 0 for h in have]


def epoch_table(big, dim_s, n_batches, batch=24, vary=False, seed=0):
    """(n_batches, batch) dataset rows, the batcher's group order; inside every group the classes go round-robin
    (``vary``: only the first dim_s slots do, the others are drawn -- another composition in every batch)"""
    s = big['s'].reshape(-1)
    hy, hx = big['has_y'].reshape(-1).astype(bool), big['has_x2'].reshape(-1).astype(bool)
    rs = np.random.RandomState(seed)
    nxt = {}
    counts = group_counts(big, batch)
    tab = np.zeros((n_batches, batch), np.int64)
    for b in range(n_batches):
        col = 0
        for gi, (gy, gx) in enumerate(GROUPS):
            for j in range(counts[gi]):
                k = (j + b) % dim_s if (not vary or j < dim_s) else int(rs.randint(dim_s))
                pool = np.nonzero((hy == bool(gy)) & (hx == bool(gx)) & (s == k))[0]
                assert len(pool) >= 6
                i = nxt.get((gi, k), 0)
                nxt[(gi, k)] = i + 1
                tab[b, col] = pool[i % len(pool)]
                col += 1
    return tab


def assert_every_side_filled(kind, big, tab, dim_s, has_x2, has_y):
    """every (data group, class) side of every batch holds a row: only then the host-list path and the device path
    define the same number"""
    s = big['s'].reshape(-1)
    masks = term_groups(kind, has_x2, has_y, 1)[3]
    for b in range(tab.shape[0]):
        sb = s[tab[b]]
        for m in masks:
            if m.any():
                cnt = np.bincount(sb[m], minlength=dim_s)
                assert (cnt > 0).all() and (cnt < m.sum()).all(), (b, cnt)
