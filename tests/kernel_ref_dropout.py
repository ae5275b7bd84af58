"""Plain-PyTorch stand-ins of the two launchers hidden-layer dropout adds to the fused step
(``drvae_amd.kernels.fill_noise_rows`` / ``mask_scale``): same names, same signatures, same output tensors -- the companion
of ``tests/kernel_ref.py`` for these, test-only, CPU or GPU tensors.  The keep rows come from ``tests/philox_ref.py``
(integer Philox words against the threshold: no float uniform, so a conforming kernel writes exactly these masks)."""
import numpy as np
import torch

from tests import kernel_ref, philox_ref

CALLS = {'fill_noise_rows': 0, 'mask_scale': 0}


def keep_rows(desc, keep_thr, seed, event):
    """(offsets, mask) flat over every element the KEEP rows ``desc`` (n x {offset, width, draw id, global row}) describe:
    mask = 1.0 where word col % 4 of Philox4x32-10(counter = (col // 4, global row, draw id, event_lo),
    key = (seed_lo, seed_hi ^ event_hi)) is < keep_thr, else 0.0"""
    desc = np.asarray(desc, dtype=np.int64).reshape(-1, 4)
    s_lo, s_hi = philox_ref._split(seed)
    e_lo, e_hi = philox_ref._split(event)
    offs, vals = [], []
    for w in np.unique(desc[:, 1]):
        if w <= 0:
            continue
        d = desc[desc[:, 1] == w]
        blk = np.arange((int(w) + 3) // 4, dtype=np.uint64).reshape(1, -1)
        words = philox_ref.philox4x32_10(blk, d[:, 3].reshape(-1, 1), d[:, 2].reshape(-1, 1), e_lo, s_lo, s_hi ^ e_hi)
        words = np.stack(words, -1).reshape(len(d), -1)[:, :int(w)]              # (rows, width): word col % 4 of block col // 4
        offs.append((d[:, 0][:, None] + np.arange(int(w))[None, :]).reshape(-1))
        vals.append((words.astype(np.uint64) < np.uint64(keep_thr)).astype(np.float32).reshape(-1))
    if not offs:
        return np.zeros(0, np.int64), np.zeros(0, np.float32)
    return np.concatenate(offs), np.concatenate(vals)


def fill_noise_rows(arena, table, seed, ctr_dev=None, park=None):
    """dv_fill_noise_rows as specified: ``table`` = descriptor rows + the trailer row {number of keep
    rows at the end, keep_thr's bits, 0, 0}; the rows in front as ``kernel_ref.fill_normal_rows``, the rest keep masks"""
    CALLS['fill_noise_rows'] += 1
    desc, tr = table[:-1], table[-1].tolist()
    n_normal, keep_thr = desc.shape[0] - tr[0], tr[1] & 0xFFFFFFFF
    assert 0 <= n_normal <= desc.shape[0] and tr[2] == tr[3] == 0
    if park is not None:
        kernel_ref.flag_wait(*park)
    d = desc.cpu().numpy()
    if n_normal:
        kernel_ref.fill_normal_rows(arena, desc[:n_normal], seed, ctr_dev)
    offs, vals = keep_rows(d[n_normal:], keep_thr, seed, kernel_ref._event(ctr_dev))
    arena.view(-1)[torch.from_numpy(offs).to(arena.device)] = torch.from_numpy(vals).to(arena.device)


def mask_scale(y, x, mask, scale):
    """dv_mask_scale: y = x * mask * scale in fp32, in that order (y may be x)"""
    CALLS['mask_scale'] += 1
    y.copy_(x * mask * torch.tensor(scale, dtype=x.dtype, device=x.device))


FUNCTIONS = ['fill_noise_rows', 'mask_scale']


def install(monkeypatch):
    """``kernel_ref.install`` plus the launchers of this module, for one CPU test (pytest monkeypatch); resets the call counts"""
    import drvae_amd.kernels as K
    kernel_ref.install(monkeypatch)
    me = globals()
    for name in FUNCTIONS:
        monkeypatch.setattr(K, name, me[name])
        CALLS[name] = 0
