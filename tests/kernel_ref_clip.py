"""Plain-PyTorch stand-ins of the launchers gradient-norm clipping adds to the fused step (``drvae_amd.kernels.clip_norm`` /
``adam_l2_clip`` / ``adamax_l2_clip``): same names, same signatures, same output tensors -- the companion of
``tests/kernel_ref.py`` for these, test-only, CPU or GPU tensors.  The clip state is the int32 buffer of
``kernels.clip_state``: word 0 the step, words 2-3 max_norm (a double), words 4-7 the record {norm, coef (fp32 bits), skip,
n_skipped}, then the workspace (``sumsq_partials``, the helpers that build and view the state are plain torch and are used as
they are)."""
import math

import numpy as np
import torch

from tests import kernel_ref

CALLS = {'clip_norm': 0, 'adam_l2_clip': 0, 'adamax_l2_clip': 0}


def clip_norm(g, state, *, gscale=1.0):
    """the whole double sum goes into the first partial (one per 8192-element share would do), the partials are summed in
    index order, the record is written"""
    import drvae_amd.kernels as K
    CALLS['clip_norm'] += 1
    part, record = K.clip_partials(state), K.clip_record(state)
    n_part = K.sumsq_partials(g.numel())
    assert part.numel() >= n_part
    max_norm = float(state[K._CLIP_MAX_NORM:K._CLIP_MAX_NORM + 2].view(torch.float64)[0])
    assert max_norm > 0
    part.zero_()
    part[0] = (g.reshape(-1).double() ** 2).sum()
    s = 0.0
    for v in part[:n_part].tolist():        # index order
        s = s + v
    skip = not math.isfinite(s)
    norm = abs(float(np.float32(gscale))) * math.sqrt(s) if s == s else float('nan')
    coef = 0.0 if skip else min(1.0, max_norm / (norm + 1e-6))
    f = record.view(torch.float32)
    f[0], f[1] = float(np.float32(norm)), float(np.float32(coef))
    record[2] = int(skip)
    record[3] += int(skip)


def _clipped(plain, name, p, g, m, v, state, kw):
    CALLS[name] += 1
    import drvae_amd.kernels as K
    clip, step_dev = K.clip_record(state), state[0:1]
    if int(clip[2]):
        return None                                 # skipped: nothing is touched, the corrections are not evaluated
    coef = np.float32(float(clip.view(torch.float32)[1]))
    kw = dict(kw, gscale=float(np.float32(kw.get('gscale', 1.0)) * coef))
    return plain(p, g, m, v, step_dev - int(clip[3]), **kw)


def adam_l2_clip(p, g, m, v, state, **kw):
    return _clipped(kernel_ref.adam_l2, 'adam_l2_clip', p, g, m, v, state, kw)


def adamax_l2_clip(p, g, m, u, state, **kw):
    return _clipped(kernel_ref.adamax_l2, 'adamax_l2_clip', p, g, m, u, state, kw)


FUNCTIONS = ['clip_norm', 'adam_l2_clip', 'adamax_l2_clip']


def install(monkeypatch):
    """``kernel_ref.install`` plus the launchers of this module, for one CPU test (pytest monkeypatch); resets the call counts"""
    import drvae_amd.kernels as K
    kernel_ref.install(monkeypatch)
    me = globals()
    for name in FUNCTIONS:
        monkeypatch.setattr(K, name, me[name])
    for name in CALLS:
        CALLS[name] = 0
