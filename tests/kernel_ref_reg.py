"""numpy float64 restatement of ``dv_reg_metrics`` (include/drvae_hip.h): the regression metrics of a continuous target in
the kernel's TWO-PASS arithmetic -- the means first, then the centred sums -- with its defined edge cases.  The companion
of ``tests/kernel_ref.py`` for this entry point; test-only."""
import numpy as np


def reg_metrics(pred, y, sel=None, n=None):
    """-> float64 array [rmse, r2, pearr] over the rows ``sel`` (None: the first ``n`` rows, default all) x all columns of
    ``pred`` / ``y`` ((rows, Y) or (rows,)), flattened"""
    pred = np.asarray(pred, np.float64).reshape(len(pred), -1)
    y = np.asarray(y, np.float64).reshape(len(y), -1)
    if sel is not None:
        sel = np.asarray(sel, np.int64)
        pred, y = pred[sel], y[sel]
    elif n is not None:
        pred, y = pred[:n], y[:n]
    p, t = pred.reshape(-1), y.reshape(-1)
    nan = float('nan')
    if t.size == 0:
        return np.array([nan, nan, nan])
    my, mp = t.sum() / t.size, p.sum() / p.size          # pass 1
    d, yc, pc = t - p, t - my, p - mp                    # pass 2
    sse, syy, spp, syp = (d * d).sum(), (yc * yc).sum(), (pc * pc).sum(), (yc * pc).sum()
    den = np.sqrt(syy * spp)
    return np.array([np.sqrt(sse / t.size), 1.0 - sse / syy if syy > 0 else nan, syp / den if den > 0 else nan])

