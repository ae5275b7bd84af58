#!/usr/bin/env python3
"""Whole-set evaluation of the regression head (``type_y='cont'``) and of a ``use_s`` model at cfg-2 sizes on an HBM-resident
8192-row set: the captured path (``evaluate_performance_on_dataset``: one graph replay + one copy) against the step-by-step
path ``model._evaluate`` on the same model and set, taken in alternation in one process (profiler off, shapes warmed up,
host clock around work that ends in a device synchronise -- both paths end in a device-to-host copy of their scalars).

``python tools/eval_variants_bench.py [reps] [--only cont|s] [--captured-only]`` (GPU box only; under
``rocprofv3 --kernel-trace --stats`` with ``--only ... --captured-only`` the kernel table says where the replay's time goes).
Prints a markdown table: median and spread (min, quartiles, max) of each path in ms."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drvae_amd import data as D, synth          # noqa: E402
from drvae_amd.DrVAE import DrVAE               # noqa: E402


def model_and_set(variant, n=8192, seed=1, dev='cuda'):
    kw = dict(type_y='cont', dim_y=1) if variant == 'cont' else dict(use_s=True, dim_s=3, dim_y=2)
    kw = dict(dict(dim_s=1, use_MMD=False), **kw)
    model = DrVAE(dim_x=978, dim_h_en_z1=[800], dim_h_de_z1=[200], dim_h_en_z3=[200], dim_h_de_x=[600], dim_h_clf=[], dim_z1=100,
                  dim_z3=100, type_rec='diag_gaussian', nonlinearity='elu', learning_rate=5e-4, L=2, weight_decay=0.05,
                  add_noise_var=0.01, pertloss_rate=0.05, random_seed=123, epochs=1, batch_size=150, **kw).to(dev)
    model.w2log = lambda *a: None
    b = synth.make_batch('drvae', n, 978, 2, seed=seed)
    rs = np.random.RandomState(seed + 7)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    if variant == 'cont':
        y = (0.5 + 0.3 * np.tanh(b['x1'][:, 0]) + 0.05 * rs.standard_normal(n)).clip(0.02, 0.98).astype(np.float32)
        s = np.zeros(n, np.int64)
    else:
        y, s = b['y'], rs.randint(0, 3, n)
    return model, D.DrVAEDataset(t(b['x1']), t(b['x2']), t(s), t(y), t(b['has_x2']), t(b['has_y']))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    reps = int(args[0]) if args else 200
    only = sys.argv[sys.argv.index('--only') + 1] if '--only' in sys.argv else None
    captured_only = '--captured-only' in sys.argv
    from drvae_amd import fit as F
    print('| variant | path | n | median ms | min | q25 | q75 | max | window s |')
    print('|---|---|---|---|---|---|---|---|---|')
    for variant in ('cont', 's'):
        if only not in (None, variant):
            continue
        model, ds = model_and_set(variant)
        g = lambda k: getattr(ds, k, None)
        captured = lambda: model.evaluate_performance_on_dataset(ds)
        stepwise = lambda: model._evaluate(g('x1'), g('x2'), g('s'), g('y'), g('has_x2'), g('has_y'))
        captured()                                   # capture
        assert F._EvalGraph.get(model, ds) is not None, 'the captured path was not taken'
        paths = [('captured', captured)] + ([] if captured_only else [('step by step', stepwise)])
        for _, fn in paths:                          # warm-up of every shape of both paths
            fn(), fn()
        ms = {name: [] for name, _ in paths}
        for _ in range(reps):                        # in alternation
            for name, fn in paths:
                ms[name].append(timed(fn))
        for name, _ in paths:
            v = np.asarray(ms[name])
            print('| drvae %s | %s | %d | %.3f | %.3f | %.3f | %.3f | %.3f | %.2f |'
                  % ("type_y='cont'" if variant == 'cont' else 'use_s, dim_s=3', name, len(v), np.median(v), v.min(),
                     np.percentile(v, 25), np.percentile(v, 75), v.max(), v.sum() / 1e3), flush=True)
        del model, ds
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
