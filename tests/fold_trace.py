"""Helpers of ``tests/test_fold_rows_cpu.py``: the dual-graph train step on CPU stand-ins, recorded launch by launch with
its arguments (``trace``), and RUN -- both chains issued the way ``capture()`` issues them, their launches held back and then
executed in an order the device flags allow (a launch that waits runs once the other chain has published), so the values a
step leaves are those of a replay.  Also writes the golden trace ``tests/golden/fold_rows_trace.json`` (``python -m
tests.fold_trace``): the recorded default step of the commit in front of ``Tail.fold_rows``, which the unfolded forms must
keep argument for argument."""
import functools
import json
import os

import torch

from oracle import models_ref as M
from tests import kernel_ref
from tests.golden import cases as C

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'fold_rows_trace.json')
HELPERS = ('smalln_ws_numel', 'col_moment_blocks', 'nll_raw_cs_shape', 'heads_tiles')      # no launch: answered at once
CASES = (('tiny_drvae', False), ('tiny_drvae', True), ('tiny_drvae_prior', False), ('tiny_vfae', False))


def _owner(eng, t):
    if t.numel() == 0:
        return 'empty'
    ptr = t.untyped_storage().data_ptr()
    for scope, obj in (('plan', eng.plan), ('eng', eng), ('arena', eng.arena)):
        for k in sorted(vars(obj)):
            v = vars(obj)[k]
            if torch.is_tensor(v) and v.numel() and v.untyped_storage().data_ptr() == ptr:
                return '%s.%s' % (scope, k)
    return 'other'


def describe(eng, a):
    """an argument as plain data: tensors by the buffer that owns them, their offset, shape and strides"""
    if torch.is_tensor(a):
        return [_owner(eng, a), a.storage_offset(), list(a.shape), list(a.stride())]
    if isinstance(a, dict):
        return {str(k): describe(eng, v) for k, v in sorted(a.items())}
    if isinstance(a, (list, tuple)):
        return [describe(eng, v) for v in a]
    if isinstance(a, float):
        return repr(float(a))
    if a is None or isinstance(a, (bool, int, str)):
        return a
    return type(a).__name__


class Deferred:
    """wraps every launcher of ``functions``: a call is noted (chain, name, arguments) and held back"""

    def __init__(self, eng, K, mp, functions):
        self.eng, self.chain = eng, None
        self.queue = {'main': [], 'side': []}
        self.trace = []
        for name in functions:
            fn = getattr(K, name)
            if name in HELPERS:
                continue
            mp.setattr(K, name, functools.partial(self._launch, name, fn))

    def _launch(self, name, fn, *a, **kw):
        self.trace.append([self.chain, name, describe(self.eng, a), describe(self.eng, kw)])
        self.queue[self.chain].append((name, fn, a, kw))

    @staticmethod
    def _waits(name, a, kw):
        """(flag, counter, add) of every wait that takes effect on the launch's entry"""
        w = []
        if name == 'flag_wait':
            w.append((a[0], a[1], kw.get('add', a[3] if len(a) > 3 else 1)))
        for k in ('park', 'after'):
            if kw.get(k) is not None:
                p = kw[k]
                w.append((p[0], p[1], p[3] if len(p) > 3 else 1))
        if kw.get('gate') is not None:
            w.append((kw['gate'][0], kw['gate'][1], kw['gate'][2]))
        return w

    def run(self):
        """execute what was held back; a launch whose wait is not met yields to the other chain"""
        order = []
        while self.queue['main'] or self.queue['side']:
            progress = False
            for chain in ('main', 'side'):
                q = self.queue[chain]
                while q and all(int(f[0]) >= int(c[0]) + add for f, c, add in self._waits(q[0][0], q[0][2], q[0][3])):
                    name, fn, a, kw = q.pop(0)
                    fn(*a, **kw)
                    order.append((chain, name))
                    progress = True
            assert progress, ('the two chains wait for each other', [q[0][0] for q in self.queue.values() if q])
        return order


def make(name, universal, install, mp, device='cpu'):
    """(engine, arena, case) of a small model case on the stand-ins ``install`` puts in place"""
    from tests.test_engine_cpu import make_engine, set_batch
    install(mp)
    case = C.model_case(name)
    spec = case['spec']
    eng, arena = make_engine(spec, M.init_params(spec, case['param_seed'], as_numpy=True), device)
    eng.universal = universal
    set_batch(eng, case['batch'], device)
    eng.training = True
    return eng, arena, case


def step(eng, tail, functions, run=True):
    """one dual-graph train step of ``tail``: both chains recorded (main with its optimiser launch, then side), then run.
    Returns the ``Deferred`` (its ``trace``; ``order``: the execution order)"""
    import drvae_amd.kernels as K
    import pytest
    eng.plan.set_beta(eng.beta_pert())
    if tail.noise_ahead and eng._noise_stale:        # (what ``replay`` does in front of the first step)
        eng._fill_noise(eng.plan)
        eng._noise_stale = False
    with pytest.MonkeyPatch.context() as inner:
        rec = Deferred(eng, K, inner, functions)
        with eng._recording('main', tail):
            rec.chain = 'main'
            eng._launch_sequence()
        with eng._recording('side', tail):
            rec.chain = 'side'
            eng._launch_sequence(draw=False, optimizer=False)
    rec.order = rec.run() if run else None
    eng.iters += 1
    return rec


def default_trace(name, universal):
    """the recorded (not run) dual-graph step of a case on the stand-ins, as ``DRVAE_TUNE`` has it"""
    import pytest
    import drvae_amd.tuning as T
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(T, '_VALUES', None)
        eng, _, case = make(name, universal, kernel_ref.install, mp)
        eng.set_noise(case['noises'][0])
        tail = eng._step_tail(False, on_gpu=True)
        assert tail.dual
        rec = step(eng, tail, kernel_ref.FUNCTIONS, run=False)
    return json.loads(json.dumps(rec.trace))


if __name__ == '__main__':
    os.environ['DRVAE_TUNE'] = 'fold_rows=0'        # the golden trace is the UNFOLDED step
    out = {'%s/%s' % (n, 'universal' if u else 'structure'): default_trace(n, u) for n, u in CASES}
    with open(GOLDEN, 'w') as f:
        json.dump(out, f, separators=(',', ':'), sort_keys=True)
    print('wrote', GOLDEN, os.path.getsize(GOLDEN), 'bytes')
