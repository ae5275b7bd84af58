"""CPU: how a pass runs its decoder heads and its reconstruction rows is decided by ONE function
(``drvae_amd.schedule.heads_route``).  Checked on the recorded launcher calls (stand-in launchers of tests/kernel_ref.py): the
loss sums the buffer the pass's own row launch wrote, the heads' bias gradient is written exactly once, and every route of
the table is reached."""
import functools

import pytest
import torch

from oracle import models_ref as M
from tests import kernel_ref
from tests.golden import cases as C
from tests.test_engine_cpu import make_engine, set_batch

TUNINGS = ('', 'fuse_heads=0', 'fuse_heads=0,raw_heads=2,nll_cs=2')
SPECS = (dict(), dict(dim_x=16), dict(kind='vfae', dim_x=16), dict(type_rec='binary', add_noise_var=0.0))
N_ROWS = 12


class Calls:
    """what the row launches, ``loss_assemble``, ``colsum`` and the decoder heads' ``linear_bwd_pair`` of one pass were given"""

    def __init__(self, eng, K, mp):
        self.heads = eng.L_decx[-1]
        self.clear()
        for name in kernel_ref.FUNCTIONS:
            mp.setattr(K, name, functools.partial(self._launch, name, getattr(K, name)))

    def clear(self):
        self.events = []         # ('rows', route, out buffer) | ('loss', first term's tensor) | ('colsum',) | ('pair', dbias is None)

    def _launch(self, name, fn, *a, **kw):
        if name == 'linear_heads' and kw.get('nll') is not None:
            self.events.append(('rows', 'heads', kw['nll']['part']))
        elif name == 'rec_nll_rows':
            self.events.append(('rows', 'rec', a[0]))
        elif name == 'nll_rows_raw_cs':
            self.events.append(('rows', 'raw_cs_eval' if a[1] is None else 'raw_cs', a[0]))
        elif name == 'nll_rows_fwd':
            self.events.append(('rows', 'raw_eval' if kw.get('bias') is not None else 'fwd', a[0]))
        elif name == 'nll_rows_fwdbwd':
            self.events.append(('rows', 'fwdbwd+bias' if kw.get('bias') is not None else 'fwdbwd', a[0]))
        elif name == 'loss_assemble':
            self.events.append(('loss', a[1][0][0]))
        elif name == 'colsum' and a[0].data_ptr() == self.heads.db.data_ptr():
            self.events.append(('colsum',))
        elif name == 'linear_bwd_pair' and a[0].data_ptr() == self.heads.dW.data_ptr():
            self.events.append(('pair', a[1] is None))
        return fn(*a, **kw)


def _check_pass(calls, eng, kind, what):
    from drvae_amd.schedule import LOSS, heads_route
    route = heads_route(eng, eng.plan, kind)
    ev = calls.events
    loss_at = [i for i, e in enumerate(ev) if e[0] == 'loss']
    assert len(loss_at) == 1, what
    before = [e for e in ev[:loss_at[0]] if e[0] == 'rows']
    after = [e for e in ev[loss_at[0]:] if e[0] == 'rows']
    assert len(before) == 1, (what, 'row launches in front of the loss scalars', [e[1] for e in before])
    _, seen, out = before[0]
    assert seen.split('+')[0] == route.nll and (seen == 'fwdbwd+bias') == (route.nll == 'fwdbwd' and route.raw_last), (what, seen, route)
    # (a loss pass of a Bernoulli / Poisson decoder: its backward runs the row pass again, for the gradient, into the same rows)
    assert [(e[1], e[2].data_ptr()) for e in after] == ([('rec', out.data_ptr())] if (seen == 'rec' and kind == LOSS) else []), what
    # the loss sums what the pass wrote
    first = ev[loss_at[0]][1]
    assert first.untyped_storage().data_ptr() == out.untyped_storage().data_ptr(), (what, seen)
    assert out.data_ptr() == getattr(eng.plan, route.rows).data_ptr(), (what, seen, route.rows)
    # the heads' bias gradient: by the row pass's column sums or by the weight-gradient launch, never both, never neither
    pairs, colsums = [e[1] for e in ev if e[0] == 'pair'], [e for e in ev if e[0] == 'colsum']
    if pairs or colsums:
        assert len(pairs) == 1 and len(colsums) <= 1 and pairs[0] == bool(colsums), (what, pairs, len(colsums))
        assert pairs[0] == route.db_done
    return seen


def test_the_loss_sums_what_the_pass_wrote_and_the_heads_bias_gradient_is_written_once(monkeypatch):
    import drvae_amd.kernels as K
    import drvae_amd.tuning as T
    from drvae_amd.schedule import EVALUATE, LOSS, NLL_ROUTES, TRAIN
    kernel_ref.install(monkeypatch)
    seen = {}
    for tune in TUNINGS:
        monkeypatch.setenv('DRVAE_TUNE', tune)
        monkeypatch.setattr(T, '_VALUES', None)
        for over in SPECS:
            over = dict(over)
            spec = C.tiny_spec(over.pop('kind', 'drvae'), **over)
            eng, _ = make_engine(spec, M.init_params(spec, 9, as_numpy=True))
            set_batch(eng, M.make_batch(spec, N_ROWS, seed=3))
            noise = M.make_noise(spec, N_ROWS, seed=4)
            with pytest.MonkeyPatch.context() as inner:
                calls = Calls(eng, K, inner)
                what = (tune, over, 'train step')
                eng.train_step(noise)
                seen.setdefault(_check_pass(calls, eng, TRAIN, what), what)
                assert [e for e in calls.events if e[0] == 'pair'], what
                calls.clear()
                what = (tune, over, 'loss pass')
                eng.training = True
                eng.set_noise(noise)
                eng.forward()
                eng.backward()
                seen.setdefault(_check_pass(calls, eng, LOSS, what), what)
                assert [e[1] for e in calls.events if e[0] == 'pair'] == [False], what
                calls.clear()
                what = (tune, over, 'evaluation')
                eng.training = False
                eng.forward()
                seen.setdefault(_check_pass(calls, eng, EVALUATE, what), what)
                assert all(e[0] in ('rows', 'loss') for e in calls.events), what
    # every route of the table is reached (``fwdbwd`` with and without the bias): one that falls silent fails here
    assert set(seen) == set(NLL_ROUTES) | {'fwdbwd+bias'}, sorted(seen)


def test_chain_refuses_split_bf16_products_it_was_not_built_for(monkeypatch):
    """``x3=True`` on a chain ``use_x3_last`` has not accepted is an error, not a silent fp32 product"""
    import drvae_amd.tuning as T
    monkeypatch.setenv('DRVAE_TUNE', 'fuse_heads=0,raw_heads=2,nll_cs=2')
    monkeypatch.setattr(T, '_VALUES', None)
    kernel_ref.install(monkeypatch)
    spec = C.tiny_spec('drvae', dim_x=16)
    eng, _ = make_engine(spec, M.init_params(spec, 9, as_numpy=True))
    set_batch(eng, M.make_batch(spec, N_ROWS, seed=3))
    p = eng.plan
    assert p.c_decx.raw_softplus_ok() and not p.c_decx.x3_last
    p.c_decx.forward(p.dec_in, raw_last=True)
    with pytest.raises(AssertionError):
        p.c_decx.forward(p.dec_in, raw_last=True, x3=True)
    with pytest.raises(AssertionError):
        p.c_decx.backward(p.DPX, p.dec_in, [[(p.DZDEC, 1.0, 0.0)]], x3_last=True)
    assert torch.isfinite(p.c_decx.out[-1]).all()
