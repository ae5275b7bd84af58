"""CPU: the device-flag hand-shake of the dual-graph train step, checked on the RECORDED launch sequence.  Both chains of
the step -- the main chain with its optimiser launch, then the side chain -- are issued on CPU tensors the way
``capture()`` issues them into their two graphs (stand-in launchers of tests/kernel_ref.py, a recorder around them), for
every small model case, every exchange form, a structure plan and a universal plan, with and without the explicit-batch tail
gate (``DRVAE_TUNE=tail_gate=2``).  The schedule recorded is the UNFOLDED one (``fold_rows=0``: the product's path under
clipping, dropout sites, the other models and every exchange form; the folded chains pass the same statements in
``tests/test_fold_rows_cpu.py``).  What is asserted comes from the trace and from the protocol table of
``drvae_amd/schedule.py`` (FLAGS / SITES) alone."""
import functools

import pytest
import torch

from oracle import models_ref as M
from tests import kernel_ref
from tests.golden import cases as C
from tests.test_engine_cpu import make_engine, set_batch

SPLITS = (False, True, 'captured', 'overlap')
OTHER = {'main': 'side', 'side': 'main'}
COUNTER = {'main': 'step_dev', 'side': 'side_ctr'}      # what each chain counts its steps in


class Recorder:
    """wraps every launcher: per launch the waits and publishes that take effect on its ENTRY (as (chain, launcher, flag
    name, value relative to the step's first launch[, site name])) and the counter bumps that follow them"""

    def __init__(self, eng, K, mp):
        self.eng, self.K = eng, K
        self.chain = None
        self.offset = {}                 # counter name -> bumps so far in the chain being recorded
        self.waits, self.pubs, self.launches = [], [], []
        self.loss_terms = []             # per ``loss_assemble`` launch: (chain, the plan attribute each term's first tensor is)
        for name in kernel_ref.FUNCTIONS:
            mp.setattr(K, name, functools.partial(self._launch, name, getattr(K, name)))

    def begin(self, chain):
        self.chain, self.offset = chain, {'step_dev': 0, 'side_ctr': 0, 'side_t': 0, 'rng_ctr': 0}

    def _counter(self, t):
        for name in self.offset:
            c = getattr(self.eng, name)
            if t.data_ptr() == c.data_ptr() and t.numel() == c.numel():
                return name
        raise AssertionError('a counter that is none of the engine\'s')

    def _word(self, t, buf, width):
        assert t.untyped_storage().data_ptr() == buf.untyped_storage().data_ptr() and t.numel() == width, \
            'not a %d-word view of the engine\'s buffer' % width
        assert t.storage_offset() % width == 0
        return t.storage_offset() // width

    def _value(self, ctr, add):
        name = self._counter(ctr)
        assert name == COUNTER[self.chain], 'the %s chain counts in %s, not in %s' % (self.chain, COUNTER[self.chain], name)
        return self.offset[name] + add

    def _wait(self, launcher, flag, ctr, err, add=1, max_spins=None):
        from drvae_amd.schedule import FLAGS, SITES
        self.waits.append((self.chain, launcher, FLAGS[self._word(flag, self.eng.flags, 1)][0], self._value(ctr, add),
                           SITES[self._word(err, self.eng.sync_err, 2)][0]))

    def _publish(self, launcher, flag, ctr, add=1):
        from drvae_amd.schedule import FLAGS
        self.pubs.append((self.chain, launcher, FLAGS[self._word(flag, self.eng.flags, 1)][0], self._value(ctr, add)))

    def _plan_attr(self, t):
        names = [k for k, v in vars(self.eng.plan).items() if torch.is_tensor(v) and v.numel()
                 and v.untyped_storage().data_ptr() == t.untyped_storage().data_ptr()]
        assert len(names) == 1, ('a loss term that is not one buffer of the plan', names)
        return names[0]

    def _launch(self, name, fn, *a, **kw):
        self.launches.append((self.chain, name))
        if name == 'loss_assemble':
            self.loss_terms.append((self.chain, tuple(self._plan_attr(term[0]) for term in a[1])))
        bumps = list(kw.get('bump') or ())
        if name == 'flag_publish':
            self._publish(name, *a)
        if kw.get('publish') is not None:
            self._publish(name, *kw['publish'])
        if name == 'flag_wait':
            self._wait(name, *a, **{k: kw[k] for k in ('add', 'max_spins') if k in kw})
        for k in ('park', 'after'):
            if kw.get(k) is not None:
                self._wait(name, *kw[k])
        if kw.get('gate') is not None:
            flag, ctr, add, err, lo, hi = kw['gate']
            assert 0 <= lo < hi <= a[0].numel(), 'the gated slice lies outside the sweep'
            self._wait(name, flag, ctr, err, add)
        if name == 'counter_add':
            bumps.append((a[0], a[1] if len(a) > 1 else kw.get('inc', 1)))
        if name == 'counters_add2':
            bumps += [(a[0], a[1]), (a[2], a[3])]
        for ctr, inc in bumps:           # (the counters move at the END of a launch: behind its publish and its wait)
            self.offset[self._counter(ctr)] += inc
        return fn(*a, **kw)


def record_side_alone(spec, params, batch, noise, universal, split, mp):
    """the side chain of the dual-graph step recorded on a FRESH engine, nothing issued in front of it"""
    import drvae_amd.kernels as K
    eng, _ = make_engine(spec, params)
    eng.universal = universal
    set_batch(eng, batch)
    eng.set_noise(noise)
    tail = eng._step_tail(split, on_gpu=True)
    assert tail.dual
    rec = Recorder(eng, K, mp)
    with eng._recording('side', tail):
        rec.begin('side')
        eng._launch_sequence(draw=False, optimizer=False)
    return rec


@functools.lru_cache(maxsize=None)
def recorded_steps(tail_gate):
    """{(case name, universal plan?, exchange form): Recorder} for every combination ``capture()`` records as two graphs"""
    import drvae_amd.kernels as K
    import drvae_amd.tuning as T
    out = {}
    with pytest.MonkeyPatch.context() as mp:
        kernel_ref.install(mp)
        mp.setenv('DRVAE_TUNE', 'fold_rows=0,tail_gate=2' if tail_gate else 'fold_rows=0')
        mp.setattr(T, '_VALUES', None)       # (re-read the switches now, and again after this block)
        for name in C.SMALL_MODEL_CASES:
            case = C.model_case(name)
            spec = case['spec']
            for universal in (False, True):
                for split in SPLITS:
                    with pytest.MonkeyPatch.context() as inner:
                        eng, _ = make_engine(spec, M.init_params(spec, case['param_seed'], as_numpy=True))
                        if universal and not eng.universal_ok():
                            continue
                        eng.universal = universal
                        set_batch(eng, case['batch'])
                        eng.set_noise(case['noises'][0])
                        tail = eng._step_tail(split, on_gpu=True)
                        # (PVAE's side chain is the step's tail only: under a gradient exchange it stays one graph)
                        assert tail.dual == bool(eng.cfg.has_y or not split), (name, universal, split)
                        if not tail.dual:
                            continue
                        rec = Recorder(eng, K, inner)
                        with eng._recording('main', tail):
                            rec.begin('main')
                            eng._launch_sequence(allreduce=(lambda buf: None) if split == 'captured' else None)
                        with eng._recording('side', tail):
                            rec.begin('side')
                            eng._launch_sequence(draw=False, optimizer=False)
                        out[(name, universal, split)] = rec
    return out


def test_the_matrix_is_the_one_asked_for():
    from drvae_amd.schedule import FLAGS, SITES
    steps = recorded_steps(False)
    assert {k[0] for k in steps} == set(C.SMALL_MODEL_CASES)
    assert {k[2] for k in steps} == set(SPLITS) and {k[1] for k in steps} == {False, True}
    assert set(recorded_steps(True)) == set(steps)
    for rec in steps.values():
        assert rec.eng.flags.numel() == len(FLAGS) and rec.eng.sync_err.numel() == 2 * len(SITES)
        assert rec.eng.flags.dtype == rec.eng.sync_err.dtype == torch.int32
        assert {c for c, _ in rec.launches} == {'main', 'side'}
        assert ('main', 'adam_l2') in rec.launches or ('main', 'adamax_l2') in rec.launches, 'no optimiser launch recorded'


@pytest.mark.parametrize('tail_gate', [False, True])
def test_every_wait_meets_one_publish_of_the_other_chain_with_the_same_value(tail_gate):
    """1: flag and ``counter + add`` agree on both sides, each counter taken with the bumps that precede the launch in its
    own chain; the wait of site ``next_step`` is met by the PREVIOUS step's tail (counters one lower)"""
    for key, rec in recorded_steps(tail_gate).items():
        assert rec.waits, key
        for chain, launcher, flag, value, site in rec.waits:
            met = [p for p in rec.pubs if p[0] == OTHER[chain] and p[2] == flag]
            assert len(met) == 1, (key, chain, launcher, flag, site, met)
            assert met[0][3] - (1 if site == 'next_step' else 0) == value, (key, chain, launcher, flag, site, value, met)


@pytest.mark.parametrize('tail_gate', [False, True])
def test_every_wait_reports_into_the_error_slot_of_its_own_site(tail_gate):
    """2 (the slots of two sites are disjoint by ``Recorder._word``: whole (error, ticks) pairs of ``sync_err``)"""
    from drvae_amd.schedule import SITES
    sites = {s[0]: s for s in SITES}
    assert len(sites) == len(SITES)
    for key, rec in recorded_steps(tail_gate).items():
        for chain, launcher, flag, value, site in rec.waits:
            assert sites[site][1] == chain and flag in sites[site][2], (key, chain, launcher, flag, site)


def test_the_sites_reached_are_the_table_s():
    from drvae_amd.schedule import SITES
    seen = {(w[4], w[2]) for tg in (False, True) for rec in recorded_steps(tg).values() for w in rec.waits}
    assert seen == {(s[0], f) for s in SITES for f in s[2]}
    # (the explicit-batch tail gate is what reaches the next step's wait and the classifier's flag)
    assert 'next_step' not in {w[4] for rec in recorded_steps(False).values() for w in rec.waits}


@pytest.mark.parametrize('tail_gate', [False, True])
def test_a_chain_publishes_only_its_own_flags(tail_gate):
    """3"""
    from drvae_amd.schedule import FLAGS
    owner = {f[0]: f[1] for f in FLAGS}
    assert set(owner.values()) == {'main', 'side', None} and owner['unused'] is None
    for key, rec in recorded_steps(tail_gate).items():
        for chain, launcher, flag, value in rec.pubs:
            assert owner[flag] == chain, (key, chain, launcher, flag)
        assert len({(p[0], p[2]) for p in rec.pubs}) == len(rec.pubs), (key, 'a flag published twice in one step', rec.pubs)


def test_flags_nobody_waits_for_are_the_ones_the_table_declares():
    """4: in every recorded step inside the declared set, over all of them exactly that set"""
    from drvae_amd.schedule import FLAGS
    declared = {f[0] for f in FLAGS if f[2]}
    seen = set()
    for tg in (False, True):
        for key, rec in recorded_steps(tg).items():
            idle = {p[2] for p in rec.pubs} - {w[2] for w in rec.waits}
            assert idle <= declared, (key, idle)
            if not rec.eng.cfg.has_y:        # (PVAE: published as part of the launch arguments, no fprop chain to wait)
                assert {'z1', 'z2f'} <= idle, (key, idle)
            seen |= idle
    assert seen == declared


def _side(rec):
    return [n for c, n in rec.launches if c == 'side'], [t for c, t in rec.loss_terms if c == 'side']


def test_the_side_chain_s_recording_does_not_depend_on_what_ran_before_it(monkeypatch):
    """which buffer the side chain's ``loss_assemble`` sums is decided by ``heads_route`` from the plan and the kind of pass,
    not left behind by the pass issued before it: recorded alone on a fresh engine the side chain is the one recorded behind
    the main chain -- same launchers, same buffers summed"""
    import drvae_amd.tuning as T
    steps = recorded_steps(False)
    kernel_ref.install(monkeypatch)
    monkeypatch.setenv('DRVAE_TUNE', 'fold_rows=0')
    monkeypatch.setattr(T, '_VALUES', None)
    assert steps
    for (name, universal, split), rec in steps.items():
        case = C.model_case(name)
        with pytest.MonkeyPatch.context() as inner:
            alone = record_side_alone(case['spec'], M.init_params(case['spec'], case['param_seed'], as_numpy=True),
                                      case['batch'], case['noises'][0], universal, split, inner)
        assert _side(alone) == _side(rec), (name, universal, split)
        assert alone.launches == [l for l in rec.launches if l[0] == 'side']


@pytest.mark.parametrize('kind', ['drvae', 'vfae'])
def test_the_side_chain_sums_the_raw_row_pass_s_partials_whatever_ran_before_it(kind, monkeypatch):
    """the same on the raw-heads route with the bias gradient in the row pass (the chip-filling step's, forced at a small
    size): main-then-side and side alone both sum ``NLLC``"""
    import drvae_amd.kernels as K
    import drvae_amd.tuning as T
    monkeypatch.setenv('DRVAE_TUNE', 'fuse_heads=0,raw_heads=2,nll_cs=2,fold_rows=0')
    monkeypatch.setattr(T, '_VALUES', None)
    kernel_ref.install(monkeypatch)
    spec = C.tiny_spec(kind, dim_x=16, h_de_x=[8])
    params, batch, noise = M.init_params(spec, 4, as_numpy=True), M.make_batch(spec, 12, seed=3), M.make_noise(spec, 12, seed=5)
    seen = []
    for split in SPLITS:
        eng, _ = make_engine(spec, params)
        set_batch(eng, batch)
        eng.set_noise(noise)
        tail = eng._step_tail(split, on_gpu=True)
        assert tail.dual
        with pytest.MonkeyPatch.context() as inner:
            rec = Recorder(eng, K, inner)
            with eng._recording('main', tail):
                rec.begin('main')
                eng._launch_sequence(allreduce=(lambda buf: None) if split == 'captured' else None)
            with eng._recording('side', tail):
                rec.begin('side')
                eng._launch_sequence(draw=False, optimizer=False)
        with pytest.MonkeyPatch.context() as inner:
            alone = record_side_alone(spec, params, batch, noise, False, split, inner)
        assert ('main', 'nll_rows_raw_cs') in rec.launches, split
        assert _side(alone) == _side(rec), split
        for chain, terms in rec.loss_terms + alone.loss_terms:
            if terms:       # (``terms_elsewhere``: the main chain's launch only parks and bumps)
                assert terms[0] == 'NLLC', (split, chain, terms)
                seen.append(chain)
    assert 'side' in seen and 'main' in seen
