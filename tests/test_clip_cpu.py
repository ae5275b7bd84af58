"""CPU: gradient-norm clipping and the non-finite guard of the fused train step -- the reference's checks against faulty
emulations, construction, the schedule decision, the clipped step against torch's clip + optimiser in float64, the skipped
step and the optimiser-state round trip -- with the HIP launchers replaced by their plain-PyTorch references
(tests/kernel_ref.py).  The kernels themselves are checked on the GPU (tests/test_gpu_clip.py)."""
import dataclasses
import math

import numpy as np
import pytest
import torch

from oracle import models_ref as M
from tests import clip_ref as R
from tests import kernel_ref
from tests.golden import cases as C
from tests.test_dropout_cpu import set_batch, tiny_model

# the tiny golden cases of the three models, a WeightNorm one and an Adamax one
STEP_CASES = ['tiny_drvae', 'tiny_vfae', 'tiny_pvae', 'tiny_drvae_wn', 'tiny_drvae_adamax']
CLIP_LAUNCHES = {'clip_norm', 'adam_l2_clip', 'adamax_l2_clip'}
STATE = ('param', 'exp_avg', 'exp_avg_sq')


def make_engine(spec, params, max_grad_norm=None, device='cpu', **kw):
    from drvae_amd import engine as E
    from drvae_amd.arena import ParamArena
    cfg_kw = {k: getattr(spec, k) for k in E.StepConfig.__dataclass_fields__ if hasattr(spec, k)}
    cfg_kw.update(kw)
    cfg = E.StepConfig(max_grad_norm=max_grad_norm, **cfg_kw)
    arena = ParamArena(E.param_shapes(cfg), device, frozen=E.frozen_params(cfg))
    arena.load(params)
    return E.FusedStep(cfg, arena), arena


def case_of(name):
    case = C.model_case(name)
    return case, case['spec'], M.init_params(case['spec'], case['param_seed'], as_numpy=True)


def gradients(eng, noise):
    """forward + backward of a train pass on injected noise; nothing is updated"""
    eng.training = True
    eng.join_side()
    eng.set_noise(noise)
    eng._launch_sequence(draw=False, optimizer=False)


def live_names(arena, cfg):
    from drvae_amd import engine as E
    frozen = set(E.frozen_params(cfg))
    return [k for k in arena.shapes if k not in frozen]


def grad_norm64(arena, cfg):
    """the float64 2-norm of the per-parameter gradient VIEWS (no pad element is read)"""
    return math.sqrt(sum(float((arena.g(k).detach().cpu().double() ** 2).sum()) for k in live_names(arena, cfg)))


class Torch64:
    """the float64 route: torch.nn.utils.clip_grad_norm_ + torch.optim.Adam / Adamax (coupled L2) on float64 copies of the
    parameters, fed with an unclipped engine's gradients"""

    def __init__(self, arena, cfg, max_norm):
        self.names = live_names(arena, cfg)
        self.p = {k: arena.p(k).detach().cpu().double().clone().requires_grad_(True) for k in self.names}
        opt = torch.optim.Adamax if cfg.optim_alg == 'adamax' else torch.optim.Adam
        self.opt = opt(list(self.p.values()), lr=cfg.learning_rate, weight_decay=cfg.weight_decay)
        self.max_norm = max_norm

    def step(self, arena):
        for k in self.names:
            self.p[k].grad = arena.g(k).detach().cpu().double().clone()
        norm = torch.nn.utils.clip_grad_norm_(list(self.p.values()), self.max_norm, norm_type=2)
        self.opt.step()
        return float(norm)

    def state(self, k, what):
        if what == 'param':
            return self.p[k].detach()
        st = self.opt.state[self.p[k]]
        return st['exp_avg'] if what == 'exp_avg' else st.get('exp_avg_sq', st.get('exp_inf'))


def compare_state(arena, ref, label, what=STATE):
    """norm-wise, per parameter, at the gradient tolerance of ``compare_step`` (tests/test_dropout_cpu.py): 1e-4"""
    from drvae_amd.arena import ParamArena  # noqa: F401
    worst = 0.0
    for w in what:
        buf = getattr(arena, w)
        for k in ref.names:
            a, b = arena._view(buf, k).detach().cpu().double(), ref.state(k, w)
            dev, nb = float((a - b).norm()), float(b.norm())
            worst = max(worst, dev / nb if nb > 0 else dev)
            assert dev <= 1e-4 * nb, (label, w, k, dev, nb)
    print('%s: worst norm-wise deviation of parameters and moments from the float64 route %.3g' % (label, worst))
    return worst


# ------------------------------------------------------------------------------------------------ 1. the checks themselves
def test_reference_bound_catches_an_fp32_accumulation():
    n = (1 << 20) + 3
    g = R.values('normal', n)
    want = R.ref(g, 1.0, 1.0)
    good = R.as_f32(want)
    assert R.check(good, want) <= 0.51            # the fp32 store of the reference itself: half an ulp, a quarter of the bound
    bad = R.as_f32(R.record(R.sumsq_fp32(g), 1.0, 1.0))
    err = abs(bad['norm'] - want['norm']) / R.bound(want['norm'])
    print('fp32 running sum over %d unit normals: norm %.1f bounds off' % (n, err))
    assert err > 4.0
    with pytest.raises(AssertionError):
        R.check(bad, want)
    # ... and the class at the ends of the fp32 range: no skip, the norm is the one large element
    g = R.values('one_huge', 4099)
    assert R.ref(g)['skip'] == 0 and abs(R.ref(g)['norm'] / 1e18 - 1) < 1e-6


def test_reference_bound_catches_a_missing_epsilon():
    g = (R.values('normal', 4099) / np.float32(64.0)).astype(np.float32)      # norm ~ 1: 1e-6 is 8 U of it
    s = R.sumsq64(g)
    want = R.record(s, 1.0, 0.5)
    assert 0.5 < want['norm'] < 2.0 and want['coef'] < 1.0
    bad = R.as_f32(R.record_no_eps(s, 1.0, 0.5))
    with pytest.raises(AssertionError):
        R.check(bad, want)
    assert R.check(R.as_f32(want), want) <= 0.51
    # the record's corner cases
    assert R.ref(R.values('zeros', 5), 1.0, 2.0) == dict(norm=0.0, coef=1.0, skip=0)
    assert R.ref(g, 1.0, float('inf'))['coef'] == 1.0
    for bad_value in (np.nan, np.inf, -np.inf):
        h = g.copy()
        h[7] = bad_value
        assert R.ref(h, 1.0, 0.5)['skip'] == 1 and R.ref(h, 1.0, 0.5)['coef'] == 0.0


def test_stand_in_record_matches_the_reference(monkeypatch):
    import drvae_amd.kernels as K
    kernel_ref.install(monkeypatch)
    for cls in R.CLASSES:
        for n in (1, 5, 4099):
            g = R.values(cls, n)
            st = K.clip_state('cpu', n, 0.25)
            K.clip_norm(torch.from_numpy(g), st, gscale=0.5)
            got = K.clip_record_values(K.clip_record(st))
            R.check(dict(norm=got['norm'], coef=got['coef'], skip=int(got['skipped_last'])), R.ref(g, 0.5, 0.25), (cls, n))
            assert got['n_skipped'] == 0


# ------------------------------------------------------------------------------------------------ 2. construction
@pytest.mark.parametrize('kind', ['drvae', 'pvae', 'vfae'])
def test_models_construct_with_and_without_a_threshold(kind):
    from drvae_amd import engine as E
    plain, none = tiny_model(kind), tiny_model(kind, max_grad_norm=None)
    assert plain._step_config() == none._step_config() and none._step_config().max_grad_norm is None
    today = {f.name: getattr(plain._step_config(), f.name) for f in dataclasses.fields(E.StepConfig) if f.name != 'max_grad_norm'}
    assert E.StepConfig(**today) == plain._step_config()
    assert tiny_model(kind, max_grad_norm=2.5)._step_config().max_grad_norm == 2.5
    assert tiny_model(kind, max_grad_norm=float('inf'))._step_config().max_grad_norm == float('inf')
    assert list(tiny_model(kind, max_grad_norm=1.0).state_dict()) == list(plain.state_dict())
    for bad in (0, 0.0, -1, float('nan')):
        with pytest.raises(ValueError):
            tiny_model(kind, max_grad_norm=bad)
        with pytest.raises(ValueError):
            E.StepConfig(max_grad_norm=bad)
    with pytest.raises(RuntimeError):
        plain.grad_clip_stats()


def _launch_log(monkeypatch_ctx, names):
    import drvae_amd.kernels as K
    log = []
    for fn in names:
        real = getattr(K, fn)
        monkeypatch_ctx.setattr(K, fn, lambda *a, _f=real, _n=fn, **k: (log.append(_n), _f(*a, **k))[1])
    return log


@pytest.mark.parametrize('name', ['tiny_drvae', 'tiny_pvae', 'tiny_vfae', 'tiny_drvae_adamax'])
def test_switch_off_launches_what_it_always_did(name, monkeypatch):
    kernel_ref.install(monkeypatch)
    case, spec, params = case_of(name)
    lists = {}
    for tag, kw in (('absent', None), ('none', dict(max_grad_norm=None)), ('set', dict(max_grad_norm=0.5))):
        if kw is None:
            from tests.test_dropout_cpu import make_engine as plain_engine
            eng, _ = plain_engine(spec, params)
        else:
            eng, _ = make_engine(spec, params, **kw)
        set_batch(eng, case['batch'])
        with pytest.MonkeyPatch.context() as mp:
            log = _launch_log(mp, kernel_ref.FUNCTIONS)
            eng.train_step(case['noises'][0])
        lists[tag] = log
        assert (eng.clip_rec is None) == (tag != 'set') and (eng.clip_part is None) == (tag != 'set')
    assert lists['absent'] == lists['none'] and not (set(lists['none']) & CLIP_LAUNCHES)
    sweep = 'adamax_l2' if spec.optim_alg == 'adamax' else 'adam_l2'
    assert lists['none'][-1] == sweep and lists['none'].count(sweep) == 1
    assert lists['set'] == lists['none'][:-1] + ['clip_norm', sweep + '_clip']


# ------------------------------------------------------------------------------------------------ 3. the schedule
def test_a_clipped_step_keeps_nothing_behind_the_join(monkeypatch):
    """cfg-2 shape (the default DrVAE configuration, 150 rows): the unclipped single-process step runs the classifier's weight
    gradient and the decoder heads' half of the sweep behind the join; the clipped one is recorded like an exchange form"""
    kernel_ref.install(monkeypatch)
    spec = M.ModelSpec(kind='drvae')
    params = M.init_params(spec, 3, as_numpy=True)
    batch = M.make_batch(spec, 150, seed=5)
    tails = {}
    for tag, kw in (('plain', {}), ('inf', dict(max_grad_norm=float('inf'))), ('set', dict(max_grad_norm=1.0))):
        eng, _ = make_engine(spec, params, **kw)
        set_batch(eng, batch)
        tails[tag] = {split: eng._step_tail(split, on_gpu=True) for split in (False, True, 'overlap', 'captured')}
    from tests.test_dropout_cpu import make_engine as plain_engine
    eng, _ = plain_engine(spec, params)
    set_batch(eng, batch)
    for split, t in tails['plain'].items():
        assert t == eng._step_tail(split, on_gpu=True)
    t = tails['plain'][False]
    assert t.dual and t.late and t.side_adam and t.adam_gated and t.noise_ahead, t
    for tag in ('inf', 'set'):
        c = tails[tag][False]
        assert c.dual and not (c.late or c.side_adam or c.adam_gated or c.tail_gated or c.side_loss or c.noise_ahead
                               or c.cap_fork), c
        # ... which is how the overlapped exchange is recorded, clipped or not
        assert c == tails['plain']['overlap'] == tails[tag]['overlap']
        assert tails[tag][True] == tails['plain'][True]
        assert not tails[tag]['captured'].cap_fork and not tails[tag]['captured'].late
    # a model without a classifier has only the tail to give to a side chain: clipped, its step is one graph
    spec = M.ModelSpec(kind='pvae', L=1)
    params = M.init_params(spec, 3, as_numpy=True)
    batch = M.make_batch(spec, 150, seed=5)
    for kw, dual in (({}, True), (dict(max_grad_norm=1.0), False)):
        eng, _ = make_engine(spec, params, **kw)
        set_batch(eng, batch)
        t = eng._step_tail(False, on_gpu=True)
        assert t.dual == dual and t.late == dual and t.side_adam == dual, t


# ------------------------------------------------------------------------------------------------ 4. the clipped step
@pytest.mark.parametrize('name', STEP_CASES)
def test_clipped_step_against_torch_in_float64(name, monkeypatch):
    kernel_ref.install(monkeypatch)
    case, spec, params = case_of(name)
    noise = case['noises'][0]
    plain, parena = make_engine(spec, params)
    set_batch(plain, case['batch'])
    gradients(plain, noise)
    norm = grad_norm64(parena, plain.cfg)
    assert math.isfinite(norm) and norm > 0
    thr = 0.5 * norm                                   # clipping is active
    ref = Torch64(parena, plain.cfg, thr)
    assert abs(ref.step(parena) - norm) <= 1e-12 * norm
    eng, arena = make_engine(spec, params, max_grad_norm=thr)
    set_batch(eng, case['batch'])
    eng.train_step(noise)
    st = eng.clip_stats()
    assert not st['skipped_last'] and st['n_skipped'] == 0
    # the norm over the whole live slice (pad elements included) is the norm over the parameters' views
    R.check(dict(norm=st['norm'], coef=st['coef'], skip=0), R.record(norm * norm, 1.0, thr), name)
    assert abs(st['coef'] - 0.5) < 1e-5
    compare_state(arena, ref, name)
    # the moments say that the coefficient was applied (Adam's update alone is nearly invariant under it): unclipped, the
    # first moment is twice as large
    plain.optimizer_step()
    k = ref.names[0]
    a, b = parena._view(parena.exp_avg, k).double(), ref.state(k, 'exp_avg')
    assert float((a - b).norm()) > 0.1 * float(b.norm())


@pytest.mark.parametrize('name', ['tiny_drvae', 'tiny_drvae_wn', 'tiny_drvae_adamax'])
def test_threshold_above_the_norm_changes_no_bit(name, monkeypatch):
    kernel_ref.install(monkeypatch)
    case, spec, params = case_of(name)
    states = []
    for kw in ({}, dict(max_grad_norm=1e6), dict(max_grad_norm=float('inf'))):
        eng, arena = make_engine(spec, params, **kw)
        set_batch(eng, case['batch'])
        for noise in case['noises'][:2]:
            eng.train_step(noise)
        if kw:
            assert eng.clip_stats()['coef'] == 1.0
        states.append([getattr(arena, w).clone() for w in STATE])
    for other in states[1:]:
        assert all(torch.equal(a, b) for a, b in zip(states[0], other))


# ------------------------------------------------------------------------------------------------ 5. the skipped step
@pytest.mark.parametrize('bad', [float('inf'), float('nan')], ids=['inf', 'nan'])
@pytest.mark.parametrize('name', ['tiny_drvae', 'tiny_drvae_adamax'])
def test_a_non_finite_gradient_skips_the_step_and_leaves_no_trace(name, bad, monkeypatch):
    kernel_ref.install(monkeypatch)
    case, spec, params = case_of(name)
    noises = case['noises']
    eng, arena = make_engine(spec, params, max_grad_norm=float('inf'))
    set_batch(eng, case['batch'])
    eng.train_step(noises[0])
    before = [getattr(arena, w).clone() for w in STATE]
    halt = eng.sync_err.clone()
    gradients(eng, noises[1 % len(noises)])
    arena.g(list(arena.shapes)[1]).view(-1)[0] = bad            # one element of one gradient
    eng.optimizer_step()
    st = eng.clip_stats()
    assert st['skipped_last'] and st['n_skipped'] == 1 and st['coef'] == 0.0 and not math.isfinite(st['norm'])
    assert all(torch.equal(a, getattr(arena, w)) for a, w in zip(before, STATE))
    assert torch.equal(halt, eng.sync_err) and int(eng.step_dev) == 2
    # the next clean step is the SECOND step of an engine that never saw the skipped one: t was corrected
    eng.train_step(noises[1 % len(noises)])
    st = eng.clip_stats()
    assert not st['skipped_last'] and st['n_skipped'] == 1 and int(eng.step_dev) == 3
    twin, tarena = make_engine(spec, params, max_grad_norm=float('inf'))
    set_batch(twin, case['batch'])
    twin.train_step(noises[0])
    twin.train_step(noises[1 % len(noises)])
    assert int(twin.step_dev) == 2 and twin.clip_stats()['n_skipped'] == 0
    assert all(torch.equal(getattr(tarena, w), getattr(arena, w)) for w in STATE)


def test_a_skipped_first_step_divides_by_nothing(monkeypatch):
    kernel_ref.install(monkeypatch)
    case, spec, params = case_of('tiny_drvae')
    eng, arena = make_engine(spec, params, max_grad_norm=1.0)
    set_batch(eng, case['batch'])
    before = [getattr(arena, w).clone() for w in STATE]
    gradients(eng, case['noises'][0])
    arena.grad[arena.n_live - 1] = float('-inf')
    eng.optimizer_step()                               # t = step - n_skipped = 0: the corrections are never evaluated
    assert eng.clip_stats()['n_skipped'] == 1
    assert all(torch.equal(a, getattr(arena, w)) for a, w in zip(before, STATE))


# ------------------------------------------------------------------------------------------------ 6. the state travels
def test_stash_and_restore_keep_the_skip_count(monkeypatch):
    kernel_ref.install(monkeypatch)
    model = tiny_model('drvae', max_grad_norm=3.0)
    eng = model.engine()
    eng.clip_rec[3] = 5
    eng.step_dev.fill_(9)
    model._stash_optimizer_state()
    assert model._opt_stash['n_skipped'] == 5
    model._engine = model._arena = None
    eng2 = model.engine()
    assert eng2 is not eng and int(eng2.clip_rec[3]) == 5 and int(eng2.step_dev) == 9
    assert model.grad_clip_stats()['n_skipped'] == 5
    # a model without the switch stashes nothing of it
    plain = tiny_model('drvae')
    plain.engine()
    plain._stash_optimizer_state()
    assert 'n_skipped' not in plain._opt_stash


# ------------------------------------------------------------------------------------------------ 7. header and bindings
def _header():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(root, 'include', 'drvae_hip.h')).read(), flags=re.S)


def _c_ternary(expr, env):
    """value of a C expression of integer literals, names of ``env``, + - * / comparisons, parentheses and ?: (as the header's
    DV_SUMSQ_PARTIALS is written)"""
    expr = expr.strip()
    while expr.startswith('('):           # outer parentheses that enclose the whole expression
        depth = 0
        for i, ch in enumerate(expr):
            depth += ch == '('
            depth -= ch == ')'
            if depth == 0:
                break
        if i != len(expr) - 1:
            break
        expr = expr[1:-1].strip()
    depth, q = 0, -1
    for i, ch in enumerate(expr):
        depth += ch == '('
        depth -= ch == ')'
        if depth == 0 and ch == '?':
            q = i
            break
    if q < 0:
        return eval(expr.replace('/', '//'), {'__builtins__': {}}, dict(env))
    depth = nest = 0
    for j in range(q + 1, len(expr)):
        ch = expr[j]
        depth += ch == '('
        depth -= ch == ')'
        if depth == 0 and ch == '?':
            nest += 1
        if depth == 0 and ch == ':':
            if nest == 0:
                break
            nest -= 1
    cond, a, b = expr[:q], expr[q + 1:j], expr[j + 1:]
    return _c_ternary(a, env) if _c_ternary(cond, env) else _c_ternary(b, env)


def test_bindings_follow_the_header():
    """the clip state's layout and the workspace size are written twice (header, python): the ctypes mirrors have the header's
    fields, and ``kernels.sumsq_partials`` -- what the caller sizes the workspace by -- is the header's DV_SUMSQ_PARTIALS --
    what the launch sizes its grid by -- at every size where either changes"""
    import ctypes
    import re
    from drvae_amd import _lib
    import drvae_amd.kernels as K
    src = _header()
    for cname, py in (('dv_clip_record', _lib.ClipRecord), ('dv_clip_state', _lib.ClipState)):
        body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (cname, cname), src, flags=re.S).group(1)
        decls = [d.strip().rsplit(None, 1) for d in body.split(';') if d.strip()]
        assert [n for _, n in decls] == [f[0] for f in py._fields_], cname
        size = {'float': 4, 'int32_t': 4, 'double': 8, 'dv_clip_record': ctypes.sizeof(_lib.ClipRecord)}
        assert [size[t] for t, _ in decls] == [ctypes.sizeof(f[1]) for f in py._fields_], cname
    assert ctypes.sizeof(_lib.ClipState) == 32 and _lib.ClipState.max_norm.offset == 8 and _lib.ClipState.rec.offset == 16
    assert K.CLIP_STATE_WORDS == 8
    defs = {k: int(v) for k, v in re.findall(r'#define (DV_SUMSQ_PER_BLOCK|DV_SUMSQ_MAX_BLOCKS)\s+(\d+)', src)}
    assert defs == {'DV_SUMSQ_PER_BLOCK': _lib.SUMSQ_PER_BLOCK, 'DV_SUMSQ_MAX_BLOCKS': _lib.SUMSQ_MAX_BLOCKS}
    macro = re.search(r'#define DV_SUMSQ_PARTIALS\(n\)\s+(.*)', src).group(1).replace('(int64_t)', '')
    per, cap = defs['DV_SUMSQ_PER_BLOCK'], defs['DV_SUMSQ_MAX_BLOCKS']
    sizes = {0, 1, 2, per - 1, per, per + 1, 2 * per, 2 * per + 1, 4099, (1 << 20) + 3, (16 << 20) + 5, 1 << 31, 1 << 40}
    for k in (cap - 2, cap - 1, cap, cap + 1):
        sizes |= {k * per - 1, k * per, k * per + 1}
    for n in sorted(sizes):
        want = _c_ternary(macro, dict(defs, n=n))
        assert K.sumsq_partials(n) == want, (n, K.sumsq_partials(n), want)
        assert 1 <= want <= cap
    assert _c_ternary(macro, dict(defs, n=per + 1)) == 2 and _c_ternary(macro, dict(defs, n=1 << 40)) == cap
