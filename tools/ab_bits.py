"""Bits of two builds of the library, side by side: runs a fixed, seeded list of calls through whichever library DRVAE_HIP_LIB
names (default: the tree's) and writes {case: sha256 over every output buffer, pads included} as JSON.  One process per library:

    DRVAE_HIP_LIB=build_lab/libdrvae_prev.so python tools/ab_bits.py prev.json
    python tools/ab_bits.py new.json && python tools/ab_bits.py --diff prev.json new.json

The cases are the row kernels whose formulas are shared device functions (y-marginalisation, the classifier head and its riders,
KL rows, the z2Fz1 backward, the prior-KL rider, clamp(softmax)), the Philox fills, the counter launches, a wait on a flag that
is already published, and three eager train steps per model and optimiser.  Small shapes: every path of every kernel, seconds in
total.  ``dv_source_hash`` is not looked at: the libraries are meant to differ in source."""
import hashlib
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = None
CASES = {}


def rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def padded(rows, w, seed=None, pad=3):
    """(base, view): a (rows, w) view of a (rows, w + pad) buffer -- sentinel or seeded contents, the pads are hashed too"""
    base = rnd(rows, w + pad, seed=seed) if seed is not None else torch.full((rows, w + pad), 7.0, device=DEV)
    return base, base[:, :w]


def i32(a):
    return torch.as_tensor(np.asarray(a, dtype=np.int64).astype(np.int32)).to(DEV)


def record(name, *outs):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in outs:
        a = t.detach().contiguous().cpu().numpy()
        h.update(('%s%s' % (a.dtype, a.shape)).encode())
        h.update(a.tobytes())
    assert name not in CASES, name
    CASES[name] = h.hexdigest()


# ------------------------------------------------------------------------------------------------- y-marginalisation
def ymarg_rows(R, Y, seed):
    """rows of all three kinds: labeled with one fprop row, label <= -2 with Y slots, marginalised (label -1, Y slots)"""
    rs = np.random.RandomState(seed)
    label, sizes = [], []
    for r in range(R):
        c = int(rs.randint(0, Y))
        kind = r % 3
        label.append(c if kind == 0 else (-2 - c if kind == 1 else -1))
        sizes.append(1 if kind == 0 else Y)
    return i32(label), i32(np.concatenate([[0], np.cumsum(sizes)]))


def probs_rows(R, Y, seed):
    q = torch.softmax(rnd(R, Y, seed=seed, scale=2.0), 1).clamp(1e-10, 1.0)
    q[4, 0] = 1e-10                      # probabilities on the clamp, in rows of all three kinds
    q[3, Y - 1] = 1e-10
    q[5, 1] = 1e-10
    return q.contiguous()


def ymarg_cases(K):
    R = 37
    for Y in (2, 5, 8):
        label, fp_ptr = ymarg_rows(R, Y, 10 + Y)
        Mf = int(fp_ptr[-1])
        qy, klfp = probs_rows(R, Y, 20 + Y), rnd(Mf, seed=30 + Y).abs() * 3
        c_kld, c_yl = rnd(R, seed=40 + Y), rnd(R, seed=50 + Y)
        for tag, lp in (('scalar', math.log(1.0 / Y)), ('vector', torch.log_softmax(rnd(Y, seed=60 + Y), 0))):
            new = lambda: (torch.full((R,), 7.0, device=DEV), torch.full((R,), 7.0, device=DEV),
                           torch.full((Mf,), 7.0, device=DEV)) + padded(R, Y)
            yl, kld, _, _, _ = new()
            K.ymarg_fwd(yl, kld, qy, label, fp_ptr, klfp, lp)
            record('ymarg_fwd/Y%d/%s' % (Y, tag), yl, kld)
            _, _, cfp, dbase, dqy = new()
            K.ymarg_bwd(cfp, dqy, qy, label, fp_ptr, klfp, lp, c_kld, c_yl)
            record('ymarg_bwd/Y%d/%s' % (Y, tag), cfp, dbase)
            yl, kld, cfp, dbase, dqy = new()
            K.ymarg_fwdbwd(yl, kld, cfp, dqy, qy, label, fp_ptr, klfp, lp, c_kld, c_yl)
            record('ymarg_fwdbwd/Y%d/%s' % (Y, tag), yl, kld, cfp, dbase)


# ------------------------------------------------------------------------------------------------- classifier head
def smalln_case(K, tag, N, K1, K2, Z1, Z3, riders, kl_mins=(0.0,)):
    """dv_smalln_linear_fwd, M = 9; riders: '' | 'y' | 'yk' | 'ykd' (ymarg, + fprop_kl, + dgrad).  'tie' among kl_mins: a value
    equal to a stored raw1 (taken from the kl_min = 0 run of the same library)"""
    M = 9
    a1, a2 = rnd(M, K1, seed=1), rnd(M, K2, seed=2)
    W, bias = rnd(N, K1 + K2, seed=3, scale=0.2), rnd(N, seed=4)
    if N == 1:
        label, fp_ptr = i32([0] * M), i32(np.arange(M + 1))
    else:
        label, fp_ptr = ymarg_rows(M, N, 5)
    Mf = int(fp_ptr[-1])
    c_kld, c_yl = rnd(M, seed=6), rnd(M, seed=7)
    nq = M + 2
    Q, P, Q3 = rnd(nq, 2 * Z1, seed=8, scale=0.5), rnd(Mf, 2 * Z1, seed=9, scale=0.5), rnd(Mf, 2 * Z3, seed=10, scale=0.5)
    qidx = i32(np.random.RandomState(11).randint(0, nq, Mf))
    tie = None
    for kl_min in kl_mins:
        if kl_min == 'tie':
            kl_min = tie
        lbase, logits = padded(M, N)
        pbase, probs = padded(M, N)
        outs, kw = [lbase, pbase], {}
        if riders:
            yl, kld, cfp = (torch.full((n,), 7.0, device=DEV) for n in (M, M, Mf))
            dbase, dqy = padded(M, N)
            klfp = rnd(Mf, seed=12).abs() * 3 if 'k' not in riders else torch.full((Mf,), 7.0, device=DEV)
            kw['ymarg'] = (yl, kld, cfp, dqy, label, fp_ptr, klfp, math.log(1.0 / N), c_kld, c_yl)
            outs += [yl, kld, cfp, dbase, klfp]
        if 'k' in riders:
            raw1, raw3 = torch.full((Mf,), 7.0, device=DEV), torch.full((Mf,), 7.0, device=DEV)
            qb, dq = padded(Mf, 2 * Z1)
            pb, dp = padded(Mf, 2 * Z1)
            kw['fprop_kl'] = dict(Q=Q, qidx=qidx, P=P, Q3=Q3, Z1=Z1, Z3=Z3, kl_min=kl_min, raw1=raw1, raw3=raw3, dq=dq, dp=dp)
            outs += [raw1, raw3, qb, pb]
        if 'd' in riders:          # both destinations, the first with a second column block (classifier on [z1, z2F - z1])
            b0, d0 = padded(M, K1, seed=13)
            b1, d1 = padded(M, K2, seed=14)
            kw['dgrad'] = [(d0, 0, 1.0, 1.0, K1, -1.0), (d1, K1, 0.5, 0.0)]
            outs += [b0, b1]
        K.smalln_fwd(probs, logits, a1, W, bias, a2, **kw)
        which = 'tie' if kl_min == tie and tie is not None else kl_min
        record('smalln_fwd/%s/%s/kl_min=%s' % (tag, riders or 'bare', which), *outs)
        if 'k' in riders and tie is None:
            tie = float(raw1[1])


def smalln_cases(K):
    for riders in ('', 'y', 'yk', 'ykd'):
        smalln_case(K, 'fwd2_64_32', 2, 64, 64, 32, 32, riders)
    three = (0.0, 1e4, 'tie')
    smalln_case(K, 'fwd2_64_32/gates', 2, 64, 64, 32, 32, 'ykd', three)
    smalln_case(K, 'fwd2_edges', 2, 128, 128, 128, 100, 'ykd', three)
    smalln_case(K, 'fwd2_N1', 1, 64, 64, 32, 32, 'ykd', three)
    smalln_case(K, 'generic_N3', 3, 64, 64, 32, 32, 'ykd', three)
    smalln_case(K, 'generic_Z130', 2, 64, 64, 130, 32, 'ykd', three)
    smalln_case(K, 'generic_K260', 2, 130, 130, 32, 32, 'ykd', three)
    smalln_case(K, 'generic_N3', 3, 64, 64, 32, 32, 'y')
    smalln_case(K, 'generic_N3', 3, 64, 64, 32, 32, '')


# ------------------------------------------------------------------------------------------------- KL rows
def kl_cases(K):
    n = 7
    for reps in (1, 3):
        for Z in (5, 64, 130):
            for mode in (K.GAUSS_LOGVAR, K.GAUSS_SIGMA):
                R = n * reps
                tag = 'reps%d/Z%d/mode%d' % (reps, Z, mode)
                sd = (lambda t: t.abs() + 0.1) if mode == K.GAUSS_SIGMA else (lambda t: t)
                Qb, Pb = rnd(n + 2, 2 * Z + 1, seed=1, scale=0.5), rnd(R + 2, 2 * Z + 1, seed=2, scale=0.5)
                mq, sq, mp, sp = Qb[:, :Z], sd(Qb[:, Z:2 * Z]), Pb[:, :Z], sd(Pb[:, Z:2 * Z])
                if mode == K.GAUSS_SIGMA:      # (two views of one buffer again: the launchers take one leading dimension)
                    Qb[:, Z:2 * Z], Pb[:, Z:2 * Z] = sq, sp
                    sq, sp = Qb[:, Z:2 * Z], Pb[:, Z:2 * Z]
                rs = np.random.RandomState(3)
                qidx, pidx = i32(rs.randint(0, n + 2, n)), i32(rs.permutation(R + 2)[:R])
                add = rnd(R, seed=4)
                gathered = dict(mode=mode, qidx=qidx, pidx=pidx, reps=reps)
                # gathered operands against mu_p, free bits with a tie, add
                out, raw = torch.full((R,), 7.0, device=DEV), torch.full((R,), 7.0, device=DEV)
                K.kl_rows_fwd(out, raw, mq, sq, mp, sp, **gathered)
                kl_min = float(raw[1])
                out2, raw2 = torch.full((R,), 7.0, device=DEV), torch.full((R,), 7.0, device=DEV)
                K.kl_rows_fwd(out2, raw2, mq, sq, mp, sp, free_bits=True, kl_min=kl_min, add=add, **gathered)
                record('kl_rows_fwd/%s/gathered' % tag, out, raw, out2, raw2)
                # plain rows against the prior, with the fused sample and the second term
                prior = (0.0, 0.0) if mode == K.GAUSS_LOGVAR else (0.0, 1.0)
                eps, (zb, zout) = rnd(R, Z, seed=5), padded(R, Z)
                S = rnd(R, 2 * Z, seed=6, scale=0.5)
                if mode == K.GAUSS_SIGMA:
                    S[:, Z:] = S[:, Z:].abs() + 0.1
                out3, raw3, rawS = (torch.full((R,), 7.0, device=DEV) for _ in range(3))
                K.kl_rows_fwd(out3, raw3, mq[:n], sq[:n], prior=prior, mode=mode, reps=reps, free_bits=True, kl_min=kl_min,
                              eps=eps, zout=zout, second=(S[:, :Z], S[:, Z:], rawS))
                out4 = torch.full((R,), 7.0, device=DEV)
                K.kl_rows_fwd(out4, None, mq[:n], sq[:n], prior=prior, mode=mode, reps=reps)
                record('kl_rows_fwd/%s/prior' % tag, out3, raw3, rawS, zb, out4)
                # the two sets in one launch
                o1, r1, o2, r2 = (torch.full((R,), 7.0, device=DEV) for _ in range(4))
                K.kl_rows_fwd_pair(((o1, r1, mq, sq, mp, sp), dict(free_bits=True, kl_min=kl_min, add=add, **gathered)),
                                   ((o2, r2, mq[:n], sq[:n]), dict(prior=prior, mode=mode, reps=reps)))
                record('kl_rows_fwd_pair/%s' % tag, o1, r1, o2, r2)
                # backward: both operand sides, free bits on (the tie) and off, the sample's gradient, beta 0 and 1
                coef, dz = rnd(R, seed=7), rnd(R, Z, seed=8)
                for beta in (0.0, 1.0):
                    (qb, dq), (pb, dp) = padded(R, 2 * Z, seed=9), padded(R, 2 * Z, seed=10)
                    K.kl_rows_bwd(dq[:, :Z], dq[:, Z:], dp[:, :Z], dp[:, Z:], coef, raw2, mq, sq, mp, sp, free_bits=True,
                                  kl_min=kl_min, beta=beta, dz=dz, eps=eps, **gathered)
                    (q2b, dq2) = padded(R, 2 * Z, seed=11)
                    K.kl_rows_bwd(dq2[:, :Z], dq2[:, Z:], None, None, coef, None, mq[:n], sq[:n], prior=prior, mode=mode,
                                  reps=reps, beta=beta)
                    record('kl_rows_bwd/%s/beta%d' % (tag, beta), qb, pb, q2b)


# ------------------------------------------------------------------------------------------------- z2Fz1 backward, prior rider
def z2f_cases(K):
    L, B, Np = 2, 12, 5
    slot = torch.full((B,), -1, dtype=torch.int32)
    slot[torch.tensor([1, 4, 5, 8, 11])] = torch.arange(Np, dtype=torch.int32)
    slot = slot.to(DEV)
    for Z in (100, 130):                  # the narrow (two dims per lane) and the wide kernel
        Q2 = rnd(Np, 2 * Z, seed=1, scale=0.5)
        p2, pert = rnd(L * B, 2 * Z, seed=2, scale=0.5), rnd(L * Np, Z, seed=3)
        eps, dz2f, dz1b = rnd(L * B, Z, seed=4), rnd(L * B, Z, seed=5), rnd(L * B, Z, seed=6)
        coef, pc = rnd(L * Np, seed=7), rnd(Np, seed=8)
        praw = torch.empty(Np, device=DEV)
        K.kl_rows_fwd(torch.empty(Np, device=DEV), praw, Q2[:, :Z], Q2[:, Z:], prior=(0.0, 0.0))
        seg_ptr = i32(np.concatenate([[0], np.cumsum(np.random.RandomState(9).randint(0, 3, L * B))]))
        seg_src = rnd(int(seg_ptr[-1]) + 1, Z + 2, seed=10)
        raw_in = rnd(L * Np, seed=11).abs() * 40
        for kl_min, own in ((float(praw[2]), True), (float(raw_in[3]), False), (0.0, True)):
            (pb, dp2), (zb, dz1), (qb, dq2) = padded(L * B, 2 * Z), padded(L * B, Z, seed=12), padded(Np, 2 * Z)
            kl_out, raw = torch.full((L * Np,), 7.0, device=DEV), (torch.full((L * Np,), 7.0, device=DEV) if own else raw_in)
            K.z2f_post_bwd(dp2, dz1, dq2, dz2f, pert, slot, eps, p2, Q2, coef, raw, kl_min, dz1b, L, B, Np, prior=(pc, praw),
                           kl_out=kl_out if own else None, seg=(seg_src[:, :Z], seg_ptr, 0.5), z1_dz2f=-1.0)
            record('z2f_post_bwd/Z%d/kl_min=%r/own%d' % (Z, kl_min, own), pb, zb, qb, kl_out, raw)
        (pb, dp2), (zb, dz1) = padded(L * B, 2 * Z), padded(L * B, Z, seed=12)
        K.z2f_post_bwd(dp2, dz1, None, None, None, slot, eps, p2, Q2, coef, raw_in, 0.0, None, L, B, 0)
        record('z2f_post_bwd/Z%d/no_pairs' % Z, pb, zb)
    # dv_reparam_bwd_seg with a dv_prior_kl: the gate above, below and on the tie
    nq, Z, R_, F_ = 7, 37, 20, 9
    Q = rnd(nq + 2, 2 * Z, seed=1, scale=0.5)
    dz, eps, extra = rnd(R_, Z, seed=2), rnd(R_, Z, seed=3), rnd(F_, 2 * Z, seed=4)
    rs = np.random.RandomState(5)
    sp = i32(np.concatenate([[0], np.cumsum(rs.randint(0, 4, nq))]))
    sr = i32(rs.randint(0, R_, int(sp[-1])))
    ep = i32(np.concatenate([[0], np.cumsum(rs.randint(0, 3, nq))]))
    er = i32(rs.randint(0, F_, int(ep[-1])))
    raw, coef = rnd(nq, seed=6).abs() * 40, rnd(nq, seed=7)
    for beta in (0.0, 1.0):
        gb, got = padded(nq, 2 * Z, seed=8)
        K.reparam_bwd_seg(got[:, :Z], got[:, Z:], dz, eps, Q[:nq, Z:], sp, sr, extra=extra, ex_ptr=ep, ex_rows=er, beta=beta,
                          prior=(coef, raw, float(raw[2]), Q[:nq, :Z]))
        record('reparam_bwd_seg/prior/beta%d' % beta, gb)


# ------------------------------------------------------------------------------------------------- clamp(softmax)
def softmax_cases(K):
    M = 9
    for Y, sig in ((2, False), (8, False), (2, True)):
        logits = rnd(M, Y + 1, seed=1, scale=3.0)[:, :Y]
        logits[0, 0], logits[0, 1] = 60.0, -60.0          # one class onto each clamp
        logits[1, 0], logits[1, 1] = -60.0, 60.0
        pb, probs = padded(M, Y)
        K.softmax_clamp_fwd(probs, logits, sigmoid1=sig)
        record('softmax_clamp_fwd/Y%d/sig%d' % (Y, sig), pb)
        dprobs = rnd(M, Y, seed=2)
        for beta in (0.0, 1.0):
            W = 1 if sig else Y
            db, dl = padded(M, W, seed=3)
            K.softmax_clamp_bwd(dl, dprobs, probs, sigmoid1=sig, beta=beta)
            record('softmax_clamp_bwd/Y%d/sig%d/beta%d' % (Y, sig, beta), db)


# ------------------------------------------------------------------------------------------------- Philox fills, counters
def fill_cases(K):
    ctrs = {'ctr0': [0, 0], 'ctr_carry': [-1, 1]}          # {0xFFFFFFFF, 1}
    for n in (1, 6, 1025):
        for tag, c in ctrs.items():
            out = torch.full((n + 3,), 7.0, device=DEV)
            K.fill_normal(out[:n], 0x1234567887654321, i32(c))
            record('fill_normal/n%d/%s' % (n, tag), out)
    out = torch.full((9,), 7.0, device=DEV)
    K.fill_normal(out[:6], 99)
    record('fill_normal/n6/no_ctr', out)
    # 5 normal + 3 keep rows, widths {1, 4, 7, 130}, row 3 at an unaligned offset
    widths, off, rows = [1, 4, 7, 130, 4, 130, 7, 1], 0, []
    for r, w in enumerate(widths):
        if r == 3:
            off += 1
        rows.append([off, w, r % 3, 100 + r])
        off += (w + 3) // 4 * 4
    desc, total = i32(rows), off + 4
    for tag, c in ctrs.items():
        for lo in (0, 2):
            arena = torch.full((total,), 7.0, device=DEV)
            K.fill_normal_rows(arena, desc[lo:5], 0xABCDEF0123456789, i32(c))
            record('fill_normal_rows/%s/from%d' % (tag, lo), arena)
            for rate in (0.5, 0.0):
                table = K.noise_table(desc, 5, K.keep_threshold(rate))
                arena = torch.full((total,), 7.0, device=DEV)
                K.fill_noise_rows(arena, table[lo:], 0xABCDEF0123456789, i32(c))
                record('fill_noise_rows/%s/from%d/rate%s' % (tag, lo, rate), arena)


def counter_cases(K):
    one, two = i32([-1]), i32([-3, 1])                   # across the 32-bit carry: 0xFFFFFFFF + 3, {0xFFFFFFFD, 1} + 5
    K.counter_add(one, 3)
    K.counter_add(two, 5)
    record('counter_add', one, two)
    for pub in (False, True):
        c1, c2, flag = i32([0x7FFFFFFF]), i32([-2, 7]), i32([0])
        K.counters_add2(c1, 1, c2, 4, publish=(flag, c2, 2) if pub else None)
        record('counters_add2/pub%d' % pub, c1, c2, flag)
    # a wait on a flag that is already published (5 >= 4 + 1), with a publish of its own; err[1] (ticks parked) is a clock
    flag, ctr, err, flag2, ctr2 = i32([5]), i32([4]), i32([0, 0]), i32([0]), i32([40])
    K.flag_wait(flag, ctr, err, 1, publish=(flag2, ctr2, 2))
    record('flag_wait/published', flag, err[:1], flag2)


# ------------------------------------------------------------------------------------------------- train steps
def step_cases(K):
    from drvae_amd import engine as E
    from drvae_amd.arena import ParamArena
    from oracle import models_ref as M
    configs = [('drvae', 'adam', {}), ('pvae', 'adam', {}), ('vfae', 'adam', {}),
               ('drvae', 'adamw', dict(max_grad_norm=1.0, ema_decay=0.9, anneal_learning_rate=True, anneal_lr_itermax=3)),
               ('drvae', 'adamax', {})]
    B = 12
    for kind, alg, extra in configs:
        spec = M.ModelSpec(kind=kind, dim_x=64, dim_z1=16, dim_z3=12, h_en_z1=[48], h_de_z1=[24], h_en_z3=[24], h_de_x=[40],
                           L=2, optim_alg='adam' if alg == 'adamw' else alg)
        kw = {k: getattr(spec, k) for k in E.StepConfig.__dataclass_fields__ if hasattr(spec, k)}
        kw.update(extra, optim_alg=alg)
        cfg = E.StepConfig(**kw)
        arena = ParamArena(E.param_shapes(cfg), DEV, frozen=E.frozen_params(cfg))
        arena.load(M.init_params(spec, 5, as_numpy=True))
        eng = E.FusedStep(cfg, arena, seed=777)
        batch = M.make_batch(spec, B, seed=3)
        if kind != 'vfae':               # 5 pairs
            hx = np.zeros(B, np.int64)
            hx[[1, 4, 5, 8, 11]] = 1
            batch['x2'] = (batch['x1'] + 0.1 * np.random.RandomState(4).standard_normal(batch['x1'].shape)).astype(np.float32)
            batch['x2'] *= hx[:, None].astype(np.float32)
            batch['has_x2'] = hx
        if kind != 'pvae':               # mixed labels
            batch['has_y'] = (np.arange(B) % 3 != 1).astype(np.int64)
        t = lambda k: torch.from_numpy(batch[k].copy()).to(DEV)
        eng.set_batch(t('x1'), t('x2'), batch['y'], batch['has_x2'], batch['has_y'])
        losses = []
        for _ in range(3):
            eng.train_step()             # (Philox noise: the row fills are part of the step)
            losses.append(eng.arena.loss.detach().clone())
        outs = [arena.param, arena.exp_avg, arena.exp_avg_sq] + ([arena.avg] if hasattr(arena, 'avg') else []) + losses
        name = 'train_step/%s/%s%s' % (kind, alg, '/clip_ema_lr' if extra else '')
        record(name, *outs)
        print(name, 'losses of step 3:', [round(v, 4) for v in losses[-1].tolist()])


def main(argv):
    if argv and argv[0] == '--diff':
        a, b = (json.load(open(f)) for f in argv[1:3])
        bad = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
        print('%d cases, %d differ' % (len(set(a) | set(b)), len(bad)))
        for k in bad:
            print('  DIFFERS', k)
        return 1 if bad else 0
    global DEV
    DEV = torch.device('cuda:0')
    import drvae_amd.kernels as K
    from drvae_amd import _lib
    _lib.load()
    for fn in (ymarg_cases, smalln_cases, kl_cases, z2f_cases, softmax_cases, fill_cases, counter_cases, step_cases):
        fn(K)
    out = json.dumps(CASES, indent=0, sort_keys=True)
    if argv:
        with open(argv[0], 'w') as fh:
            fh.write(out + '\n')
    print('%d cases from %s' % (len(CASES), os.environ.get('DRVAE_HIP_LIB', _lib.LIB_PATH)))
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
