"""CPU, world_size 2 over gloo: the data-parallel train step of a negative-binomial model with the depth-normalised encoder
input (``x_transform='log1p_norm'``, ``library_size=True``: the row's own total is row-local) reproduces the single-process step
on the concatenated batch -- ``tests/test_counts_dp_gloo.py`` with the normalised feed."""
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oracle import models_ref as M
from tests.test_counts_dp_gloo import _case
from tests.test_dp_gloo import _free_port

SW = dict(type_rec='nb', x_transform='log1p_norm', library_size=True)


def _install_refs():
    import drvae_amd.kernels as K
    from tests import kernel_ref as R
    for name in R.FUNCTIONS:
        setattr(K, name, getattr(R, name))


def _run_steps(spec, params, batch, noises, counts, allreduce, lo=None, hi=None):
    from tests.test_nb_cpu import make_engine
    if lo is not None:
        batch = {k: v[lo:hi] for k, v in batch.items()}
        noises = [M.slice_noise(n, lo, hi) for n in noises]
    eng, arena = make_engine(spec, params, **SW)
    t = lambda k: torch.from_numpy(batch[k].copy())
    eng.set_batch(t('x1'), t('x2'), batch['y'], batch['has_x2'], batch['has_y'], counts=counts)
    assert eng.plan.XT is not None
    out = []
    for noise in noises:
        eng.train_step(noise, allreduce=allreduce)
        out.append(arena.loss.clone().numpy())
    return np.stack(out), arena.param.clone().numpy(), arena.grad.clone().numpy()


def _worker(rank, world, port, kind, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    torch.set_num_threads(1)
    _install_refs()
    from drvae_amd import dist as D
    r, w, _ = D.init_from_env(backend='gloo')
    assert (r, w) == (rank, world)
    spec, batch, noises, params = _case(kind)
    n = batch['x1'].shape[0]
    lo, hi = D.shard_rows(n, rank, world)
    counts = D.global_counts(batch['has_x2'][lo:hi], batch['has_y'][lo:hi], kind, spec.semi_supervised)
    res = _run_steps(spec, params, batch, noises, counts, D.allreduce_sum, lo, hi)
    q.put((rank, counts) + res)
    import torch.distributed as dist
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize('kind', ['drvae', 'vfae'])
def test_two_ranks_equal_one_rank_with_the_normalised_feed(kind, monkeypatch):
    from tests import kernel_ref
    kernel_ref.install(monkeypatch)
    spec, batch, noises, params = _case(kind)
    single = _run_steps(spec, params, batch, noises, None, None)
    assert kernel_ref.CALLS['norm_feed'] > 0 and kernel_ref.CALLS['lib_rows'] > 0 and np.isfinite(single[1]).all()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, kind, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted([q.get(timeout=180) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    n = batch['x1'].shape[0]
    want_counts = (n, int(batch['has_x2'].sum()), int(batch['has_y'].sum()))
    for rank, counts, losses, prm, grad in got:
        assert tuple(counts) == want_counts
        np.testing.assert_allclose(losses, single[0], rtol=1e-5, atol=1e-6)      # summed loss tail == global loss
        np.testing.assert_allclose(grad, single[2], rtol=1e-4, atol=1e-6 * np.abs(single[2]).max())
        np.testing.assert_allclose(prm, single[1], rtol=1e-5, atol=1e-6)
    np.testing.assert_array_equal(got[0][3], got[1][3])                          # replicas stay bit-identical
