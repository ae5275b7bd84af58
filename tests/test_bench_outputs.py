"""bench.py --dump-outputs on the host: what a caller of the timed step receives (loss scalars, trained parameters),
and the fixed, seeded sample that keeps a large model's outputs under the size budget."""
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


class _Arena:
    def __init__(self, seed=0):
        g = torch.Generator().manual_seed(seed)
        self.shapes = OrderedDict([('enc.weight', (50, 30)), ('enc.bias', (50,)), ('dec.W_mu', (7, 3))])
        # (a row-padded weight, as the arena stores one whose inner dimension is no multiple of 4)
        self._t = {'enc.weight': torch.randn(50, 32, generator=g)[:, :30], 'enc.bias': torch.randn(50, generator=g),
                   'dec.W_mu': torch.randn(7, 3, generator=g)}

    def p(self, name):
        return self._t[name]


class _Engine:
    def losses(self):
        return OrderedDict([('RECL', 1.5), ('KLD', 0.25), ('ELBO', -3.125)])


def test_outputs_are_the_losses_and_the_whole_parameters(tmp_path):
    arena = _Arena()
    out = bench.snapshot_outputs(_Engine(), arena)
    assert sorted(out) == sorted(['loss_RECL', 'loss_KLD', 'loss_ELBO', 'param_enc.weight', 'param_enc.bias',
                                  'param_dec.W_mu'])
    assert out['loss_ELBO'].dtype == np.float64 and float(out['loss_ELBO']) == -3.125
    for name in arena.shapes:
        assert out['param_' + name].dtype == np.float32
        assert np.array_equal(out['param_' + name], arena.p(name).numpy())
    bench.write_outputs(out, str(tmp_path / 'd'))
    assert sorted(os.listdir(tmp_path / 'd')) == sorted(k + '.npy' for k in out)
    assert np.array_equal(np.load(tmp_path / 'd' / 'param_enc.weight.npy'), arena.p('enc.weight').numpy())


def test_large_outputs_are_a_fixed_sample_within_the_budget(monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_BUDGET_BYTES', 4 * 600)
    arena = _Arena()
    a, b = bench.snapshot_outputs(_Engine(), arena), bench.snapshot_outputs(_Engine(), _Arena())
    assert sum(v.nbytes for v in a.values()) <= 4 * 600 + 4 * 3
    assert all(a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]) for k in a)     # same positions every run
    for name in arena.shapes:
        full = arena.p(name).reshape(-1).numpy()
        s = a['param_' + name]
        assert 0 < s.size < full.size and np.isin(s, full).all()
