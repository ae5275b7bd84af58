"""Developer switches of the train step's launch schedule.  NOT part of the user surface: every default is the
measured best on MI355X ("Step scheduling"); a switch is kept only where a test, ``bench.py`` or a tool in
tools/ sets another value, and only those values are accepted.  One variable carries them all::

    DRVAE_TUNE="sched=3" python bench.py

User-facing environment variables (the whole list): DRVAE_HIP_LIB (another build of the library), DRVAE_SIDE_CUS
(compute units reserved for the side chain; 0 = no partition), DRVAE_WAIT_SPINS (bound of a device-side wait),
DRVAE_DIST_BACKEND (torch.distributed backend of the data-parallel step; default nccl = RCCL on a GPU),
DRVAE_FORCE_DP=1 (the multi-rank step path over a one-rank communicator: functional check on a one-GPU box)."""
import os

# (``fuse_heads`` / ``raw_heads`` / ``nll_cs``: read in ONE place, ``schedule.heads_route`` and its static part ``heads_static``)
DEFAULTS = {
    'sched': 5,          # 5 two graphs ordered by device flags | 3 one graph, one fork/join per step (tools/pmc_collect.sh)
    'fuse_heads': 1,     # samples / NLL forward+backward in the epilogue of the heads' GEMM (dv_gemm_heads); -> schedule.heads_route
    'raw_heads': 1,      # chip-filling decoder heads (train step) as a plain product, finished by the NLL row pass (2: at any size -- tests); -> schedule.heads_route
    'tail_gate': 1,      # the side chain's tail is awaited by the NEXT step's first launch where that is a graph-resident feed (2: any first launch -- tests)
    'concurrent': 1,     # side chain at all (0: one stream)
    'nll_cs': 1,         # chip-filling heads: their bias gradient folded into the NLL row pass (no column-sum pass of its own; 2: buffers at any size -- tests, with raw_heads=2); -> schedule.heads_route
    'mmd_explicit': 1,   # model-level MMD penalty (use_s extension, rbf_fourier / identity kernels) as explicit launch lists, no autograd inside the step (0: the block-level operators -- tests)
    'fold_rows': 1,      # the pairs' KL rows formed by ``z2f_post_bwd``, the classifier's data gradient by its forward launch (0: launches of their own -- tests, A/B); -> schedule._step_tail
    'dp_fork': 1,        # captured gradient exchange: the side chain draws the next step's noise behind the join (as in the single-GPU step)
}

# the values a switch accepts: the default and the ones a test or tool sets
CHOICES = {'sched': (3, 5), 'fuse_heads': (0, 1), 'raw_heads': (1, 2), 'tail_gate': (1, 2), 'concurrent': (0, 1),
           'nll_cs': (1, 2), 'mmd_explicit': (0, 1), 'dp_fork': (0, 1), 'fold_rows': (0, 1)}


def _parse():
    out = dict(DEFAULTS)
    for kv in filter(None, os.environ.get('DRVAE_TUNE', '').split(',')):
        k, _, v = kv.partition('=')
        k = k.strip()
        if k not in DEFAULTS:
            raise ValueError('DRVAE_TUNE: unknown switch %r (known: %s)' % (k, ', '.join(sorted(DEFAULTS))))
        out[k] = int(v)
        if out[k] not in CHOICES[k]:
            raise ValueError('DRVAE_TUNE: %s=%d is not a schedule (known: %s)' % (k, out[k], CHOICES[k]))
    return out


_VALUES = None


def get(name):
    global _VALUES
    if _VALUES is None:
        _VALUES = _parse()
    return _VALUES[name]


def reload():
    """re-read DRVAE_TUNE (tests that change the environment)"""
    global _VALUES
    _VALUES = None
