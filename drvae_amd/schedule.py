"""How the launch sequence of the fused train step is put on the GPU: hipGraph capture / replay, the
dual-graph schedule (main chain and side chain as two single-stream graphs ordered by device flags),
the CU partition of the two chains, and the data-parallel graph splits.  Mixed into ``FusedStep``."""
import contextlib
import ctypes
import gc
import os
import weakref
from typing import NamedTuple

import torch

from . import kernels as K
from . import tuning as T


def _masked_stream(bits, device):
    """a HIP stream whose kernels only run on the CUs set in ``bits`` (hipExtStreamCreateWithCUMask),
    wrapped for torch; lives for the rest of the process"""
    hip = ctypes.CDLL('libamdhip64.so')
    st = ctypes.c_void_p()
    arr = (ctypes.c_uint32 * len(bits))(*bits)
    with torch.cuda.device(device):
        rc = hip.hipExtStreamCreateWithCUMask(ctypes.byref(st), len(bits), arr)
    if rc != 0:
        raise RuntimeError('hipExtStreamCreateWithCUMask failed: %d' % rc)
    import atexit

    def _destroy(handle=st.value):       # before the HIP runtime tears down (profilers crash otherwise)
        try:
            torch.cuda.synchronize()
            hip.hipStreamDestroy(ctypes.c_void_p(handle))
        except Exception:
            pass
    atexit.register(_destroy)
    return torch.cuda.ExternalStream(st.value, device=device)


SYNC_POLL = 64                # steps between two polls of the wait-error words

# what ``_mode()`` answers: how the pass being issued orders the step's two chains
EVAL, FORK_JOIN, DUAL = 'evaluation pass', 'one graph with a fork/join', 'one chain of the dual-graph step'

# ---------------------------------------------------------------- the device-flag protocol of the dual-graph step
# The one statement of how the two single-stream graphs of a step are ordered (DESIGN.md section 6 prints the same
# table).  A flag is published with the value ``counter + add`` on entry of a launch and awaited as ``counter + add`` by
# the other chain; the main chain counts in ``step_dev``, the side chain in ``side_ctr``.  ``flags`` has one word per row
# of FLAGS, ``sync_err`` an (error, ticks parked) pair per row of SITES, in this order: the layout is part of what
# ``bench.py``, ``fit`` and the tests read (``sync_err[0::2]``).
#   (name, publishing chain, goes unawaited)      published on entry of ...; ``goes unawaited``: nothing may wait for it
FLAGS = (
    ('z1', 'main', True),       # the z2Fz1 heads launch (VFAE: the decoder's first launch): the z1 samples are final.
    #                             Unawaited by PVAE (its side chain is the tail only; the publish stays part of the
    #                             captured launch arguments)
    ('join', 'side', False),    # the first leaf launch behind the side chain's backward, else a launch of its own: every
    #                             side-chain data gradient is final
    ('z2f', 'main', True),      # the decoder's first launch, models with a perturbation function: the z2Fz1 samples are
    #                             final.  Unawaited by PVAE, as ``z1``
    ('tail', 'side', True),     # the side chain's counter launch: its tail is through.  Unawaited under a two-graph
    #                             exchange split (``replay`` orders the streams on the host); eager steps publish it from
    #                             ``optimizer_step`` for the next captured step
    ('rows', 'main', False),    # the launch behind the decoder heads' backward products: reconstruction rows final
    ('noise', 'main', False),   # the encoder backward's first launch: this step's noise has no reader left
    ('clf_dw', 'side', False),  # the wait launch of site ``rows``: the classifier's dW is through
    ('unused', None, False),    # (allocated: the layout of ``flags`` stays)
)
#   (name, waiting chain, flags awaited)           the launch that waits
SITES = (
    ('join', 'main', ('join',)),               # park of ``z2f_post_bwd``, else ``loss_assemble(after=...)``
    ('z1', 'side', ('z1',)),                   # the side chain's first launch, a ``flag_wait``
    ('z2f', 'side', ('z2f',)),                 # park of ``smalln_fwd`` / of the pairs' KL rows, else a ``flag_wait``
    ('adam_gate', 'main', ('tail', 'clf_dw')),   # the optimiser sweep's gated slice; ``clf_dw`` when the tail is gated
    ('rows', 'side', ('rows',)),               # the ``flag_wait`` in front of the tail's Adam half / loss scalars
    ('noise', 'side', ('noise',)),             # the ``flag_wait`` in front of the draw-ahead
    ('next_step', 'main', ('tail',)),          # tail-gated step: the NEXT step's first launch waits for the previous tail
)
FLAG_INDEX = {f[0]: i for i, f in enumerate(FLAGS)}
SITE_INDEX = {s[0]: i for i, s in enumerate(SITES)}


class StepSync:
    """the flag and error words of one engine, asked by the names of FLAGS / SITES"""
    # (so a wait cannot be built with another site's error slot, or for a flag its site does not await)

    def __init__(self, device):
        self.flags = torch.zeros(len(FLAGS), dtype=torch.int32, device=device)
        self.err = torch.zeros(2 * len(SITES), dtype=torch.int32, device=device)

    def flag(self, name):
        return self.flags[FLAG_INDEX[name]:FLAG_INDEX[name] + 1]

    def pub(self, name, ctr, add=1):
        return K.Publish(self.flag(name), ctr, add)

    def wait(self, site, ctr, add=1, max_spins=None, flag=None):
        i, flags = SITE_INDEX[site], SITES[SITE_INDEX[site]][2]
        assert flag is None or flag in flags, (site, flag)
        return K.Wait(self.flag(flag or flags[0]), ctr, self.err[2 * i:2 * i + 2], add, max_spins)

    def gate(self, flag, ctr, lo, hi):
        w = self.wait('adam_gate', ctr, 0, flag=flag)        # (the step counter is advanced before the sweep: counter + 0)
        return K.Gate(w.flag, w.ctr, w.add, w.err, lo, hi)


class Tail(NamedTuple):
    """what the side chain of a recorded step carries behind the join (``_step_tail``); default: no dual-graph step"""
    dual: bool = False             # two flag-ordered graphs
    late: bool = False             # the step's leaf work (classifier dW, ...) runs behind the join
    adam_gated: bool = False       # ... so the optimiser sweep gates the classifier's slice on a flag
    side_adam: bool = False        # ... and the decoder heads' half of the sweep runs on the side chain,
    hs: int = 0                    #     which starts at this element of the arena
    side_loss: bool = False        # ... and the loss scalars
    cap_fork: bool = False         # captured exchange: the side chain draws ahead behind the join
    tail_gated: bool = False       # the NEXT step's first launch waits for the tail, the sweep for the classifier's dW only
    noise_ahead: bool = False      # the side chain draws the NEXT step's noise
    klz2_on_main: bool = False     # the pairs' KL(q(z2|x2)||p(z2|z1)) rows run on the main chain
    fold_join: bool = False        # the join rides on its first consumer (``z2f_post_bwd`` parks)
    late_fork: bool = False        # one-graph chip-filling step: the side chain forks behind the decoder heads' product
    fold_rows: bool = False        # no launch for the pairs' KL rows (``z2f_post_bwd`` forms them) nor for the classifier's
    #                                data gradient (it leaves ``smalln_fwd``; ``z2f_post_bwd`` sums the fprop rows' d/dz1)


# the kinds of pass ``heads_route`` tells apart: forward with its backward fused behind it (``fuse_bwd``) | forward of a
# training-mode loss whose backward is a call of its own | evaluation forward
TRAIN, LOSS, EVALUATE = 'train pass', 'loss pass, separate backward', 'evaluation pass'
# the launch that writes a pass's reconstruction rows (``HeadsRoute.nll``) -> the plan buffer that receives them; the
# table in DESIGN.md section 6 says when each is taken
NLL_ROUTES = {'heads': 'NLLP', 'rec': 'NLL', 'raw_cs_eval': 'NLLC', 'raw_eval': 'NLL', 'raw_cs': 'NLLC', 'fwdbwd': 'NLL',
              'fwd': 'NLL'}
# ... and beside that table (``tests/test_heads_route_cpu.py`` holds every key of it to a 'gene-cell' configuration that takes
# it): the one route of the ``dispersion='gene'`` models -- ``gene_rows`` at every size, per-chunk partials into ``NLLG``
GENE_ROUTE, GENE_ROWS = 'gene', 'NLLG'


class HeadsRoute(NamedTuple):
    """how one pass runs its dual-head layers and its reconstruction rows (``heads_route``)"""
    sample_epi: bool           # the samples of q(z1|x) and of the perturbation function leave their heads' launches
    fprop_from_heads: bool     # ... and the encoder's epilogue also fills the z1 columns of the fprop input
    z3_in_heads: bool          # the q(z3|z1,y) sample leaves its heads' launch
    fprop_tail: bool           # the fprop rows' KL forward + the z1 term's backward ride on the classifier launch (``dv_fprop_kl``)
    nll: str                   # a key of NLL_ROUTES: the launch that writes the reconstruction rows
    rows: str                  # ... and the plan buffer that holds them: 'NLLP' | 'NLLC' | 'NLL'
    raw_last: bool             # the decoder's heads run as a plain product, finished by that row pass (``_Chain.forward``)
    x3: bool                   # ... as split-bf16 products, with the gradient pair behind them (the rung: ``_Chain.x3_parts``)
    db_done: bool              # the heads' bias gradient is written by the row pass (``colsum``), not by the dW launch


def heads_static(cfg, c_decx, dpx):
    """the part of ``heads_route`` a plan's buffers follow: (small, raw heads allowed, NLLC / NLLWS exist)"""
    # small: the paired-heads launch (32 x (32+32) tiles) is for the latency-bound sizes; once the decoder heads alone fill
    # the chip with 128x128 tiles many times over (wide configuration) the plain product + row pass wins.  The other two are
    # predicates of their own (the buffers do not ask for a raw-capable layer, raw heads not for 4 | genes) that meet in the
    # ``raw_cs`` routes
    gauss = cfg.type_rec == 'diag_gaussian'
    small = ((dpx.shape[0] + 127) // 128) * ((dpx.shape[1] + 127) // 128) < 1024
    raw_ok = bool(gauss and c_decx.raw_softplus_ok() and (not small or T.get('raw_heads') == 2))     # (2: any size -- tests)
    nll_cs = bool(gauss and cfg.dim_x % 4 == 0 and dpx.shape[0] > 0 and (T.get('nll_cs') == 2 or not small))
    return small, raw_ok, nll_cs


def heads_route(eng, plan, kind):
    """THE decision of how a pass of ``kind`` (TRAIN | LOSS | EVALUATE) over ``plan`` runs its heads: a ``HeadsRoute``"""
    # a function of the configuration, the plan and the tuning switches ``fuse_heads`` / ``raw_heads`` / ``nll_cs`` alone:
    # every reader (forward, backward, the loss scalars, either chain of a recorded step) asks it and gets the same answer
    cfg, p, train, gauss = eng.cfg, plan, kind == TRAIN, eng.cfg.type_rec == 'diag_gaussian'
    small, raw_ok, nll_cs = heads_static(cfg, p.c_decx, p.DPX)
    assert nll_cs == (p.NLLC is not None), 'the tuning switches changed since the plan was built'
    epi = bool(eng.fuse_heads and small)
    fprop = bool(cfg.has_y and not cfg.cont and p.Mf)
    # (an EVALUATION pass takes the raw heads too -- whole-set evaluation: the heads are needed for the row terms only; a
    # loss pass leaves finished heads for the backward call that follows it)
    raw_last = bool(raw_ok and not (train and epi) and kind != LOSS)
    if gauss and train and epi:      # train step: the heads' launch emits the rows' partials and d/d(mu, pre-softplus)
        nll = 'heads'
    elif cfg.rec.gene:               # 'nb' / 'zinb' with a gene-wise theta, at every size (``gene_rows``: per-chunk partials)
        nll = GENE_ROUTE
    elif not gauss:                 # Bernoulli / Poisson / (zero-inflated) negative-binomial rows, at every size (``dv_rec_nll_rows``)
        nll = 'rec'
    elif raw_last and nll_cs:        # the row pass finishes the heads (+ in a train step: their bias gradient's column sums)
        nll = 'raw_cs' if train else 'raw_cs_eval'
    elif raw_last:                   # (gene counts that are no multiple of 4 -- 978: the wave-per-row passes, with bias)
        nll = 'fwdbwd' if train else 'raw_eval'
    else:
        nll = 'fwdbwd' if train else 'fwd'
    # (``z3_in_heads``: evaluation passes over many fprop rows -- whole-set evaluation: 24576 -- take the plain product + row pass)
    return HeadsRoute(sample_epi=epi, fprop_from_heads=bool(epi and fprop),
                      z3_in_heads=bool(eng.fuse_heads and (train or p.Mf < 8192)),
                      fprop_tail=bool(train and eng.fuse_heads and fprop and eng.clf_small), nll=nll,
                      rows=GENE_ROWS if nll == GENE_ROUTE else NLL_ROUTES[nll],
                      raw_last=raw_last, x3=bool(raw_last and p.c_decx.x3_last), db_done=nll == 'raw_cs')


_PINNED_POOL = []           # pinned int32 buffers of retired engines (see ``_poll_sync``)
_PARTITION_STREAMS = {}      # device index -> {reserved CUs -> (main stream, side stream) | None}


class _Branch:
    """Fork/join of an independent launch chain onto a side HIP stream.  Inside a hipGraph
    capture the side stream joins the capture, so the chain becomes a parallel branch of the
    graph; on CPU tensors (unit tests with stand-in launchers) it degrades to inline execution."""

    def __init__(self, device, enabled=True):
        self.on = enabled and torch.device(device).type == 'cuda'
        self.side = torch.cuda.Stream(device=device) if self.on else None
        self._forked = False

    def fork(self):
        """mark the point of the current stream the side chain depends on; the chain itself may be
        recorded later (``with branch:``).  Measured on MI355X (tools/graph_fork_probe.py): the hipGraph
        executor runs a fork/join ~30 us faster when the MAIN continuation is recorded before the side
        chain, so callers fork, record the main work, and only then the side chain."""
        if self.on:
            self.side.wait_stream(torch.cuda.current_stream())
            self._forked = True

    def __enter__(self):
        if self.on:
            if not self._forked:
                self.side.wait_stream(torch.cuda.current_stream())
            self._forked = False
            self._ctx = torch.cuda.stream(self.side)
            self._ctx.__enter__()
        return self

    def __exit__(self, *exc):
        if self.on:
            self._ctx.__exit__(*exc)

    def join(self):
        if self.on:
            torch.cuda.current_stream().wait_stream(self.side)


# what ``capture()`` leaves on the engine: kept per plan by ``stash_capture`` / swapped back in by ``use_capture``
_CAPTURE_STATE = ('_graphs', '_side_graph', 'noise_ahead', '_graph_key', '_graph_feed', '_graph_mmd_sig',
                  '_captured_allreduce', '_graph_noise')


class StepSchedule:
    """scheduling half of ``FusedStep`` (see the module docstring); relies on its forward / backward /
    optimizer_step / draw_noise and on its plan, arena and counters"""

    def _init_schedule_state(self):
        """the host-side state of the schedule, all of it: what ``capture()`` leaves (``_CAPTURE_STATE``), how the step
        being recorded is split, and the bookkeeping of replays"""
        # what capture() leaves: see _CAPTURE_STATE
        self._graphs = []                 # the captured graph(s) of the main chain, in replay order
        self._side_graph = None           # dual-graph schedule: the side chain's graph
        self.noise_ahead = False          # the side chain draws the NEXT step's noise behind the join
        self._graph_key = None            # key of the plan the graphs point into
        self._graph_feed = None           # ... its graph-resident feed at capture time
        self._graph_mmd_sig = None        # ... its nuisance-class composition (use_MMD)
        self._captured_allreduce = None   # the collective captured into the step ('captured' exchange)
        self._graph_noise = None          # the ``add_noise`` the graphs were captured with (None: any; set by fit)
        self._captures = {}               # plan key -> the above, kept by ``stash_capture``
        # the step being recorded
        self._rec = 'both'                # 'both' | the dual-graph schedule's 'main' / 'side' chain (``_recording``)
        self._tail = Tail()               # ... and what its side chain carries
        self._after_decoder_bwd = None    # graph split point of the overlapped exchange
        # (the next two count device-side EVENTS across launches -- draws not yet added to the Philox counter, a counter
        # bump that rode on an earlier launch of the step: state by nature, unlike what ``heads_route`` / ``_step_tail``
        # answer; untangling them is a piece of work of its own)
        self._rng_pending = 0             # Philox draw events not yet added to the counter
        self._ctr_bumped = False          # the loss-scalar launch has advanced the step / Philox counters
        # replays
        self._noise_stale = True          # the noise buffer does not hold the draws of the current Philox counter
        self._flag_side = None            # the stream the side graph is launched on (``flag_side``)
        self._flags_ok = None             # None: not probed yet (``_flags_usable``)
        self._side_cus = None             # CUs reserved by ``tune_partition`` (None: DRVAE_SIDE_CUS / 64)
        self._since_poll = 0
        self._sync_host = None            # pinned landing buffer of the error words: from the pool on first poll
        self._sync_event = None

    # ------------------------------------------------ several captured plans side by side
    def stash_capture(self):
        """remember the graphs just captured for the current plan (a feed that switches between a few plans from step
        to step -- ``DeviceBatcher(pair_bucket=...)`` -- captures each once and swaps them with ``use_capture``)"""
        assert self._graph_key == self.plan.key, 'stash_capture right after capture(): another plan is current'
        self._captures[self.plan.key] = {k: getattr(self, k) for k in _CAPTURE_STATE}

    def use_capture(self, key):
        """make the plan ``key`` and its captured graphs current; False when it has not been captured yet"""
        cap = self._captures.get(key)
        if cap is None or cap['_graph_feed'] is not self._plans[key].live_feed or \
                cap['_graph_noise'] not in (None, self.add_noise):
            return False
        if self._graph_key != key:
            for k, v in cap.items():
                setattr(self, k, v)
            self.plan = self._plans[key]
            # the side chain drew ahead into the OTHER plan's noise buffer: the replay draws for this one first (in front
            # of the main graph; drawn on the side stream with an event edge instead, the step is 2 % slower)
            self._noise_stale = True
        return True

    def _mode(self):
        # (eager steps of the dual-graph schedule fork and join, too)
        return EVAL if not self.fuse_bwd else DUAL if self._rec != 'both' else FORK_JOIN

    def _step_tail(self, split_kind, on_gpu=None):
        """how the train step of the current plan is recorded under the exchange form ``split_kind``: a ``Tail``"""
        # ``split_kind``: False | True (two graphs) | 'overlap' | 'captured'.  Decided HERE, once per recording (``capture``),
        # and read by forward / backward / the side chain's tail: copies of a condition that disagree deadlock the step into
        # a wait time-out.  ``on_gpu``: what the device contributes -- a side stream on a hardware queue of its own; None:
        # ask it (CPU tests of the recorded sequence pass True)
        cfg, p = self.cfg, self.plan
        branch_on = self.branch.on if on_gpu is None else bool(self.concurrent and cfg.has_y and on_gpu)
        # gradient-norm clipping (``StepConfig.max_grad_norm``): the norm launch in front of the sweep reads EVERY gradient, so
        # nothing of the backward pass may still be in flight behind the join and the sweep has no gated or side-chain form:
        # the single-process step is recorded the way the exchange forms record theirs.  Decided here and only here (the
        # sweep asserts it)
        clip = cfg.max_grad_norm is not None
        # two flag-ordered graphs only for the latency-bound steps: once the decoder products alone fill the chip many
        # times over (wide configuration) the side chain's small kernels, squeezed in between the resident GEMM
        # workgroups of a second queue, cost more than they hide (36.7 ms dual, 35.9 ms as one graph with a fork/join)
        # (not PVAE under a gradient exchange: its side chain is the step's tail only (optimiser half, loss scalars, noise);
        # the optimiser half cannot move there then and the rest does not pay for the second graph -- one-rank RCCL, cfg 1:
        # 0.1848 -> 0.1913 split, 0.1695 -> 0.1737 captured)
        if not (self.sched == 5 and self._dual_capable(on_gpu) and self._latency_bound() and
                (self._flags_usable() if on_gpu is None else on_gpu) and (cfg.has_y or not (split_kind or clip))):
            # ONE graph.  A chip-filling step (wide configuration): its side chain is 0.5 ms of small launches next to 31 ms of
            # products that want every CU.  Forked at the start of the step they squeeze in between the resident GEMM workgroups
            # of the other queue and cost more than they hide (round 4: 32.0 ms with the fork/join, 31.5 ms in order on one
            # stream); forked LATE -- behind the decoder heads' product, next to the HBM-bound NLL row pass, the one stretch of
            # the main chain that leaves the matrix pipes idle -- and joined behind the decoder's backward products, they win
            # (round 6, cfg 5: 31.09-31.15 -> 30.87-30.89 ms; the side chain's 0.4 ms are through long before the join)
            return Tail(late_fork=bool(branch_on and not self._latency_bound()))
        # the side chain carries the step's leaf work (classifier dW, heads' optimiser half, loss scalars) behind the join
        late_ok = bool(not cfg.cont and cfg.optim_alg in ('adam', 'adamw') and (self.clf_small if cfg.has_y else True))
        # (dual-graph schedule) the classifier's weight gradient is a leaf -- only the optimiser reads it --
        # and the side chain is the one the join waits for: it runs AFTER the side chain has published its
        # data gradients, and the optimiser launch gates that slice of the arena on a flag of its own
        # Under data parallelism every gradient (and the loss tail) must be final before the exchange: with the plain
        # two-graph split ``replay`` makes the launching stream wait for the side stream before the all-reduce, so the
        # leaf work may still move behind the join (only the optimiser half cannot: it follows the exchange); the
        # overlapped / captured exchanges keep everything in front of the join
        # (a clipped step without an exchange: like those -- with the two-graph split the side stream is awaited in front of
        # the exchange and the sweep is a graph of its own, nothing is in flight there)
        late = late_ok and (split_kind is True or (split_kind is False and not clip))
        # ... and HALF of the optimiser sweep moves there too: the decoder heads (the tail of the arena, half of
        # all parameters) are final and no longer read once the heads' backward products are through -- the
        # launch after them publishes that -- so the side chain updates them next to the main chain's tail
        side_ok, hs = self._side_adam_layout()
        side_adam = late and not split_kind and side_ok
        # the gradient exchange captured INTO the step's graph (data parallelism, ``split_kind == 'captured'``): every gradient
        # and the loss scalars are final in front of the collective, so no leaf work moves behind the join -- but the side chain,
        # idle behind it, draws the NEXT step's noise (the main chain's graph then no longer starts with the draw) and the
        # sweep's first workgroup orders the next step behind that.  Measured (one-rank RCCL, same box): cfg 2 0.2042 -> 0.2007 ms,
        # cfg 4 0.1799 -> 0.1769; the heads' half of the sweep behind the collective on the side chain's 64 CUs as well
        # (a flag published on entry of the main chain's sweep): 0.2124 / 0.1871 -- half the arena through a quarter of the
        # chip's bandwidth takes longer than the whole sweep on the rest (profiles/r06_experiments.md)
        # (not a clipped step: this form parks the sweep's first workgroup on the side chain's flag)
        cap_fork = bool(split_kind == 'captured' and side_ok and late_ok and cfg.has_y and T.get('dp_fork') and not clip)
        # the loss scalars (a leaf: only the host / the exchange reads them) are assembled by the side chain behind
        # the join, once the main chain has published that its reconstruction rows are final
        side_loss = side_adam or (late and split_kind is True and len(self.L_decx) > 1)
        # tail gating: dual-graph train step (ONE pair of graphs) whose side chain runs its half of the optimiser sweep (the
        # tail then holds the wait launch of site ``rows``) and the loss scalars behind the join: the optimiser launch gates on
        # the classifier's gradient only, and the NEXT step's first launch waits for the tail's end
        # ... where the step's first launch is the graph-resident feed (a few dozen workgroups that can park): sampler feed
        # 0.213 -> 0.2074 ms.  With the resident batch the first launch is the input gather (856 workgroups; parked with
        # 128 it is slower by itself and waits the 4 us the optimiser launch used to wait: 0.1932 -> 0.198 ms)
        # (an annealed plan without the feed: its head is ``dv_batch_masks`` as a launch of its own, which cannot park and
        # rewrites what the tail reads -- see ``_head_behind_tail``; the tuning switch does not reach it)
        tail_gated = side_adam and (p.live_feed is not None or (T.get('tail_gate') == 2 and not p.annealed))
        # the pairs' KL rows on the main chain (in every other schedule: on the side chain)
        # (not with the batch-independent plan: its worst-case decoder rows make the main chain the longer one again,
        # the side chain parks ~13 us per step behind it -- sampler feed 0.250 -> 0.248 ms with the rows on the side chain;
        # that is the every-row-may-be-anything plan: the bucketed ones are close to a structure plan's rows and keep the
        # rows on the main chain, sampler feed 0.2181 -> 0.2140 ms in a same-box A/B)
        klz2_on_main = not cfg.cont and cfg.has_y and not p.every_row_anything
        # the join rides on its first consumer
        # (only where the join does not wait: every workgroup of the consumer polls the flag, and a long wait -- VFAE:
        # its side chain is the longer one, 30 us/step -- slows the very chain it waits for: 0.184 -> 0.208 ms)
        # ... and only where the parked grid is a small fraction of what the chip holds resident (256 CUs x 8
        # workgroups): a consumer grid that filled the chip would leave the side chain nowhere to run
        fold_join = side_loss and cfg.has_pert and (p.B * cfg.dim_z1 + 255) // 256 <= 256 and (p.B + 3) // 4 <= 256
        # (noise drawn ahead under a CAPTURED exchange too: the side chain then draws behind the join and sweeps its half
        # behind the collective)
        # ... but not over a plan with dropout sites: the next step's draw is released when the encoder backward STARTS --
        # nothing behind that point reads the arena -- and with sites the encoder backward itself reads its keep masks there.
        # Such a step draws at its head, as under ``sched=3`` (no second arena in this round)
        noise_ahead = bool((late or cap_fork) and not p.drop_sites)
        # two launches folded into their neighbours (cfg 2: 33 -> 31 launches per step, one less on either chain): the pairs'
        # KL rows are formed by their consumer ``z2f_post_bwd`` -- ``klz2_on_main`` then has nothing left to place, and the loss
        # scalars, which read those rows, are assembled behind the side tail's wait for flag ``noise`` (published behind that
        # launch on the main chain) -- and the classifier's data gradient leaves the classifier's forward launch, which has its
        # inputs already; the fprop rows' d/dz1 is summed by ``z2f_post_bwd``.  Only the single-process dual-graph train step
        # of a DrVAE with the single-Linear classifier on [z1, z2Fz1 - z1].  Same bits as the unfolded step; cfg 2:
        # 0.1842 -> 0.1817 ms in alternating legs (profiles/r15_fold_rows.md)
        fold_rows = bool(T.get('fold_rows') and not split_kind and not clip and not p.drop_sites and cfg.kind == 'drvae'
                         and not cfg.cont and self.clf_small and cfg.clf_z1z2 and fold_join and side_loss and noise_ahead)
        t = Tail(dual=True, late=late, adam_gated=late and not split_kind, side_adam=side_adam, hs=hs, side_loss=side_loss,
                 cap_fork=cap_fork, tail_gated=tail_gated, noise_ahead=noise_ahead, klz2_on_main=klz2_on_main,
                 fold_join=fold_join, fold_rows=fold_rows)
        # annealing schedules (``StepConfig.annealed``): step t+1's FIRST launch (``dv_batch_masks``, on its own or as the
        # feed's extra workgroup) rewrites the schedule record and the ELBO / CMPL weights with NEW values, and step t's tail
        # on the side chain reads them -- its half of the sweep (lr_scale), the loss scalars (w_elbo, w_cmpl, the KLD weights).
        # No launch is added for this: the same launch has always rewritten the per-row weights those loss scalars read
        # (w_recl, w_pert, w_yl, c_klz2: they change with every batch's composition), so every recorded form already parks
        # the head of the next step on flag ``tail`` or behind a launch that did.  Checked here, where the tail is decided,
        # instead of believed (DESIGN.md section 9 gives the argument form by form)
        assert not p.annealed or self._head_behind_tail(t, split_kind), 'annealed step: the next head may overtake this tail'
        return t

    @staticmethod
    def _head_behind_tail(t, split_kind):
        """is the first launch of step t+1 ordered behind the LAST launch of step t's side chain (the one that publishes
        flag ``tail``) in the dual-graph step ``t``?"""
        if not (t.late or t.cap_fork):
            # nothing of the side chain behind the join reads a coefficient: its tail is the publish of ``join`` and its
            # counters, and the main chain's sweep is behind its own wait for ``join``
            return not (t.side_adam or t.side_loss or t.noise_ahead)
        if split_kind is True:
            return True          # two main graphs: ``replay`` makes the launching stream wait for the side stream between them
        if t.tail_gated:
            return True          # the head itself parks on ``tail`` (site ``next_step``): the feed launch, masks workgroup included
        # the sweep's gated workgroup parks on ``tail`` (site ``adam_gate``), and the head follows the whole sweep in stream order
        return bool(t.adam_gated or t.cap_fork)

    @contextlib.contextmanager
    def _recording(self, chain, tail):
        """the passes issued inside are the ``chain`` ('main' | 'side' of a dual-graph step, 'both': one graph) of the ``tail`` step"""
        self._rec, self._tail = chain, tail
        try:
            yield
        finally:
            self._rec, self._tail = 'both', Tail()

    # ------------------------------------------------------------------- hipGraph
    def _launch_sequence(self, allreduce=None, draw=True, optimizer=True):
        """the train pass: [draw] + forward + backward [+ exchange + optimiser]; the only place that sets ``fuse_bwd``"""
        self.fuse_bwd = True
        try:
            if draw:
                self.draw_noise(bump=False)
            self.forward()
            self.backward()
            if optimizer and allreduce is not None:
                allreduce(self.arena.xchg)
        finally:
            self.fuse_bwd = False
        if optimizer:
            self.optimizer_step()

    def capture(self, split_for_allreduce=False, allreduce=None):
        """Capture the train step (Philox noise + forward + backward + Adam: ~100 launches)
        into hipGraph(s) for the current batch structure.  With ``split_for_allreduce`` the
        step is captured as two graphs so that an (uncaptured) RCCL all-reduce of the
        gradient arena can run between backward and Adam; ``split_for_allreduce='captured'`` with
        ``allreduce``: the collective is captured INTO the step's graph (RCCL supports stream capture),
        no graph boundary, no host-side launch of the exchange."""
        self._refuse_averaged('capture')
        self._captured_allreduce = allreduce if split_for_allreduce == 'captured' else None
        assert self.plan is not None, 'set_batch first'
        self.join_side()
        if self.plan.DZMMD is not None and split_for_allreduce:
            raise NotImplementedError('use_MMD: the model-level MMD penalty is a cross-row term (every row of a nuisance '
                                      'class against every other row): it cannot be sharded over ranks')
        self.training = True
        self.plan.set_beta(*self.betas())
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):         # warm-up on a side stream (loads code objects)
            self.draw_noise(bump=False)       # (the Philox counter is NOT advanced: capturing leaves the stream
            self._rng_pending = 0             #  of draw events exactly where an eager step would find it)
            self.forward()
            self.backward()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self._graphs = []
        self._side_graph = None
        tail = self._step_tail(split_for_allreduce)
        self.noise_ahead = tail.noise_ahead
        self._noise_stale = True
        # no garbage collection while a stream is capturing: a collected cycle may own device or pinned memory,
        # events or graphs of a retired engine, and releasing those calls HIP functions that are illegal
        # during (global-mode) capture -- the process aborts
        gc.collect()
        gc_was_on = gc.isenabled()
        gc.disable()
        try:
            with self._recording('main' if tail.dual else 'both', tail):
                self._capture_main(split_for_allreduce)
            if tail.dual:
                self.sync_side_counters()
                self.flag_side.wait_stream(torch.cuda.current_stream())
                gs = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gs, stream=self.flag_side), self._recording('side', tail):
                    self._launch_sequence(draw=False, optimizer=False)
                self._side_graph = gs
        finally:
            if gc_was_on:
                gc.enable()
        self._graph_key = self.plan.key
        self._graph_feed = self.plan.live_feed
        self._graph_mmd_sig = getattr(self.plan, 'mmd_sig', None)
        return self

    # ------------------------------------------------------------ CU partition
    def _latency_bound(self):
        """the step's big products do not fill the chip many times over (<= 4 M elements of decoder output)"""
        return self.plan is not None and self.plan.DPX.shape[0] * self.plan.DPX.shape[1] <= (4 << 20)

    def _partition_applicable(self):
        # only for latency-bound steps: once the decoder products alone fill the chip many times over
        # (wide configuration) the main chain needs every CU (measured: 52 ms -> 66 ms/step when masked)
        small = self._latency_bound()
        # (a model without a classifier -- PVAE's tail-only side chain -- only once its step IS captured as two graphs:
        # under a gradient exchange it is not, and a masked main stream would only cost it CUs)
        if not self.cfg.has_y and self._side_graph is None:
            return False
        return bool(self.sched == 5 and self._dual_capable() and small and
                    int(os.environ.get('DRVAE_SIDE_CUS', '64')) > 0)

    def _part_streams(self, n_side):
        """(main, side) CU-masked streams reserving ``n_side`` CUs for the side chain (cached)"""
        cache = _PARTITION_STREAMS.setdefault(torch.device(self.dev).index or 0, {})   # per device, process-wide:
        n_side = int(n_side)
        if n_side not in cache:                    # masked streams own hardware queues, so engines share them
            n_cu = torch.cuda.get_device_properties(self.dev).multi_processor_count
            words = (n_cu + 31) // 32
            side_bits, all_bits = [0] * words, [0] * words
            # bit i of a CU mask = XCD i % 8, shader engine (i / 8) % 4 of it, CU i / 32 of that engine (tools/cumask_probe.hip):
            # the first n_side bits = n_side / 32 CUs of every shader engine of every XCD.  (The reserve as whole XCDs, L2s of
            # the side chain's own, was measured slower: every hand-over between the chains becomes a cross-XCD miss -- cfg 2
            # 0.199 -> 0.243 ms, profiles/r04_experiments.md)
            for i in range(n_cu):
                all_bits[i // 32] |= 1 << (i % 32)
                if i < min(n_side, n_cu - 1):
                    side_bits[i // 32] |= 1 << (i % 32)
            main_bits = [a & ~b for a, b in zip(all_bits, side_bits)]
            try:
                pair = (_masked_stream(main_bits, self.dev), _masked_stream(side_bits, self.dev))
                with torch.cuda.stream(pair[0]):
                    if not self._probe(pair[1]):         # must sit on different hardware queues
                        pair = None
            except (OSError, RuntimeError, AttributeError) as e:      # runtime without CU masking: plain streams
                import warnings
                warnings.warn('drvae_amd: CU partition unavailable (%s)' % e)
                pair = None
            cache[n_side] = pair
        return cache[n_side]

    def partition(self, n_side=None):
        """Context manager: run the train step with the GPU's compute units split between the two
        launch chains -- the side chain (many small launches) on ``n_side`` reserved CUs, the main
        chain (the big GEMMs) on the rest -- via CU-masked HIP streams.  Inside the context the
        masked main stream is the current stream, so everything the caller enqueues (batch feed,
        loss accumulation, replays) is ordered with the step; on exit the outer stream waits for it.
        Measured on MI355X (cfg 2): 64 reserved CUs take the step from 0.264 to 0.240 ms; without the
        reservation the side chain's small kernels queue behind the GEMM workgroups and the main
        chain waits ~32 us per step at the join.  ``tune_partition()`` picks the split by timing.
        No-op when not applicable, disabled (DRVAE_SIDE_CUS=0) or off-GPU."""
        import contextlib
        if not self._partition_applicable():
            return contextlib.nullcontext()
        if n_side is None:
            n_side = self._side_cus or int(os.environ.get('DRVAE_SIDE_CUS', '64'))
        pair = self._part_streams(n_side)
        if pair is None:
            return contextlib.nullcontext()
        main, side = pair

        @contextlib.contextmanager
        def ctx():
            outer = torch.cuda.current_stream()
            prev = self._flag_side
            main.wait_stream(outer)
            side.wait_stream(outer)
            self._flag_side = side
            try:
                with torch.cuda.stream(main):
                    yield self
            finally:
                outer.wait_stream(main)
                outer.wait_stream(side)
                self._flag_side = prev
        return ctx()

    def tune_partition(self, candidates=(32, 64, 96, 128), steps=24):
        """Pick the CU split of ``partition()`` by timing replays of the captured step (the best split
        depends on how the two chains balance, i.e. on the model and on the individual GPU).  Runs on a
        scratch copy of the training state: parameters, Adam moments and all device counters are restored
        afterwards.  Returns the chosen number of reserved CUs (None when partitioning does not apply).
        Candidates are multiples of 32: bit i of a CU mask is a CU of shader engine i % 32 (8 XCDs x 4), and the dispatcher
        hands every shader engine the same share of a grid -- a reserve that gives some engines one CU less makes those
        the pace of the whole side chain (cfg 2: 56 reserved CUs 0.249 ms, 64: 0.1975, 72: 0.2125; every 8th / 4th / 2nd
        bit instead of the first 64: 0.236; masks that overlap -- CUs open to both chains: 0.216-0.258)."""
        if not (self._partition_applicable() and self._side_graph is not None and len(self._graphs) == 1) or \
                'DRVAE_SIDE_CUS' in os.environ:       # (multi-rank: split graphs need the exchange; keep the default)
            return None
        a = self.arena
        state = (a.param, a.exp_avg, a.exp_avg_sq, self.step_dev, self.side_ctr, self.side_t, self.rng_ctr, self.flags)
        if self.clip_rec is not None:     # a tuning replay the guard skips counts in ``n_skipped``: it goes back with the step
            state = state + (self.clip_rec,)
        if hasattr(a, 'avg'):             # the tuning replays move the parameter average too: it goes back with the parameters
            state = state + (a.avg,)
        keep = [t.clone() for t in state]
        iters = self.iters
        best = (None, float('inf'))
        for n in candidates:
            if self._part_streams(n) is None:
                continue
            with self.partition(n):
                for _ in range(4):
                    self.replay()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(steps):
                    self.replay()
                e1.record()
                e1.synchronize()
                t = e0.elapsed_time(e1)
            if t < best[1]:
                best = (n, t)
        torch.cuda.synchronize()
        for dst, src in zip(state, keep):
            dst.copy_(src)
        self.iters = iters
        self._noise_stale = True
        self.plan.set_beta(*self.betas())
        torch.cuda.synchronize()
        self._side_cus = best[0]
        return best[0]

    @property
    def flag_side(self):
        """the stream the side-chain graph of the dual-graph schedule is launched on: CU-masked inside
        ``partition()``, otherwise a plain stream that ``_flags_usable`` has verified to sit on a
        different hardware queue than the launching stream."""
        if self._flag_side is None:
            self._flag_side = torch.cuda.Stream(device=self.dev)
        return self._flag_side

    def _probe(self, side):
        """park a short wait on the launching stream, publish from ``side``: a timeout means the two
        streams share a hardware queue (a parked wait kernel blocks everything behind it in its queue)"""
        probe = torch.zeros(4, dtype=torch.int32, device=self.dev)      # flag, counter, error, ticks
        torch.cuda.synchronize()
        K.flag_wait(probe[0:1], probe[1:2], probe[2:4], add=1, max_spins=20000)
        with torch.cuda.stream(side):
            K.flag_publish(probe[0:1], probe[1:2], 1)
        torch.cuda.synchronize()
        return int(probe[2]) == 0

    def _flags_usable(self):
        """Device-flag ordering needs the two streams on DIFFERENT hardware queues.  HIP multiplexes its
        streams onto a few queues, so probe candidates until one qualifies (the CU-masked stream of
        ``partition()`` has a queue of its own); otherwise fall back to graph edges.  (High-priority
        streams are avoided on purpose: with one in the process, captured fork/joins ran 2.4x slower.)"""
        if self._flags_ok is None:
            ok = self._probe(self.flag_side)
            tries = 0
            while not ok and tries < 8:
                self._flag_side = torch.cuda.Stream(device=self.dev)
                ok = self._probe(self._flag_side)
                tries += 1
            self._flags_ok = ok
            if not ok:
                import warnings
                warnings.warn('drvae_amd: no side stream on a hardware queue of its own; using graph edges')
        return self._flags_ok

    def check_sync(self):
        """raise if a device-side wait of the dual-graph schedule ever timed out (results would be stale)"""
        self.join_side()
        if int(self.sync_err[0::2].abs().sum()) != 0:
            self._raise_sync(self.sync_err.cpu().tolist())

    @staticmethod
    def _raise_sync(words):
        sites = ', '.join('%d %s (on the %s chain)' % ((i,) + SITES[i][:2]) for i, v in enumerate(words[0::2]) if v != 0)
        raise RuntimeError('drvae_amd: a device-side chain wait timed out (main / side stream ordering; wait site(s) %s). '
                           'From that step on the loss scalars are NaN and the optimiser leaves the parameters '
                           'untouched: the state is that of the last good step -- except when the timed-out wait was the '
                           'optimiser gate itself (site %d adam_gate): that one step is applied to every parameter but the gated '
                           'slice (the classifier head).  Restore from the last checkpoint.' % (sites, SITE_INDEX['adam_gate']))

    def _poll_sync(self):
        """Called once per replayed step.  Every ``SYNC_POLL`` steps the sticky error words of the device-side
        waits are copied to pinned host memory asynchronously; the copy issued one period earlier is checked
        first (waiting for it bounds how far the host runs ahead to two periods of queued steps, so the device
        never idles on it).  A timed-out wait therefore raises within two periods even in a ``replay()`` loop
        that never reads the losses."""
        self._since_poll += 1
        if self._since_poll < SYNC_POLL:
            return
        self._since_poll = 0
        if self._sync_host is None:
            # pinned landing buffers are pooled for the life of the process: returning one to torch's host
            # allocator queries its events, which is illegal while ANY stream is capturing -- and garbage
            # collection may run in the middle of a later capture
            if _PINNED_POOL:
                self._sync_host = _PINNED_POOL.pop()
            else:
                self._sync_host = torch.zeros(self.sync_err.numel(), dtype=torch.int32).pin_memory()
                ctypes.pythonapi.Py_IncRef(ctypes.py_object(self._sync_host))   # never deallocated, not even at exit
            weakref.finalize(self, _PINNED_POOL.append, self._sync_host).atexit = False
        if self._sync_event is not None:
            self._sync_event.synchronize()
            words = self._sync_host.tolist()
            if any(words[0::2]):
                self._raise_sync(words)
        self._sync_host.copy_(self.sync_err, non_blocking=True)
        self._sync_event = torch.cuda.Event()
        self._sync_event.record()

    def _capture_main(self, split_for_allreduce):
        if split_for_allreduce == 'overlap' and self.arena.late_end < self.arena.xchg.numel():
            # three graphs: [noise .. decoder backward] | [rest of backward] | [Adam]; the exchange of the
            # decoder block is launched between the first two and travels while the second runs
            ga, gb, gc = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
            cap = torch.cuda.Stream(device=self.dev)
            cap.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(cap):
                def split():
                    ga.capture_end()
                    gb.capture_begin()
                self._after_decoder_bwd = split
                try:
                    ga.capture_begin()
                    self._launch_sequence(optimizer=False)
                    gb.capture_end()
                finally:
                    self._after_decoder_bwd = None
                gc.capture_begin()
                self.optimizer_step()
                gc.capture_end()
            torch.cuda.current_stream().wait_stream(cap)
            self._graphs = [ga, gb, gc]
        elif split_for_allreduce and split_for_allreduce != 'captured':
            g1, g2 = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
            with torch.cuda.graph(g1):
                self._launch_sequence(optimizer=False)
            with torch.cuda.graph(g2):
                self.optimizer_step()
            self._graphs = [g1, g2]
        else:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._launch_sequence(allreduce=self._captured_allreduce)
            self._graphs = [g]

    def replay(self, allreduce=None):
        """One captured train step.  New data is fed by copying into plan.x1 / plan.x2 in place."""
        self._refuse_averaged('replay')
        assert self._graph_key == self.plan.key, 'batch structure changed: capture again'
        assert self._graph_feed is self.plan.live_feed, 'input source changed (epoch feed <-> explicit batch): capture again'
        assert self._graph_mmd_sig == getattr(self.plan, 'mmd_sig', None), \
            'use_MMD: the nuisance classes of the batch changed (the penalty compares row sets): capture again'
        self.plan.set_beta(*self.betas())      # 0.01 on iteration 0, 1.0 afterwards (device-side coefficients)
        self.plan.masks_injected = False          # (the captured step draws its own keep masks)
        if self.noise_ahead and self._noise_stale:        # first replay (or an eager draw since): this step's noise
            self._fill_noise(self.plan)
            self._noise_stale = False
        # the main chain's graph goes first (the host needs ~60 us per graph launch: with the side chain's graph launched first --
        # it only parks on the z1 flag -- the step's first kernels started a launch later whenever the device had run dry: after a
        # host sync, i.e. at the head of every timed region and of every epoch; 20 steps behind a sync: 0.1905 -> 0.188 ms per
        # step, steady state 0.183 either way)
        self._graphs[0].replay()
        if self._side_graph is not None:
            with torch.cuda.stream(self.flag_side):
                self._side_graph.replay()
        if len(self._graphs) == 3:               # overlapped exchange: ``allreduce`` has start()/finish()
            a = self.arena
            w_early = allreduce.start(a.xchg[a.late_end:])
            self._graphs[1].replay()
            w_late = allreduce.start(a.xchg[:a.late_end])
            allreduce.finish(w_early)
            allreduce.finish(w_late)
            self._graphs[2].replay()
        elif len(self._graphs) == 2:
            if self._side_graph is not None:
                # the side chain's work behind the join (leaf gradients, loss scalars) must be final before the
                # exchange reads the buffer: order the side stream in front of it
                torch.cuda.current_stream().wait_stream(self.flag_side)
            if allreduce is not None:
                allreduce(self.arena.xchg)
            self._graphs[1].replay()
        self.iters += 1
        if self._side_graph is not None:
            self._poll_sync()
