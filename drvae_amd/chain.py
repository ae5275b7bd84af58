"""Linear layers bound to arena views and chains of them (trunk + head of one block) evaluated on stacked
rows with pre-allocated buffers: the GEMM-level building block of the fused train step."""
import torch

from . import kernels as K


def _pad4(n):
    return (n + 3) // 4 * 4


def _whole_rows(t):
    """is ``t`` made of whole rows of a row-padded 2-D buffer (``zeros(r, pad4(c))[:, :c]`` or a row range of one)?"""
    b = t._base
    return (b is not None and b.dim() == 2 and t.dim() == 2 and b.is_contiguous() and t.stride() == (b.shape[1], 1)
            and b.shape[1] == _pad4(t.shape[1]) and (t.storage_offset() - b.storage_offset()) % b.shape[1] == 0)


class _Lin:
    """One Linear layer (or two fused heads) bound to arena views.  ``third`` (with ``second``; the zero-inflated decoder's
    dropout-logit head): one more head behind the pair, identity activation -- ``W`` / ``b`` / ``g`` and their gradients are the
    fused (3 split, K) views, which is all the backward products need; the forward runs the pair as it runs any pair and the
    third head as one more plain Linear from the same input (``_Chain.forward``)."""

    def __init__(self, arena, wname, bname, gname=None, second=None, act='identity', act1=None, shift0=0.0,
                 shift1=0.0, third=None):
        self.tri = third is not None
        if self.tri:
            names = list(zip((wname, bname, gname), second, third))
            self.W, self.dW = arena.fused(arena.param, *names[0]), arena.fused(arena.grad, *names[0])
            self.b, self.db = arena.fused(arena.param, *names[1]), arena.fused(arena.grad, *names[1])
            self.g = arena.fused(arena.param, *names[2]) if all(names[2]) else None
            self.dg = arena.fused(arena.grad, *names[2]) if all(names[2]) else None
            self.split = arena.shapes[wname][0]
        elif second is None:
            self.W, self.dW = arena.p(wname), arena.g(wname)
            self.b, self.db = arena.p(bname), arena.g(bname)
            self.g = arena.p(gname) if gname else None
            self.dg = arena.g(gname) if gname else None
            self.split = self.W.shape[0]
        else:
            w2, b2, g2 = second
            self.W, self.dW = arena.fused(arena.param, wname, w2), arena.fused(arena.grad, wname, w2)
            self.b, self.db = arena.fused(arena.param, bname, b2), arena.fused(arena.grad, bname, b2)
            self.g = arena.fused(arena.param, gname, g2) if gname and g2 else None
            self.dg = arena.fused(arena.grad, gname, g2) if gname and g2 else None
            self.split = arena.shapes[wname][0]
        self.N, self.Kin = self.W.shape
        self.act0, self.act1 = act, (act if act1 is None else act1)
        self.shift0, self.shift1 = shift0, shift1
        dev = self.W.device
        if self.g is not None:
            self.scale = torch.empty(self.N, device=dev)
            self.norm = torch.empty(self.N, device=dev)
            self.raw = torch.empty(self.N, self.Kin, device=dev)
        else:
            self.scale = self.norm = self.raw = None


# ``StepConfig.matmul`` -> bf16 parts per operand element of the split-bf16 rungs (3: ``dv_gemm_x3``; 2, 1: ``dv_gemm_split``)
X3_PARTS = {'bf16x3': 3, 'bf16x2': 2, 'bf16x1': 1}


class _Chain:
    """trunk layers + final layer of one block evaluated on M stacked rows, with buffers.

    Inputs handed to ``forward`` whose width is no multiple of 4 must either have unpadded rows (row stride == width)
    or be WHOLE row-padded buffers with zero pads (``plan.mat``): the products then run over the padded K (``kpad`` of
    ``kernels._gemm_desc``; the arena's weights are row-padded the same way).  ``backward`` likewise runs the weight
    gradient of a single-source layer and the data gradients into its own buffers (or into a destination made of whole
    padded rows) over the padded N (``npad``): the pad columns receive the zeros they hold anyway.

    Hidden-layer dropout (``add_dropout``): a SITE is the input of layer li >= 1, the hidden activation ``out[li - 1]``.  A
    pass with ``drop=True`` writes ``outd[li - 1] = out[li - 1] * mask / keep`` behind the producing launch (one
    ``K.mask_scale``) and every consumer -- the next layer's product on whichever route, its weight gradient -- reads
    ``outd``; ``out`` stays undropped (the activation derivative is taken from it) and ``dpre[li - 1]`` is scaled in place
    by the same mask behind the data-gradient launch.  A pass with ``drop=False`` launches nothing and reads ``out``."""

    def __init__(self, layers, M, device, resid_cols=0):
        self.layers, self.M, self.resid_cols = layers, M, resid_cols
        # opt-in (``use_x3_last``, decided where the plan is built): the LAST layer's plain product (``raw_last``) and the two
        # gradient products behind it MAY run as split-bf16 products; a pass says whether they do (``forward(x3=...)``)
        # ``x3_parts``: the rung, bf16 parts per operand (3: ``dv_gemm_x3``; 2, 1: ``dv_gemm_split``) -- remembered with it
        self.x3_last = False
        self.x3_parts = 3
        self.out = [torch.zeros(M, _pad4(l.N), device=device)[:, :l.N] for l in layers]
        # gradient w.r.t. the pre-activation of every layer but the last (the caller owns that one)
        self.dpre = [torch.zeros(M, _pad4(l.N), device=device)[:, :l.N] for l in layers[:-1]]
        # dropout sites (``add_dropout``): keep masks (views the caller owns), the dropped activations, 1 / keep
        self.masks, self.outd, self.inv_keep = None, None, 1.0

    def add_dropout(self, masks, keep):
        """make every hidden activation of the chain a dropout site: ``masks[li]`` is the (M, N) keep mask of ``out[li]``
        (1.0 / 0.0, filled by the caller before a ``drop=True`` pass), ``keep`` the keep probability"""
        assert len(masks) == len(self.layers) - 1 and not self.x3_last, 'sites first, then use_x3_last'
        assert all(m.shape == o.shape for m, o in zip(masks, self.out))
        dev = self.out[0].device
        self.masks, self.inv_keep = list(masks), 1.0 / keep
        # whole-row buffers with zero pads, like ``out``: the next product runs over the padded K
        self.outd = [torch.zeros(self.M, _pad4(l.N), device=dev)[:, :l.N] for l in self.layers[:-1]]

    def _hidden(self, li, drop):
        """what the consumers of hidden activation ``li`` read in a pass"""
        return self.outd[li] if (drop and self.masks) else self.out[li]

    @staticmethod
    def _pad_ok(t):
        """may a product over ``t`` run over its padded width?  Only when the caller's contract is checkable: rows that are
        not padded at all, or WHOLE rows of a row-padded buffer (``plan.mat`` / this chain's own buffers / the arena's
        padded weights), whose pad columns are zero by construction.  A column slice of a wider buffer (``Q[:, :Z]`` with
        ld = 2 Z) has neighbours, not zeros, behind its last column (round-4 advisor)."""
        if t.dim() != 2 or t.shape[1] % 4 == 0:
            return True
        ld = t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])
        return ld == t.shape[1] or _whole_rows(t)

    def raw_last_ok(self):
        """may the last layer run as a plain product (no bias, no activation), finished by its consumer?"""
        l = self.layers[-1]
        return l.g is None and l.split * 2 == l.N and l.act0 == 'identity' and self.resid_cols == 0

    def raw_softplus_ok(self):
        """... by a row pass that adds the bias and applies the second head's softplus + shift (NLL rows, recon statistics)?"""
        return bool(self.raw_last_ok() and self.layers[-1].act1 == 'softplus')

    # the last layer's raw product and its gradient pair, as launched AND as asked about at plan time (``use_x3_last``)
    def _raw_last_call(self, x, publish=None):
        return (self.out[-1], x, self.layers[-1].W, True, True), dict(overread=True, publish=publish, kpad=self._pad_ok(x))

    def _bwd_pair_call(self, li, db, dpre, x, publish=None):
        l, prev = self.layers[li], self.layers[li - 1]
        return (l.dW, db, self.dpre[li - 1], dpre, x, l.W), dict(yref=self.out[li - 1], act=prev.act0, shift=prev.shift0,
                                                               overread=True, publish=publish, npad=self._pad_ok(x),
                                                               npad_x=True)

    def _x3_kw(self):
        """the launcher keywords of this chain's split-bf16 products: three parts are ``x3=True`` alone, as ever"""
        return dict(x3=True) if self.x3_parts == 3 else dict(x3=True, parts=self.x3_parts)

    def use_x3_last(self, dpre_last, db_in_pass, parts=3):
        """Route the last layer's raw product, its weight gradient and its data gradient to ``dv_gemm_x3`` (``parts`` = 2, 1:
        to ``dv_gemm_split`` with that many bf16 parts per operand, matmul 'bf16x2' / 'bf16x1') from now on.
        Decides up front: raises ValueError naming the reason when one of the three descriptors is not one the split-bf16
        kernels run (``dpre_last`` as ``backward`` will get it; ``db_in_pass``: the bias gradient comes from the producer
        of ``dpre_last``, not from the weight-gradient product)."""
        l, n = self.layers[-1], len(self.layers)
        why = None
        if parts not in (1, 2, 3):
            raise ValueError('use_x3_last(parts=%r): 1, 2 or 3' % (parts,))
        pk = {} if parts == 3 else dict(parts=parts)
        if not self.raw_last_ok():
            why = 'the layer cannot run as a plain product'
        elif n == 1:
            why = 'the layer is the chain\'s only one (its gradient products are not a plain pair)'
        else:
            # (the operand as a pass will really read it: a train pass of a chain with dropout sites reads the dropped
            # buffer, its evaluation passes the undropped one -- both are asked about)
            for x in ([self.outd[n - 2]] if self.masks else []) + [self.out[n - 2]]:
                a, kw = self._raw_last_call(x)
                why = K.x3_refusal(*a, **kw, **pk)
                if why is None:
                    a, kw = self._bwd_pair_call(n - 1, None if db_in_pass else l.db, dpre_last, x)
                    why = K.x3_pair_refusal(*a, **kw, **pk)
                if why is not None:
                    break
        if why is not None:
            raise ValueError("matmul='bf16x%d': the decoder-heads layer (%d x %d, %d rows) cannot run on %s: %s"
                             % (parts, l.N, l.Kin, self.M, 'dv_gemm_x3' if parts == 3 else 'dv_gemm_split', why))
        self.x3_last, self.x3_parts = True, parts

    def forward(self, inputs, resid=None, publish=None, heads=None, raw_last=False, x3=False, drop=False):
        """``publish`` = (flag, counter, add): the FIRST launch of the chain publishes on entry.
        ``raw_last``: the last layer's launch is the plain product x W^T -- bias, the second head's activation and its
        shift are left to the consumer (``K.nll_rows_fwdbwd(bias=...)``: chip-filling heads, plain GEMM epilogue);
        ``x3``: ... as a split-bf16 product (a chain that ``use_x3_last`` has accepted; ``backward(x3_last=True)`` goes with it).
        ``heads`` = dict(sample=...) | dict(nll=..., out=...): the dual-head last layer runs as ``K.linear_heads``
        with that row work fused into its epilogue (with ``nll`` the heads themselves are NOT stored: ``out``
        receives their gradients).
        ``drop``: a training pass of a chain with dropout sites (see the class docstring); else no site launches anything."""
        x = list(inputs)
        drop = bool(drop and self.masks)
        assert not x3 or (self.x3_last and raw_last and heads is None), 'x3: a raw last layer that use_x3_last accepted'
        for li, l in enumerate(self.layers):
            if l.g is not None:
                K.wn_scale(l.scale, l.norm, l.W, l.g)
            last = li == len(self.layers) - 1
            kpad = len(x) == 1 and self._pad_ok(x[0])      # (only inputs whose pad columns are zero BY CONSTRUCTION)
            if last and heads is not None:
                assert l.split * 2 == l.N
                K.linear_heads(heads.get('out', self.out[li]), x[0], l.W, l.b, split=l.split,
                               x2=x[1] if len(x) > 1 else None, scale=l.scale, act0=l.act0, act1=l.act1,
                               shift0=l.shift0, shift1=l.shift1, resid=resid,
                               resid_cols=self.resid_cols if resid is not None else 0, overread=True,
                               publish=publish if (li == 0 and l.g is None) else None,
                               sample=heads.get('sample'), nll=heads.get('nll'), kpad=kpad)
                return self.out[-1]
            if last and raw_last:
                assert self.raw_last_ok() and resid is None
                if x3:
                    a, kw = self._raw_last_call(x[0], publish if li == 0 else None)
                    K.gemm(*a, **self._x3_kw(), **kw)
                else:
                    K.gemm(self.out[li], x[0], l.W, True, True, A2=x[1] if len(x) > 1 else None, overread=True,
                           publish=publish if li == 0 else None, kpad=kpad)
                return self.out[-1]
            if last and l.tri:
                # three heads (zero-inflated decoder): the pair exactly as a two-head layer runs, into columns [0, 2 split),
                # and the identity head as one more plain Linear from the same input into columns [2 split, 3 split)
                assert resid is None
                n2, x2 = 2 * l.split, x[1] if len(x) > 1 else None
                sc = (None, None) if l.scale is None else (l.scale[:n2], l.scale[n2:])
                K.linear_fwd(self.out[li][:, :n2], x[0], l.W[:n2], l.b[:n2], x2=x2, scale=sc[0], split=l.split, act0=l.act0,
                             act1=l.act1, shift0=l.shift0, shift1=l.shift1, overread=True,
                             publish=publish if (li == 0 and l.g is None) else None, kpad=kpad)
                K.linear_fwd(self.out[li][:, n2:], x[0], l.W[n2:], l.b[n2:], x2=x2, scale=sc[1], overread=True, kpad=kpad)
                break
            K.linear_fwd(self.out[li], x[0], l.W, l.b, x2=x[1] if len(x) > 1 else None, scale=l.scale, split=l.split,
                         act0=l.act0, act1=l.act1, shift0=l.shift0, shift1=l.shift1,
                         resid=resid if last else None, resid_cols=self.resid_cols if (last and resid is not None) else 0,
                         overread=True, publish=publish if (li == 0 and l.g is None) else None, kpad=kpad)
            if last:
                break
            if drop:
                K.mask_scale(self.outd[li], self.out[li], self.masks[li], self.inv_keep)
            x = [self._hidden(li, drop)]
        return self.out[-1]

    def backward(self, dpre_last, inputs, dinputs=None, publish_after_last=None, publish_first=None, db_last_done=False,
                 klq=None, x3_last=False, drop=False):
        """dpre_last: gradient w.r.t. the last layer's pre-activation.  ``dinputs``: per input
        source a list of (dst, alpha, beta) destinations for its gradient (or None to skip).
        ``publish_after_last`` = (flag, counter, add):
        the first launch AFTER the last layer's launches publishes the flag on entry (= both gradients of the
        last layer are final and its weights are no longer read); ``publish_first``: the chain's FIRST launch
        does (= everything in front of this backward pass is complete).  ``db_last_done``: the
        last layer's bias gradient has been written by the producer of ``dpre_last`` already (``kernels.nll_rows_raw_cs``).
        ``x3_last``: the last layer's forward ran as a split-bf16 product (``forward(x3=True)``): so do its two gradient products.
        ``klq`` (see ``kernels.linear_bwd_pair``): the chain's input is a sample of q rows -- the FIRST layer's data-gradient
        launch writes d/d(mu | logvar) of those rows instead of d/d(input); returns True when the launch took it (a paired
        first layer), else the caller runs the row pass itself.
        ``drop``: the forward pass ran with ``drop=True``: same masks, see the class docstring."""
        assert not x3_last or self.x3_last
        drop = bool(drop and self.masks)
        dpre = dpre_last
        pending_pub = publish_first
        took_klq = False
        n_layers = len(self.layers)
        for li in range(n_layers - 1, -1, -1):
            l = self.layers[li]
            db = None if (db_last_done and li == n_layers - 1) else l.db
            srcs = list(inputs) if li == 0 else [self._hidden(li - 1, drop)]
            if li == len(self.layers) - 2 and publish_after_last is not None:
                pending_pub = publish_after_last

            # the layer's weight- and data-gradient both only need dpre: one paired launch when the
            # layer has a single input source, no WeightNorm and a single data-gradient destination
            single_dst = li > 0 or (dinputs is not None and len(srcs) == 1 and dinputs[0] is not None
                                    and len(dinputs[0]) == 1)
            if l.g is None and len(srcs) == 1 and single_dst:
                if li > 0:
                    prev = self.layers[li - 1]
                    a, kw = self._bwd_pair_call(li, db, dpre, srcs[0], pending_pub)
                    K.linear_bwd_pair(*a, **kw, **(self._x3_kw() if (x3_last and li == n_layers - 1) else {}))
                    dpre = self.dpre[li - 1]
                    # (in place: ``dv_mask_scale`` reads and writes element i from thread i alone, so x == y is sound although its
                    # kernel declares both ``__restrict__`` -- to be dropped there)
                    if drop:     # (dpre . W) * act'(out) * mask / keep: the factors are elementwise and commute
                        K.mask_scale(dpre, dpre, self.masks[li - 1], self.inv_keep)
                else:
                    dst, alpha, beta = dinputs[0][0]
                    if klq is not None and beta == 0.0:
                        K.linear_bwd_pair(l.dW, db, None, dpre, srcs[0], l.W, alpha=alpha, overread=True, publish=pending_pub,
                                          npad=self._pad_ok(srcs[0]), klq=klq)
                        took_klq = True
                    else:
                        K.linear_bwd_pair(l.dW, db, dst, dpre, srcs[0], l.W, alpha=alpha, beta_x=beta, overread=True,
                                          publish=pending_pub, npad=self._pad_ok(srcs[0]), npad_x=_whole_rows(dst))
                pending_pub = None
                continue
            if pending_pub is not None:      # (no paired launch for this layer: a launch of its own)
                K.flag_publish(*pending_pub)
                pending_pub = None
            dW = l.raw if l.g is not None else l.dW
            c0 = 0
            for si, s in enumerate(srcs):
                w = s.shape[1]
                K.linear_bwd_weight(dW[:, c0:c0 + w], dpre, s, dbias=db if si == 0 else None, overread=True,
                                    npad=len(srcs) == 1 and l.g is None and self._pad_ok(s))
                c0 += w
            if l.g is not None:
                K.wn_bwd(l.dW, l.dg, l.raw, l.W, l.g, l.norm)
            if li > 0:
                prev = self.layers[li - 1]
                K.linear_bwd_data(self.dpre[li - 1], dpre, l.W, kscale=l.scale, yref=self.out[li - 1], act=prev.act0,
                                  shift=prev.shift0, overread=True, npad=True)
                dpre = self.dpre[li - 1]
                if drop:
                    K.mask_scale(dpre, dpre, self.masks[li - 1], self.inv_keep)
            elif dinputs is not None:
                c0 = 0
                for si, s in enumerate(srcs):
                    w = s.shape[1]
                    for (dst, alpha, beta) in (dinputs[si] or []):
                        K.linear_bwd_data(dst, dpre, l.W[:, c0:c0 + w], kscale=l.scale, alpha=alpha, beta=beta,
                                          overread=True)
                    c0 += w
        return took_klq
