"""Sparse count matrices as the device batch feed reads them: CSR rows (``CsrRows``).

Sequencing counts are 90 to 95 % zeros and every tool that produces them keeps them in CSR (AnnData's ``.X``,
``scipy.sparse``).  A dataset may hold ``x1`` and / or ``x2`` as a ``CsrRows``: the graph-resident feed (``dv_batch_feed``, the
``csr1_*`` / ``csr2_*`` fields of its descriptor) then scatters the batch's rows into the dense step buffers itself -- the bits
the dense feed writes for the densified matrix -- and the dense ``(N, X)`` matrix never exists, on the host or in HBM.
"""
import numpy as np
import torch


class CsrRows:
    """``N`` rows of ``X`` columns as three arrays: ``ptr`` (N + 1 int64 row offsets; nnz may exceed 2^31), ``idx`` (nnz int32
    column indices, strictly increasing inside a row) and ``val`` (nnz fp32 values).  The arrays are read in place by the
    feed: values edited in place are seen by the next step."""

    def __init__(self, ptr, idx, val, shape):
        n, X = int(shape[0]), int(shape[1])
        ptr, idx, val = torch.as_tensor(ptr), torch.as_tensor(idx), torch.as_tensor(val)
        if not (ptr.dim() == 1 and idx.dim() == 1 and val.dim() == 1):
            raise ValueError('CsrRows: ptr, idx and val are one-dimensional arrays')
        if ptr.numel() != n + 1 or idx.numel() != val.numel() or n < 0 or X < 0 or X >= 2 ** 31:
            raise ValueError('CsrRows: ptr holds N + 1 = %d offsets and idx / val one entry each (got %d, %d, %d)'
                             % (n + 1, ptr.numel(), idx.numel(), val.numel()))
        if not (ptr.device == idx.device == val.device):
            raise ValueError('CsrRows: ptr, idx and val live on one device')
        self.ptr = ptr.to(torch.int64).contiguous()
        self.idx = idx.to(torch.int32).contiguous()
        self.val = val.to(torch.float32).contiguous()
        self._shape = (n, X)
        self._checked = False

    # ------------------------------------------------------------------------------------------- construction
    @classmethod
    def from_scipy(cls, m):
        """from anything ``scipy.sparse.csr_matrix`` accepts (AnnData's ``.X``); duplicates are summed and the rows sorted on a
        copy first"""
        import scipy.sparse as sp
        m = sp.csr_matrix(m, copy=True)
        m.sum_duplicates()
        m.sort_indices()
        return cls(torch.from_numpy(m.indptr.astype(np.int64)), torch.from_numpy(m.indices.astype(np.int32)),
                   torch.from_numpy(m.data.astype(np.float32)), m.shape)

    @classmethod
    def from_torch(cls, t):
        """from a ``torch.sparse_csr`` tensor (its arrays are taken as they are: ``check()`` tells whether the rows are sorted)"""
        if t.layout != torch.sparse_csr or t.dim() != 2:
            raise ValueError('CsrRows.from_torch: a two-dimensional torch.sparse_csr tensor')
        return cls(t.crow_indices(), t.col_indices(), t.values(), t.shape)

    @classmethod
    def from_dense(cls, x):
        """the non-zero entries of a dense matrix (tests and small data)"""
        x = torch.as_tensor(x)
        if x.dim() != 2:
            raise ValueError('CsrRows.from_dense: a two-dimensional matrix')
        nz = x != 0
        ptr = torch.zeros(x.shape[0] + 1, dtype=torch.int64, device=x.device)
        ptr[1:] = nz.sum(1).cumsum(0)
        r, c = torch.nonzero(nz, as_tuple=True)        # (row-major: sorted inside a row)
        return cls(ptr, c.to(torch.int32), x[r, c].to(torch.float32), x.shape)

    # ------------------------------------------------------------------------------------------- what a matrix has
    @property
    def shape(self):
        return self._shape

    def size(self, dim=None):
        return self._shape if dim is None else self._shape[dim]

    def dim(self):
        return 2

    def __len__(self):
        return self._shape[0]

    @property
    def device(self):
        return self.val.device

    @property
    def is_cuda(self):
        return self.val.is_cuda

    @property
    def nnz(self):
        return int(self.val.numel())

    def nbytes(self):
        return self.ptr.numel() * 8 + self.idx.numel() * 4 + self.val.numel() * 4

    def to(self, device):
        """the three arrays on ``device`` (the same object when they are there already)"""
        device = torch.device(device)
        if device.type == self.device.type and (device.index is None or device.index == self.device.index):
            return self
        out = CsrRows(self.ptr.to(device), self.idx.to(device), self.val.to(device), self._shape)
        out._checked = self._checked
        return out

    def row_sums(self):
        """the rows' totals, fp32 (accumulated in float64 in index order: one fixed order, no atomics)"""
        cs = torch.zeros(self.nnz + 1, dtype=torch.float64, device=self.device)
        cs[1:] = self.val.double().cumsum(0)
        return (cs[self.ptr[1:]] - cs[self.ptr[:-1]]).float()

    def to_dense(self, rows=None):
        """the dense fp32 matrix, or its rows ``rows`` (any integer index tensor, repeats allowed) -- plain torch, any device"""
        n, X = self._shape
        rows = torch.arange(n, device=self.device) if rows is None else torch.as_tensor(rows).to(self.device).long().reshape(-1)
        start = self.ptr[rows]
        cnt = self.ptr[rows + 1] - start
        out = torch.zeros(rows.numel(), X, dtype=torch.float32, device=self.device)
        total = int(cnt.sum())
        if total:
            ri = torch.repeat_interleave(torch.arange(rows.numel(), device=self.device), cnt)
            first = torch.repeat_interleave(cnt.cumsum(0) - cnt, cnt)
            e = torch.arange(total, device=self.device) - first + torch.repeat_interleave(start, cnt)
            out[ri, self.idx[e].long()] = self.val[e]
        return out

    def __getitem__(self, index):
        """dense rows, as indexing the dense matrix by rows gives them (host loaders: the slow path)"""
        if isinstance(index, (int, np.integer)) or (torch.is_tensor(index) and index.dim() == 0):
            i = int(index)
            return self.to_dense(torch.tensor([i + self._shape[0] if i < 0 else i]))[0]
        if isinstance(index, slice):
            index = torch.arange(self._shape[0])[index]
        index = torch.as_tensor(index)
        if index.dtype == torch.bool:
            index = torch.nonzero(index.reshape(-1)).reshape(-1)
        return self.to_dense(index)

    # ------------------------------------------------------------------------------------------- the structure
    def check(self):
        """the structure the feed relies on, checked ONCE per object where the arrays live, with reductions only; ``ValueError``
        naming the first violated rule.  (The kernel skips an entry whose column is out of range; it does not detect one.)"""
        if self._checked:
            return self
        n, X = self._shape
        ptr, idx, val, nnz = self.ptr, self.idx, self.val, self.nnz

        def fail(rule):
            raise ValueError('CsrRows.check: %s' % rule)
        if int(ptr[0]) != 0:
            fail('ptr[0] == 0 (it is %d)' % int(ptr[0]))
        if n and bool((ptr[1:] < ptr[:-1]).any()):
            fail('ptr is non-decreasing (it decreases at row %d)' % int(torch.nonzero(ptr[1:] < ptr[:-1])[0]))
        if int(ptr[n]) != nnz:
            fail('ptr[N] == nnz (ptr[N] is %d, nnz is %d)' % (int(ptr[n]), nnz))
        if nnz:
            if int(idx.min()) < 0:
                fail('0 <= idx (a negative column: %d)' % int(idx.min()))
            if int(idx.max()) >= X:
                fail('idx < X = %d (a column %d)' % (X, int(idx.max())))
            if nnz > 1:
                inner = torch.ones(nnz + 1, dtype=torch.bool, device=idx.device)
                inner[ptr] = False          # (entry k starts a row: nothing to compare it with)
                inner = inner[1:nnz]
                if bool(((idx[1:] < idx[:-1]) & inner).any()):
                    fail('indices increase inside every row (an unsorted row)')
                if bool(((idx[1:] == idx[:-1]) & inner).any()):
                    fail('indices strictly increase inside every row (a duplicate column)')
            if not bool(torch.isfinite(val).all()):
                fail('val is finite (a NaN or an infinity)')
        self._checked = True
        return self

    # ------------------------------------------------------------------------------------------- rows to a dense buffer
    def gather_rows(self, out, idx32):
        """``out[i] = row idx32[i]`` as dense fp32 rows.  On the device ONE ``dv_batch_feed`` launch -- a one-batch table, a
        zero counter, no noise, transform 0, no label outputs: the form the step's explicit-batch path uses; on a host tensor
        plain torch"""
        assert tuple(out.shape) == (idx32.numel(), self._shape[1])
        if not out.is_cuda:
            out.copy_(self.to_dense(idx32))
            return out
        from . import kernels as K
        if idx32.numel() == 0:
            return out
        zero = self.__dict__.get('_zero')
        if zero is None or zero.device != out.device:
            zero = self._zero = torch.zeros(1, dtype=torch.int32, device=out.device)
        K.batch_feed(out, self, None, None, idx32.reshape(1, -1), 1, zero, zero)
        return out
