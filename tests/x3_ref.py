"""Emulation of the split-bf16 product contract of ``dv_gemm_x3`` (drvae_amd/csrc/gemm_x3.hip), independent of the kernel:

* every fp32 element a is split as hi = bf16_rn(a), mid = bf16_rn(a - hi), lo = bf16_rn(a - hi - mid) with
  ``torch.bfloat16`` round-to-nearest-even (the two differences are exact in fp32);
* a product a * b is the sum of the six terms hi hi, hi mid, mid hi, hi lo, lo hi, mid mid -- each an exact fp32 number
  (8-bit x 8-bit significands), so evaluating them in float64 changes nothing;
* the sums over the terms and over k are accumulated in float64 here: what the contract computes, without the rounding of
  the kernel's fp32 accumulation (which the tests bound separately).
"""
import torch

# (a part, b part): 0 = hi, 1 = mid, 2 = lo -- the cross products of weight <= 2
TERMS = ((0, 0), (0, 1), (1, 0), (0, 2), (2, 0), (1, 1))


def split(a):
    """(hi, mid, lo) of an fp32 tensor, each an fp32 tensor holding bf16-representable values"""
    a = a.detach().to('cpu', torch.float32)
    hi = a.to(torch.bfloat16).to(torch.float32)
    r = a - hi
    mid = r.to(torch.bfloat16).to(torch.float32)
    lo = (r - mid).to(torch.bfloat16).to(torch.float32)
    return hi, mid, lo


def matmul(Aop, Bop, terms=TERMS):
    """Aop (M, K) @ Bop (K, N) by the contract, float64 result; ``terms``: which of the six terms take part"""
    sa = [t.double() for t in split(Aop)]
    sb = [t.double() for t in split(Bop)]
    out = torch.zeros(Aop.shape[0], Bop.shape[1], dtype=torch.float64)
    for i, j in terms:
        out += sa[i] @ sb[j]
    return out
