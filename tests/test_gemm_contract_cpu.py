"""CPU: the checks of the fp32 GEMM family's contract tests (tests/test_gpu_gemm_contract.py) have teeth, and the references
pass them -- no device, no library.  On the exact operands the GPU tests use: the sequential fp32 fma chain and torch's fp32
matmul pass the identities and the element-wise bound (the chain is its own yardstick: ratio 1), and every faulty emulation
of tests/gemm_contract.py fails the check that is meant to catch it."""
import pytest
import torch

from tests import gemm_contract as G

CASE_IDS = [G.case_id(c) for c in G.CASES]
REFERENCES = {'chain': G.chain_matmul, 'torch': lambda A, B: A @ B}


def identity_holds(mm, M, N, Kd):
    (A, P), (P2, B), C0 = G.identity_operands(M, N, Kd)
    ok = torch.equal(mm(A, P), G.exact_product(A, P)) and torch.equal(mm(P2, B), G.exact_product(P2, B))
    acc = mm(A, P)                     # alpha = -0.5, beta = 1 on small integers: the epilogue's one rounding
    return ok and torch.equal(acc * -0.5 + C0, G.exact_product(A, P, -0.5, 1.0, C0))


# ------------------------------------------------------------------------------------------------ the references pass
@pytest.mark.parametrize('case', G.CASES, ids=CASE_IDS)
@pytest.mark.parametrize('ref', sorted(REFERENCES))
def test_references_pass_the_identities(ref, case):
    _, M, N, Kd, _ = case
    assert identity_holds(REFERENCES[ref], M, N, Kd)


@pytest.mark.parametrize('case', G.CASES, ids=CASE_IDS)
def test_references_pass_the_bounds(case):
    _, M, N, Kd, _ = case
    A, B = G.random_operands(M, N, Kd)
    chain, mm = G.chain_matmul(A, B), A @ B
    for name in G.EPILOGUES:
        e = G.epilogue_case(name, M, N)
        want, bound, yard = G.expected(A, B, e, acc=chain)
        assert G.worst_excess(yard, want, bound) <= 1.0, name                # the chain through a plain fp32 epilogue
        assert G.norm_ratio(yard, yard, want) == 1.0
        _, _, got = G.expected(A, B, e, acc=mm)
        assert G.worst_excess(got, want, bound) <= 1.0, name                 # torch's blocked fp32 matmul
        assert G.norm_ratio(got, yard, want) <= 2.0, name


def test_reference_tile_maps_cover_every_grid():
    for tiling, grids in G.MAP_GRIDS.items():
        for grid in grids:
            M, N = G.map_shape(tiling, grid)
            A, B = G.integer_operands(M, N, 8)
            for tmap in G.MAPS:
                assert torch.equal(G.product_through_map(A, B, tiling, tmap), A @ B), (tiling, grid, tmap)


# ------------------------------------------------------------------------------------------------ the faults fail
def test_truncated_operands_fail_the_identities_and_the_norm_ratio():
    """operands cut to a 10-bit significand (what a reduced-precision matrix instruction would do)"""
    _, M, N, Kd, _ = G.BASE
    mm = lambda A, B: G.chain_matmul(G.truncated(A), G.truncated(B))
    assert not identity_holds(mm, M, N, Kd)
    A, B = G.random_operands(M, N, Kd)
    e = G.epilogue_case('plain', M, N)
    want, bound, yard = G.expected(A, B, e, acc=G.chain_matmul(A, B))
    assert G.norm_ratio(mm(A, B), yard, want) > 2.0


def test_a_dropped_last_k_fails_the_elementwise_bound():
    _, M, N, Kd, _ = G.BASE
    A, B = G.random_operands(M, N, Kd)
    want, bound, _ = G.expected(A, B, G.epilogue_case('plain', M, N))
    assert G.worst_excess(G.chain_matmul(A[:, :-1], B[:-1]), want, bound) > 1.0


@pytest.mark.parametrize('doubled', [0, 3, 7])
def test_a_doubled_ksplit_partial_fails_the_identities_and_the_elementwise_bound(doubled):
    _, M, N, Kd, _ = G.BASE
    assert identity_holds(lambda A, B: G.ksplit_matmul(A, B), M, N, Kd)                  # the honest K split passes
    assert not identity_holds(lambda A, B: G.ksplit_matmul(A, B, doubled=doubled), M, N, Kd)
    A, B = G.random_operands(M, N, Kd)
    want, bound, _ = G.expected(A, B, G.epilogue_case('plain', M, N))
    assert G.worst_excess(G.ksplit_matmul(A, B), want, bound) <= 1.0
    assert G.worst_excess(G.ksplit_matmul(A, B, doubled=doubled), want, bound) > 1.0


def test_lines_past_the_edge_taken_from_the_pad_fail_the_finite_check():
    """rows past the last row of an operand, read from what lies behind it (NaN guard rows) instead of being clamped or
    replaced by zeros.  Along M or N such rows only feed outputs that are never stored, whatever they hold; where they
    are k lines (the dy^T x layout) they feed every output, and the other operand's zeros do not cancel a NaN."""
    _, M, N, Kd, _ = G.BASE
    A, B = G.random_operands(M, N, Kd)
    p = G.Poisoned(A.t().contiguous(), torch.device('cpu'))           # Aop[m, k] = A[k * lda + m]
    want, bound, _ = G.expected(A, B, G.epilogue_case('plain', M, N))
    good = G.staged_matmul(p.buf, (G.GUARD, Kd, M), B)
    assert bool(torch.isfinite(good).all()) and G.worst_excess(good, want, bound) <= 1.0
    bad = G.staged_matmul(p.buf, (G.GUARD, Kd, M), B, lines='pad')
    assert not bool(torch.isfinite(bad).all())
    assert G.worst_excess(bad, want, bound) > 1.0                      # (a non-finite output counts as outside the bound)


def test_a_mask_by_multiplication_fails_the_propagation_check():
    """value * 0 keeps a NaN or an inf alive: with dense rows the chunk that straddles K holds the start of the next row, and
    that row's non-finite first element poisons the row in front of it -- an output outside the expected set"""
    for cls, Kd in (('D', 202), ('A', 200)):
        M, N = 150, 300
        A, B, want = G.poisoned_operands(M, N, Kd)
        p = G.Poisoned(A, torch.device('cpu'), cls)
        flat = p.buf.reshape(-1)[G.GUARD * p.buf.shape[1]:]
        good = G.overread_matmul(flat, M, Kd, p.buf.shape[1], B)
        assert torch.equal(~torch.isfinite(good), want)
        bad = G.overread_matmul(flat, M, Kd, p.buf.shape[1], B, mask='multiply')
        if Kd % 4:                                                      # (K % 4 == 0: no chunk straddles K, nothing to mask)
            assert not torch.equal(~torch.isfinite(bad), want)
    # ... and as the switch for k lines past K it turns the zero block's job into NaN * 0
    _, M, N, Kd, _ = G.BASE
    A, B = G.random_operands(M, N, Kd)
    p = G.Poisoned(A.t().contiguous(), torch.device('cpu'))
    assert not bool(torch.isfinite(G.staged_matmul(p.buf, (G.GUARD, Kd, M), B, lines='pad', mask='multiply')).any())
    assert bool(torch.isfinite(G.staged_matmul(p.buf, (G.GUARD, Kd, M), B, lines='pad', mask='select')).all())


def test_a_tile_map_that_skips_a_tile_fails_the_cover_check():
    for tiling, grids in G.MAP_GRIDS.items():
        for grid in grids:
            M, N = G.map_shape(tiling, grid)
            A, B = G.integer_operands(M, N, 8)
            for tmap in G.MAPS:
                got = G.product_through_map(A, B, tiling, tmap, tile_of=G.tile_of_block_skipping)
                assert not torch.equal(got, A @ B), (tiling, grid, tmap)


def test_poisoned_views_see_what_is_written_around_them():
    p = G.Poisoned(torch.zeros(5, 6), torch.device('cpu'), 'C', fill=G.SENTINEL)
    assert p.view.stride(0) % 2 == 1 and p.unchanged() and p.outside_untouched()
    p.view[2, 3] = 1.0
    assert not p.unchanged() and p.outside_untouched()
    p.buf[G.GUARD + 2, 6] = 1.0                       # the first pad column
    assert not p.outside_untouched()
    q = G.Poisoned(torch.zeros(7), torch.device('cpu'))
    q.buf[G.GUARD - 1] = 0.0                          # a NaN guard overwritten: the bits differ although NaN != NaN anyway
    assert not q.outside_untouched()
