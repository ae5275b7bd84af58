"""CPU checks of the ring-depth rule of the latency-bound GEMM launches (drvae_amd/csrc/ring_route.h: plain host code,
compiled here into a program of its own) and of the deeper rings' kernels in the built library's code-object metadata."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = '/opt/rocm/lib/llvm/bin'
GEMM, HEADS, PAIR = 0, 1, 2
FOUR_WAVE, DEPTH4, DEPTH3, FORBID = 1, 2, 3, 4
SLOT_BYTES = 16384                  # one K tile of 64: (32 + 32) lines x 64 floats
LDS_PER_CU = 160 * 1024

MAIN = r'''
#include <cstdio>
#include <cstdlib>
#include "ring_route.h"
int main(int argc, char** argv) {
    for (int i = 1; i + 5 < argc; i += 6)
        std::printf("%d\n", dv_ring_depth(std::atoi(argv[i]), std::atoi(argv[i + 1]), std::atoi(argv[i + 2]), std::atoi(argv[i + 3]),
                                          std::atoi(argv[i + 4]), std::atoi(argv[i + 5])));
    return 0;
}
'''


@pytest.fixture(scope='module')
def depth(tmp_path_factory):
    cxx = next((c for c in (os.path.join(LLVM, 'clang++'), shutil.which('c++'), shutil.which('g++')) if c and os.path.exists(c)), None)
    if cxx is None:
        pytest.skip('no host C++ compiler')
    d = tmp_path_factory.mktemp('ring')
    (d / 'main.cpp').write_text(MAIN)
    exe = str(d / 'ring')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-I', os.path.join(ROOT, 'drvae_amd', 'csrc'), str(d / 'main.cpp'), '-o', exe])

    def call(cases):
        """cases: (family, tiles32, K, a_kcontig, b_kcontig, opt7) -> ring depths"""
        out = []
        for i in range(0, len(cases), 500):          # (argv stays short)
            txt = subprocess.run([exe] + [str(v) for c in cases[i:i + 500] for v in c], capture_output=True, text=True, check=True).stdout
            out += [int(x) for x in txt.split()]
        assert len(out) == len(cases)
        return out
    return call


def const(name):
    src = open(os.path.join(ROOT, 'drvae_amd', 'csrc', 'ring_route.h')).read()
    return int(re.search(r'#define %s (\d+)' % name, src).group(1))


LAYOUTS = [(1, 1), (1, 0), (0, 0)]
# the cfg-2 step's launches of the three families: (family, workgroups, K, a_kcontig, b_kcontig)
CFG2 = [(GEMM, 175, 980, 1, 1), (PAIR, 152, 600, 0, 0), (PAIR, 60, 300, 0, 0), (PAIR, 357, 224, 0, 0), (PAIR, 88, 450, 0, 0),
        (PAIR, 154, 450, 0, 0), (HEADS, 105, 200, 1, 1), (GEMM, 361, 100, 1, 1), (GEMM, 105, 104, 1, 1)]


def test_force_and_forbid(depth):
    cases = [(f, t, k, a, b) for f in (GEMM, HEADS, PAIR) for t in (1, 49, 128, 129, 192, 193, 511) for k in (4, 64, 256, 980)
             for (a, b) in LAYOUTS]
    assert set(depth([c + (DEPTH4,) for c in cases])) == {4}
    assert set(depth([c + (DEPTH3,) for c in cases])) == {3}
    assert set(depth([c + (FORBID,) for c in cases])) == {2}
    assert set(depth([c + (FOUR_WAVE,) for c in cases])) == {2}       # opt[7] = 1 keeps its meaning: as before
    assert set(depth([c + (7,) for c in cases])) == {2}               # a value the rule does not know: the ring of two


def test_rule_returns_a_depth_the_kernels_have_and_is_monotone_in_k(depth):
    for f in (GEMM, HEADS, PAIR):
        for t in (1, 64, 128, 129, 192, 193, 400):
            ks = list(range(4, 2049, 4))
            got = depth([(f, t, k, 1, 1, 0) for k in ks])
            assert set(got) <= {2, 3, 4}
            assert got == sorted(got), 'a longer K never gets a shallower ring'


def test_rule_keeps_every_grid_resident_in_one_round_on_64_cus(depth):
    """a ring of d slots is d x 16 KiB of LDS per workgroup; wherever 64 KiB per workgroup would not fit the grid in one round
    at two workgroups per CU on 64 CUs the rule returns at most three slots, and three only where three workgroups of 48 KiB
    per CU hold the grid"""
    assert LDS_PER_CU // (4 * SLOT_BYTES) == 2 and LDS_PER_CU // (3 * SLOT_BYTES) == 3
    assert const('DV_RING_D3_MAX_TILES32') <= 3 * 64
    cases = [(f, t, k, a, b, 0) for f in (GEMM, HEADS, PAIR) for t in range(1, 600, 7) for k in (64, 256, 600, 980, 4096)
             for (a, b) in LAYOUTS]
    cases += [(f, t, 4096, 1, 1, 0) for f in (GEMM, HEADS, PAIR) for t in (127, 128, 129, 191, 192, 193)]
    for c, d in zip(cases, depth(cases)):
        if c[1] > 2 * 64:
            assert d <= 3, c
        if c[1] > 3 * 64:
            assert d == 2, c


def test_rule_at_the_cfg2_launches(depth):
    """the table of the rule: what the cold-operand timings decided (profiles/r21_ring_depth.md) -- encoder layer 1, the
    decoder layer-1 pair, the side chain's two fprop pairs and its heads launches run three slots; the z2Fz1-heads pair (the
    ranges touched), the encoder-heads pair (slower, and 357 workgroups) and the short-K controls stay on two"""
    assert depth([c + (0,) for c in CFG2]) == [3, 3, 2, 2, 3, 3, 3, 2, 2]


def test_rule_on_both_sides_of_its_thresholds(depth):
    tmax = const('DV_RING_D3_MAX_TILES32')
    for fam, name in ((GEMM, 'GEMM'), (HEADS, 'HEADS'), (PAIR, 'PAIR')):
        kt = const('DV_RING_MIN_KTILES_' + name)
        got = depth([(fam, 100, 64 * (kt - 1) + 4, 1, 1, 0), (fam, 100, 64 * (kt - 1), 1, 1, 0), (fam, tmax, 64 * kt, 1, 1, 0),
                     (fam, tmax + 1, 64 * kt, 1, 1, 0), (fam, 1, 64 * 64, 1, 1, 0)])
        assert got == [3, 2, 3, 2, 3], (name, got)


NEW_KERNELS = [r'gemm_kpipe_kernelILi32ELi32ELi64ELi8ELb[01]ELb[01]ELi%dELi\d+E', r'gemm_kpipe_kernelILi32ELi32ELi64ELi4ELb[01]ELb[01]ELi%dELi\d+E',
               r'gemm_heads_pipe_kernelILi32ELi32ELi64ELi8ELi%dELi\d+E', r'gemm_pair_pipe_kernelILi32ELi32ELi64ELi4ELb0ELb0ELb1ELb0ELi%dELi\d+E']


def test_deep_ring_kernels_keep_their_registers(tmp_path):
    """every instantiation with three or four ring slots in the built library's gfx950 code object: no spilled vector or
    scalar registers, no private segment, static LDS = the ring (the K-split reduction reuses it) and at most 64 KiB"""
    from drvae_amd import _lib, build
    if not os.path.exists(os.path.join(LLVM, 'llvm-objdump')):
        pytest.skip('needs the ROCm llvm tools')
    build.build(verbose=False)
    so = shutil.copy(_lib.LIB_PATH, str(tmp_path))
    subprocess.run([os.path.join(LLVM, 'llvm-objdump'), '--offloading', so], cwd=str(tmp_path), capture_output=True, check=True)
    found = {}
    for f in sorted(os.listdir(str(tmp_path))):
        if 'gfx950' not in f:
            continue
        notes = subprocess.run([os.path.join(LLVM, 'llvm-readelf'), '--notes', os.path.join(str(tmp_path), f)],
                               capture_output=True, text=True, check=True).stdout
        for blk in re.split(r'\n\s+- \.agpr_count:', notes):
            name = re.search(r'\.name:\s+(\S+)', blk)
            if name is None:
                continue
            for pat in NEW_KERNELS:
                for s in (3, 4):
                    if re.search(pat % s, name.group(1)):
                        val = lambda k: int(re.search(r'\.%s:\s+(\d+)' % k, blk).group(1))      # noqa: E731
                        found[name.group(1)] = (s, val('vgpr_count'), val('vgpr_spill_count'), val('sgpr_spill_count'),
                                                val('private_segment_fixed_size'), val('group_segment_fixed_size'))
    # three layouts of the eight- and of the four-wave product, the heads and the pair kernel: at each of the two depths
    assert len(found) == 2 * (3 + 3 + 1 + 1), sorted(found)
    for name, (s, vgpr, vspill, sspill, private, lds) in sorted(found.items()):
        print(name, s, vgpr, vspill, sspill, private, lds)
        assert vspill == 0 and sspill == 0 and private == 0, name
        assert lds == s * SLOT_BYTES and lds <= 65536, name
        assert vgpr <= 128, name
