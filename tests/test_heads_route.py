"""CPU checks of the paired-heads dispatch rule (drvae_amd/csrc/heads_route.h: plain host code, compiled here into a
program of its own) and of the 16-row heads kernel's code-object metadata in the built library."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = '/opt/rocm/lib/llvm/bin'
KS8, DENSE, T16 = 0, 1, 2

MAIN = r'''
#include <cstdio>
#include <cstdlib>
#include "heads_route.h"
int main(int argc, char** argv) {
    for (int i = 1; i + 5 < argc; i += 6)
        std::printf("%d\n", dv_heads_route(std::atoi(argv[i]), std::atoi(argv[i + 1]), std::atoi(argv[i + 2]), std::atoi(argv[i + 3]),
                                           std::atoi(argv[i + 4]), std::atoi(argv[i + 5])));
    return 0;
}
'''


@pytest.fixture(scope='module')
def route(tmp_path_factory):
    cxx = next((c for c in (os.path.join(LLVM, 'clang++'), shutil.which('c++'), shutil.which('g++')) if c and os.path.exists(c)), None)
    if cxx is None:
        pytest.skip('no host C++ compiler')
    d = tmp_path_factory.mktemp('route')
    (d / 'main.cpp').write_text(MAIN)
    exe = str(d / 'route')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-I', os.path.join(ROOT, 'drvae_amd', 'csrc'), str(d / 'main.cpp'), '-o', exe])

    def call(cases):
        """cases: (tiles32, K, sample, ring_ok, opt4, dense_min) -> route codes"""
        out = subprocess.run([exe] + [str(v) for c in cases for v in c], capture_output=True, text=True, check=True).stdout
        return [int(x) for x in out.split()]
    return call


def consts():
    src = open(os.path.join(ROOT, 'drvae_amd', 'csrc', 'heads_route.h')).read()
    return (int(re.search(r'#define DV_HEADS_T16_MIN_K (\d+)', src).group(1)),
            int(re.search(r'#define DV_HEADS_T16_MAX_TILES32 (\d+)', src).group(1)))


def tiles32(M, S):
    return -(-M // 32) * -(-S // 16)


def test_route_at_the_cfg2_sample_shapes(route):
    """encoder heads 224 x (100 + 100) x 800 move to the 16-row tile; the z2Fz1 heads (K = 100) and the side chain's
    450 x (100 + 100) x 200 stay (profiles/r17_enc_heads.md: the timings)"""
    got = route([(tiles32(224, 100), 800, 1, 1, 0, 512), (tiles32(300, 100), 100, 1, 1, 0, 512), (tiles32(450, 100), 200, 1, 1, 0, 512)])
    assert got == [T16, KS8, KS8]


def test_route_on_both_sides_of_its_thresholds(route):
    kmin, tmax = consts()
    t = tiles32(224, 100)
    assert t <= tmax
    got = route([(t, kmin, 1, 1, 0, 512), (t, kmin - 4, 1, 1, 0, 512), (tmax, kmin, 1, 1, 0, 512), (tmax + 1, kmin, 1, 1, 0, 512)])
    assert got == [T16, KS8, T16, KS8]


def test_route_touches_neither_the_nll_mode_nor_the_chip_filling_grids(route):
    kmin, tmax = consts()
    got = route([(49, 800, 0, 1, 0, 512),        # NLL: never the 16-row tile (dv_gemm_heads_tiles sizes its partials)
                 (49, 800, 0, 1, 4, 512),        # ... not even forced
                 (1178, 600, 0, 1, 0, 512),      # the decoder heads: the seven-per-CU route, as before
                 (1178, 600, 1, 1, 0, 512), (1178, 600, 1, 1, 5, 512),
                 (49, 800, 1, 1, 3, 512),        # opt[4] = 3 still forces that route
                 (49, 800, 1, 0, 0, 512),        # no ring (K % 4 != 0, unaligned rows, opt[3] = -1): the 32-row kernels
                 (49, 800, 1, 0, 4, 512)])
    assert got == [KS8, KS8, DENSE, DENSE, DENSE, DENSE, KS8, KS8]


def test_route_force_and_forbid(route):
    got = route([(70, 100, 1, 1, 4, 512), (1178, 600, 1, 1, 4, 512), (49, 800, 1, 1, 5, 512), (1, 4, 1, 1, 4, 512)])
    assert got == [T16, T16, KS8, T16]


def test_heads16_kernel_keeps_its_registers(tmp_path):
    """the new kernel in the built library's gfx950 code object: no spilled vector or scalar registers, no private segment,
    and its ring (four slots of 16 KiB) as static LDS"""
    from drvae_amd import _lib, build
    if not os.path.exists(os.path.join(LLVM, 'llvm-objdump')):
        pytest.skip('needs the ROCm llvm tools')
    build.build(verbose=False)
    so = shutil.copy(_lib.LIB_PATH, str(tmp_path))
    subprocess.run([os.path.join(LLVM, 'llvm-objdump'), '--offloading', so], cwd=str(tmp_path), capture_output=True, check=True)
    found = []
    for f in sorted(os.listdir(str(tmp_path))):
        if 'gfx950' not in f:
            continue
        notes = subprocess.run([os.path.join(LLVM, 'llvm-readelf'), '--notes', os.path.join(str(tmp_path), f)],
                               capture_output=True, text=True, check=True).stdout
        # one metadata map per kernel: split at the list items of amdhsa.kernels
        for blk in re.split(r'\n\s+- \.agpr_count:', notes):
            name = re.search(r'\.name:\s+(\S+)', blk)
            if name is None or 'gemm_heads16_kernel' not in name.group(1):
                continue
            val = lambda k: int(re.search(r'\.%s:\s+(\d+)' % k, blk).group(1))      # noqa: E731
            found.append((name.group(1), val('vgpr_count'), val('vgpr_spill_count'), val('sgpr_spill_count'),
                          val('private_segment_fixed_size'), val('group_segment_fixed_size')))
    assert len(found) == 1, found
    name, vgpr, vspill, sspill, private, lds = found[0]
    print(found[0])
    assert vspill == 0 and sspill == 0 and private == 0
    assert vgpr <= 128 and lds == 65536
