"""The kernels of csrc/wn_wavelet_bricks.hip (include/wnoise_bricks.h): bricks_exact_kernel<PADDED, MB> and
bricks_sep_kernel<NB>, NB = 1..8, and nothing else.  This compiles the file with the Makefile's own command line for the
device only and reads the kernel descriptors: no kernel has a private segment and no body spills; the exact kernel uses no
LDS, and the separable kernel's static LDS is its coefficient boxes alone -- two bricks of NB boxes of kBoxCap floats -- with
no dynamic LDS at the launch.  Each instantiation's VGPRs and the waves per SIMD they allow are printed; no occupancy is
asserted."""
import os
import re

import pytest

from _device_asm import PKG, assert_no_scratch, descriptor, device_assembly, kernels, waves_per_simd

EXACT = "_ZN12_GLOBAL__N_119bricks_exact_kernelILb{}ELb{}EEEvNS_15BricksExactArgsE"
SEP = "_ZN12_GLOBAL__N_117bricks_sep_kernelILi{}EEEvN2wn12BrickSepArgsE"   # the brick lists' one argument struct
KERNELS = [EXACT.format(p, m) for p in (0, 1) for m in (0, 1)] + [SEP.format(nb) for nb in range(1, 9)]


@pytest.fixture(scope="module")
def text(tmp_path_factory):
    return device_assembly("wn_wavelet_bricks", tmp_path_factory.mktemp("asm"))


def box_cap():
    src = open(os.path.join(PKG, "csrc", "wn_wavelet_bricks.hip")).read()
    (expr,) = re.findall(r"constexpr int kBoxCap = ([\d\s\*]+);", src)
    cap = 1
    for f in expr.split("*"):
        cap *= int(f)
    # the separable launch passes no dynamic LDS: `dim3(256),\n 0, stream, a`
    launch = src[src.index("hipLaunchKernelGGL(bricks_sep_kernel"):]
    assert re.match(r"[^;]*dim3\(256\),\s*0, stream, a\);", launch), launch[:200]
    return cap


def test_the_kernel_set_is_the_expected_instantiations(text):
    assert len(KERNELS) == 12
    assert kernels(text) == set(KERNELS), sorted(kernels(text) ^ set(KERNELS))


def test_no_private_segment_and_the_lds_is_the_boxes(text):
    cap = box_cap()
    assert cap == 7 * 6 * 6          # 6 cells per axis under 8 samples at a step below 1/3, and the window's fourth column
    print()
    for p in (0, 1):
        for m in (0, 1):
            sym = EXACT.format(p, m)
            d = descriptor(text, sym)
            print(f"bricks_exact_kernel<{p},{m}>: vgprs {d['next_free_vgpr']}, waves per SIMD "
                  f"{waves_per_simd(d['next_free_vgpr'])}, sgprs {d['next_free_sgpr']}, static LDS {d['group_segment_fixed_size']}")
            assert_no_scratch(text, sym)
            assert d["group_segment_fixed_size"] == 0, f"{sym} uses LDS"
    for nb in range(1, 9):
        sym = SEP.format(nb)
        d = descriptor(text, sym)
        print(f"bricks_sep_kernel<{nb}>: vgprs {d['next_free_vgpr']}, waves per SIMD {waves_per_simd(d['next_free_vgpr'])}, "
              f"sgprs {d['next_free_sgpr']}, static LDS {d['group_segment_fixed_size']} B")
        assert_no_scratch(text, sym)
        assert d["group_segment_fixed_size"] == 2 * nb * cap * 4, (sym, d["group_segment_fixed_size"])
