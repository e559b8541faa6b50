"""Every instantiation of curl3d_advect_kernel<PADDED, MB, METHOD> (csrc/wn_wavelet_advect.hip) compiles without a private
segment: the position, the stage point and RK4's running sum live in registers across the step loop, and a spill would put
scratch traffic into every stage of every step.  This compiles the file with the Makefile's own command line for the
device only, reads the kernel descriptors, and prints each instantiation's VGPRs and the waves per SIMD they allow beside
those of curl3d_points_kernel<PADDED, MB>, the velocity evaluation alone.  No occupancy is asserted."""
import re

import pytest

from _device_asm import descriptor, device_assembly, kernels, waves_per_simd

ADVECT = "_ZN12_GLOBAL__N_120curl3d_advect_kernelILb{}ELb{}ELi{}EEEvNS_10AdvectArgsE"
POINTS = "_ZN12_GLOBAL__N_120curl3d_points_kernelILb{}ELb{}EEEvNS_14CurlPointsArgsE"
METHODS = ("euler", "midpoint", "rk4")
KERNELS = [ADVECT.format(p, m, k) for p in (0, 1) for m in (0, 1) for k in range(3)]


@pytest.fixture(scope="module")
def texts(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("asm")
    return device_assembly("wn_wavelet_advect", tmp), device_assembly("wn_wavelet_curl", tmp)


def test_advect_kernels_have_no_private_segment(texts):
    advect, curl = texts
    assert kernels(advect) == set(KERNELS), sorted(kernels(advect) ^ set(KERNELS))
    print()
    for p in (0, 1):
        for m in (0, 1):
            base = descriptor(curl, POINTS.format(p, m))["next_free_vgpr"]
            print(f"curl3d_points_kernel<{p},{m}>: vgprs {base}, waves per SIMD {waves_per_simd(base)}")
            for k, name in enumerate(METHODS):
                sym = ADVECT.format(p, m, k)
                d = descriptor(advect, sym)
                body = re.search(rf"^{sym}:[^\n]*\n(.*?)^\.Lfunc_end\d+:", advect, re.S | re.M).group(1)
                count = len(re.findall(r"^\s+[a-z]\w+ ", body, re.M))
                print(f"  curl3d_advect_kernel<{p},{m},{name}>: vgprs {d['next_free_vgpr']}, waves per SIMD "
                      f"{waves_per_simd(d['next_free_vgpr'])}, static LDS {d['group_segment_fixed_size']}, "
                      f"instructions {count}")
                assert d["private_segment_fixed_size"] == 0, f"{sym} has a private segment"
                assert d["group_segment_fixed_size"] == 0, f"{sym} uses LDS"
