"""Every instantiation of perlin_curl_advect_kernel<KIND, METHOD> (csrc/wn_perlin_advect.hip) compiles without a private
segment and with the 512-byte permutation table as its only LDS: the position, the stage point, the stage velocity and
RK4's running sum live in registers across the step loop, and a spill would put scratch traffic into every stage of every
step.  This compiles the file with the Makefile's own command line for the device only, reads the kernel descriptors, and
prints each instantiation's VGPRs and the waves per SIMD they allow beside those of perlin_curl_points_kernel, the velocity
evaluation alone.  No occupancy is asserted."""
import re

import pytest

from _device_asm import descriptor, device_assembly, kernels, waves_per_simd

ADVECT = "_ZN12_GLOBAL__N_125perlin_curl_advect_kernelILi{}ELi{}EEEvNS_16PerlinAdvectArgsE"
POINTS = "_ZN12_GLOBAL__N_125perlin_curl_points_kernelENS_20PerlinCurlPointsArgsE"
KINDS = ("noise", "turb", "fractal")
METHODS = ("euler", "midpoint", "rk4")
KERNELS = [ADVECT.format(k, m) for k in range(3) for m in range(3)]


@pytest.fixture(scope="module")
def texts(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("asm")
    return device_assembly("wn_perlin_advect", tmp), device_assembly("wn_perlin_curl", tmp)


def test_perlin_advect_kernels_have_no_private_segment_and_only_the_table_in_lds(texts):
    advect, curl = texts
    assert kernels(advect) == set(KERNELS), sorted(kernels(advect) ^ set(KERNELS))
    base = descriptor(curl, POINTS)["next_free_vgpr"]
    print(f"\nperlin_curl_points_kernel: vgprs {base}, waves per SIMD {waves_per_simd(base)}")
    for k, kind in enumerate(KINDS):
        for m, method in enumerate(METHODS):
            sym = ADVECT.format(k, m)
            d = descriptor(advect, sym)
            body = re.search(rf"^{sym}:[^\n]*\n(.*?)^\.Lfunc_end\d+:", advect, re.S | re.M).group(1)
            count = len(re.findall(r"^\s+[a-z]\w+ ", body, re.M))
            print(f"  perlin_curl_advect_kernel<{kind},{method}>: vgprs {d['next_free_vgpr']}, waves per SIMD "
                  f"{waves_per_simd(d['next_free_vgpr'])}, static LDS {d['group_segment_fixed_size']}, instructions {count}")
            assert d["private_segment_fixed_size"] == 0, f"{sym} has a private segment"
            assert "scratch_" not in body, f"{sym} spills to scratch"
            assert d["group_segment_fixed_size"] == 512, f"{sym}: LDS beyond the permutation table"
