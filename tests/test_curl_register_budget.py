"""Every kernel of csrc/wn_wavelet_curl.hip (the curl point kernel, the exact grid kernel and the separable brick kernel for
1..8 bands) compiles without a private segment: a spill would put vector-memory traffic on the brick kernel's store stream.
The brick kernel keeps 4 waves per SIMD by registers and its static LDS (the boxes' geometry: 24 bytes per band).  This
compiles the file with the Makefile's own command line for the device only and reads the kernel descriptors."""
import pytest

from _device_asm import descriptor, device_assembly, kernels, waves_per_simd

SEP = "_ZN12_GLOBAL__N_122curl3d_grid_sep_kernelILi{}EEEvNS_11CurlSepArgsE"
KERNELS = ([SEP.format(nb) for nb in range(1, 9)]
           + [f"_ZN12_GLOBAL__N_125curl3d_grid_direct_kernelILb{p}EEEvNS_14CurlDirectArgsE" for p in (0, 1)]
           + [f"_ZN12_GLOBAL__N_120curl3d_points_kernelILb{p}ELb{m}EEEvNS_14CurlPointsArgsE" for p in (0, 1) for m in (0, 1)])


@pytest.fixture(scope="module")
def text(tmp_path_factory):
    return device_assembly("wn_wavelet_curl", tmp_path_factory.mktemp("asm"))


def test_curl_kernels_have_no_private_segment(text):
    assert kernels(text) == set(KERNELS), sorted(kernels(text) ^ set(KERNELS))
    for sym in KERNELS:
        assert descriptor(text, sym)["private_segment_fixed_size"] == 0, f"{sym} has a private segment"


def test_brick_kernel_keeps_its_occupancy(text):
    for nb in range(1, 9):
        d = descriptor(text, SEP.format(nb))
        print(f"curl3d_grid_sep_kernel<{nb}>: vgprs", d["next_free_vgpr"], "static LDS", d["group_segment_fixed_size"])
        assert waves_per_simd(d["next_free_vgpr"]) >= 4, (nb, d["next_free_vgpr"])
        assert d["group_segment_fixed_size"] == 24 * nb, (nb, d["group_segment_fixed_size"])
