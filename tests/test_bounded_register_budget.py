"""Every instantiation of curl3d_bounded_points_kernel<PADDED, MB> and curl3d_bounded_advect_kernel<PADDED, MB, METHOD>
(csrc/wn_wavelet_bounded.hip) compiles without a private segment and without LDS: the obstacle list is read from the launch
arguments with scalar loads, and the position, the stage point, RK4's running sum, the ramp's A and G and the potential
values live in registers.  This compiles the file with the Makefile's own command line for the device only, reads the kernel
descriptors, and prints each instantiation's VGPRs and the waves per SIMD they allow beside those of the unbounded
curl3d_points_kernel and curl3d_advect_kernel.  No occupancy is asserted."""
import pytest

from _device_asm import descriptor, device_assembly, kernels, waves_per_simd

POINTS = "_ZN12_GLOBAL__N_128curl3d_bounded_points_kernelILb{}ELb{}EEEvNS_17BoundedPointsArgsE"
ADVECT = "_ZN12_GLOBAL__N_128curl3d_bounded_advect_kernelILb{}ELb{}ELi{}EEEvNS_17BoundedAdvectArgsE"
FREE_POINTS = "_ZN12_GLOBAL__N_120curl3d_points_kernelILb{}ELb{}EEEvNS_14CurlPointsArgsE"
FREE_ADVECT = "_ZN12_GLOBAL__N_120curl3d_advect_kernelILb{}ELb{}ELi{}EEEvNS_10AdvectArgsE"
METHODS = ("euler", "midpoint", "rk4")
KERNELS = [POINTS.format(p, m) for p in (0, 1) for m in (0, 1)] + \
          [ADVECT.format(p, m, k) for p in (0, 1) for m in (0, 1) for k in range(3)]


@pytest.fixture(scope="module")
def texts(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("asm")
    return [device_assembly(stem, tmp) for stem in ("wn_wavelet_bounded", "wn_wavelet_curl", "wn_wavelet_advect")]


def test_bounded_kernels_have_no_private_segment_and_no_lds(texts):
    bounded, curl, advect = texts
    assert len(KERNELS) == 4 + 12
    assert kernels(bounded) == set(KERNELS), sorted(kernels(bounded) ^ set(KERNELS))

    def row(name, text, sym, free_text, free_sym):
        d, base = descriptor(text, sym), descriptor(free_text, free_sym)["next_free_vgpr"]
        print(f"{name}: vgprs {d['next_free_vgpr']}, waves per SIMD {waves_per_simd(d['next_free_vgpr'])}, sgprs "
              f"{d['next_free_sgpr']}, static LDS {d['group_segment_fixed_size']}; unbounded: vgprs {base}, waves per SIMD "
              f"{waves_per_simd(base)}")
        assert d["private_segment_fixed_size"] == 0, f"{sym} has a private segment"
        assert d["group_segment_fixed_size"] == 0, f"{sym} uses LDS"

    print()
    for p in (0, 1):
        for m in (0, 1):
            row(f"curl3d_bounded_points_kernel<{p},{m}>", bounded, POINTS.format(p, m), curl, FREE_POINTS.format(p, m))
            for k, name in enumerate(METHODS):
                row(f"  curl3d_bounded_advect_kernel<{p},{m},{name}>", bounded, ADVECT.format(p, m, k), advect,
                    FREE_ADVECT.format(p, m, k))
