"""Every kernel of csrc/wn_wavelet_grad_surface.hip (the 2-D point and grid kernels, the projected point and grid kernels
and the multiband projected point kernel) compiles without scratch: the projected cell loop is VALU-bound, and a spill
would add vector-memory traffic to every cell.  This compiles the file with the Makefile's own command line for the
device only and reads the kernel descriptors."""
from _device_asm import assert_no_scratch, device_assembly, kernels

KERNELS = ["_ZN12_GLOBAL__N_120grad2d_points_kernelENS_14SurfPointsArgsE",
           "_ZN12_GLOBAL__N_128grad_projected_points_kernelENS_14SurfPointsArgsE",
           "_ZN12_GLOBAL__N_138grad_multiband_projected_points_kernelENS_14SurfPointsArgsE",
           "_ZN12_GLOBAL__N_118grad2d_grid_kernelENS_12SurfGridArgsE",
           "_ZN12_GLOBAL__N_126grad_projected_grid_kernelENS_12SurfGridArgsE"]


def test_surface_gradient_kernels_use_no_scratch(tmp_path):
    text = device_assembly("wn_wavelet_grad_surface", tmp_path)
    assert kernels(text) == set(KERNELS), sorted(kernels(text) ^ set(KERNELS))
    for sym in KERNELS:
        assert_no_scratch(text, sym)
