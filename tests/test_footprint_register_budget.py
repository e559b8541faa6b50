"""The kernels of csrc/wn_wavelet_footprint.hip -- the per-lane kernel for each of the five entry points and the masked
texture -- compile without a private segment and within the register budget of their launch bounds: every point runs up to
eight bands of a 27-tap (or projected) evaluation, and a spill would put vector-memory traffic into each of them.  The file
is compiled with the Makefile's own command line for the device only, and the kernel descriptors are read."""
from _device_asm import descriptor, device_assembly, kernels

# FootprintOps<KIND, MASKED>: KIND 0 value, 1 projected, 2 gradient, 3 projected gradient, 4 texture (the only masked one)
OPS = ["Li0ELb0E", "Li1ELb0E", "Li2ELb0E", "Li3ELb0E", "Li4ELb0E", "Li4ELb1E"]
# kernel -> VGPR budget of its launch bounds (next_free_vgpr counts the unified file of 512 registers per SIMD lane): the
# 256-lane kernels put one wave of a workgroup on a SIMD, which may take all 512.
FOOTPRINT_KERNELS = {f"_ZN12_GLOBAL__N_123footprint_points_kernelINS_12FootprintOpsI{ops}EEEEvT_": 512 for ops in OPS}


def test_footprint_kernels_fit_their_launch_bounds_without_scratch(tmp_path):
    text = device_assembly("wn_wavelet_footprint", tmp_path)
    found = kernels(text)
    assert found == set(FOOTPRINT_KERNELS), sorted(found ^ set(FOOTPRINT_KERNELS))
    for sym, budget in FOOTPRINT_KERNELS.items():
        d = descriptor(text, sym)
        print(sym, "vgprs", d["next_free_vgpr"], "static LDS", d["group_segment_fixed_size"])
        assert d["private_segment_fixed_size"] == 0, f"{sym} has a private segment"
        assert d["next_free_vgpr"] <= budget, (sym, d["next_free_vgpr"])
        assert d["group_segment_fixed_size"] == 0, (sym, d["group_segment_fixed_size"])
