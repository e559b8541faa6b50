"""The kernels of csrc/wn_perlin_footprint.hip -- the per-lane kernel and the sorted kernel for each of the five entry
points and the masked texture -- compile without a private segment and within the register budget of their launch bounds:
every point runs up to sixteen octaves of fp64 noise, and a spill would put vector-memory traffic into each of them.  The
sorted kernel's static LDS is the 2 KB of sorted indices, the 512-byte table and the bins.  The file is compiled with the
Makefile's own command line for the device only, and the kernel descriptors are read."""
from _device_asm import descriptor, device_assembly, kernels

# PerlinFootprintOps<KIND, MASKED>: KIND 0 turb, 1 fractal, 2 turb gradient, 3 fractal gradient, 4 texture (the only masked one)
OPS = ["Li0ELb0E", "Li1ELb0E", "Li2ELb0E", "Li3ELb0E", "Li4ELb0E", "Li4ELb1E"]
# kernel -> (VGPR budget, static LDS).  The launch bounds of a 256-lane kernel would allow all 512 registers of a SIMD lane; the
# budget is 128, which keeps four waves on a SIMD: these kernels are bound by fp64 VALU issue and hide its latency with
# waves, and DESIGN.md's account of them rests on that occupancy.
KERNELS = {f"_ZN12_GLOBAL__N_130perlin_footprint_points_kernelINS_18PerlinFootprintOpsI{ops}EEEEvT_": (128, 512) for ops in OPS}
KERNELS.update({f"_ZN12_GLOBAL__N_130perlin_footprint_sorted_kernelINS_18PerlinFootprintOpsI{ops}EEEEvT_m":
                (128, 512 + 2 * 1024 + 4 * 17) for ops in OPS})


def test_perlin_footprint_kernels_fit_their_launch_bounds_without_scratch(tmp_path):
    text = device_assembly("wn_perlin_footprint", tmp_path)
    found = kernels(text)
    assert found == set(KERNELS), sorted(found ^ set(KERNELS))
    for sym, (budget, lds) in KERNELS.items():
        d = descriptor(text, sym)
        print(sym, "vgprs", d["next_free_vgpr"], "static LDS", d["group_segment_fixed_size"])
        assert d["private_segment_fixed_size"] == 0, f"{sym} has a private segment"
        assert d["next_free_vgpr"] <= budget, (sym, d["next_free_vgpr"])
        assert d["group_segment_fixed_size"] == lds, (sym, d["group_segment_fixed_size"])
