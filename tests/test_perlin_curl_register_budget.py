"""The Perlin curl kernels of csrc/wn_perlin_curl.hip (points, the generic grid kernel and the three run-form
instantiations) compile without a private segment and within the register budget of their launch bounds: the run form keeps
24 running sums per lane in registers, and a spill would put vector-memory traffic into every sample.  The file is compiled
with the Makefile's own command line for the device only, and the kernel descriptors are read."""
from _device_asm import descriptor, device_assembly, kernels

# kernel -> VGPR budget of its launch bounds (next_free_vgpr counts the unified file of 512 registers per SIMD lane): the
# 256-lane kernels put one wave of a workgroup on a SIMD, which may take all 512; the run form's 8 waves per workgroup put
# two on a SIMD, which share them: 256 each.
CURL_KERNELS = {"_ZN12_GLOBAL__N_131perlin_curl_grid_generic_kernelENS_18PerlinCurlGridArgsE": 512,
                "_ZN12_GLOBAL__N_125perlin_curl_points_kernelENS_20PerlinCurlPointsArgsE": 512,
                "_ZN12_GLOBAL__N_127perlin_curl_grid_run_kernelILi0EEEvNS_18PerlinCurlGridArgsE": 256,
                "_ZN12_GLOBAL__N_127perlin_curl_grid_run_kernelILi1EEEvNS_18PerlinCurlGridArgsE": 256,
                "_ZN12_GLOBAL__N_127perlin_curl_grid_run_kernelILi2EEEvNS_18PerlinCurlGridArgsE": 256}


def test_perlin_curl_kernels_fit_their_launch_bounds_without_scratch(tmp_path):
    text = device_assembly("wn_perlin_curl", tmp_path)
    found = kernels(text)
    assert found == set(CURL_KERNELS), sorted(found ^ set(CURL_KERNELS))
    for sym, budget in CURL_KERNELS.items():
        d = descriptor(text, sym)
        print(sym, "vgprs", d["next_free_vgpr"], "static LDS", d["group_segment_fixed_size"])
        assert d["private_segment_fixed_size"] == 0, f"{sym} has a private segment"
        assert d["next_free_vgpr"] <= budget, (sym, d["next_free_vgpr"])
