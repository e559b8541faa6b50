"""The Perlin gradient kernels of csrc/wn_perlin_grad.hip (points, the generic grid kernel and the three run-form
instantiations) compile without scratch: the run form keeps 24 running sums per lane in registers, and a spill would put
vector-memory traffic into every sample.  The value kernels of csrc/wn_perlin.hip are not this feature's to change: their
VGPR counts, static LDS and scratch are pinned to the figures they had before the gradient was added.  Both files are
compiled with the Makefile's own command line for the device only, and the kernel descriptors are read."""
from _device_asm import assert_no_scratch, descriptor, device_assembly, kernels

GRAD_KERNELS = ["_ZN12_GLOBAL__N_131perlin_grad_grid_generic_kernelENS_18PerlinGradGridArgsE",
                "_ZN12_GLOBAL__N_125perlin_grad_points_kernelENS_20PerlinGradPointsArgsE",
                "_ZN12_GLOBAL__N_127perlin_grad_grid_run_kernelILi0EEEvNS_18PerlinGradGridArgsE",
                "_ZN12_GLOBAL__N_127perlin_grad_grid_run_kernelILi1EEEvNS_18PerlinGradGridArgsE",
                "_ZN12_GLOBAL__N_127perlin_grad_grid_run_kernelILi2EEEvNS_18PerlinGradGridArgsE"]

# kernel -> (next_free_vgpr, static group segment bytes) of csrc/wn_perlin.hip before this feature
VALUE_KERNELS = {"_ZN12_GLOBAL__N_126perlin_grid_generic_kernelENS_14PerlinGridArgsE": (54, 512),
                 "_ZN12_GLOBAL__N_120perlin_points_kernelENS_16PerlinPointsArgsE": (64, 512),
                 "_ZN12_GLOBAL__N_122perlin_grid_run_kernelILi0ELi16EEEvNS_14PerlinGridArgsE": (80, 0),
                 "_ZN12_GLOBAL__N_122perlin_grid_run_kernelILi1ELi16EEEvNS_14PerlinGridArgsE": (90, 0),
                 "_ZN12_GLOBAL__N_122perlin_grid_run_kernelILi2ELi16EEEvNS_14PerlinGridArgsE": (94, 0),
                 "_ZN12_GLOBAL__N_122perlin_grid_run_kernelILi0ELi8EEEvNS_14PerlinGridArgsE": (80, 0),
                 "_ZN12_GLOBAL__N_122perlin_grid_run_kernelILi1ELi8EEEvNS_14PerlinGridArgsE": (90, 0),
                 "_ZN12_GLOBAL__N_122perlin_grid_run_kernelILi2ELi8EEEvNS_14PerlinGridArgsE": (96, 0),
                 "_ZN12_GLOBAL__N_120noise_texture_kernelILb1EEEvNS_12NoiseTexArgsE": (56, 8704),
                 "_ZN12_GLOBAL__N_120noise_texture_kernelILb0EEEvNS_12NoiseTexArgsE": (60, 512)}


def test_perlin_gradient_kernels_use_no_scratch(tmp_path):
    text = device_assembly("wn_perlin_grad", tmp_path)
    found = kernels(text)
    assert found == set(GRAD_KERNELS), sorted(found ^ set(GRAD_KERNELS))
    for sym in GRAD_KERNELS:
        assert_no_scratch(text, sym)
        d = descriptor(text, sym)
        print(sym, "vgprs", d["next_free_vgpr"], "static LDS", d["group_segment_fixed_size"])
        # the run form is launched with 8 waves per workgroup: two waves per SIMD share its 512 registers
        assert d["next_free_vgpr"] <= 256


def test_perlin_value_kernels_keep_their_resources(tmp_path):
    text = device_assembly("wn_perlin", tmp_path)
    found = kernels(text)
    assert found == set(VALUE_KERNELS), sorted(found ^ set(VALUE_KERNELS))
    for sym, (vgprs, lds) in VALUE_KERNELS.items():
        assert_no_scratch(text, sym)
        d = descriptor(text, sym)
        assert (d["next_free_vgpr"], d["group_segment_fixed_size"]) == (vgprs, lds), (sym, d["next_free_vgpr"],
                                                                                        d["group_segment_fixed_size"])
