"""The kernels of csrc/wn_wavelet_multiband2d.hip -- the dense kernel (value / gradient, tile in LDS / gathered from global
memory) and the point kernel (value / gradient, uniform / per-point s, LDS / global) -- compile without a private segment and
within the register budget of their launch bounds: two workgroups of 1024 lanes share a CU (the LDS form needs both to hide
its reads), which leaves 64 VGPRs a lane, and a spill would put vector-memory traffic into every band of every sample.  The
LDS forms declare no static LDS: their whole allocation is the dynamic size the host requests, n * (n + 2) floats, which
must fit twice into a CU's 160 KiB for a 128^2 tile and not at all for a 256^2 one.  The file is compiled with the
Makefile's own command line for the device only, and the kernel descriptors are read; no instruction is inspected."""
import os
import re

from _device_asm import PKG, descriptor, device_assembly, kernels

B = {False: "Lb0E", True: "Lb1E"}
GRID = [f"_ZN12_GLOBAL__N_123multiband2d_grid_kernelI{B[g]}{B[l]}EEvNS_8Mb2dArgsE" for g in B for l in B]
POINTS = [f"_ZN12_GLOBAL__N_125multiband2d_points_kernelI{B[g]}{B[p]}{B[l]}EEvNS_8Mb2dArgsE" for g in B for p in B for l in B]
WORKGROUP, WORKGROUPS_PER_CU, CU_LDS = 1024, 2, 160 * 1024
# 512 registers per SIMD lane, shared by the waves of WORKGROUPS_PER_CU workgroups: 2 * 1024 / 64 waves on 4 SIMDs
VGPR_BUDGET = 512 // (WORKGROUPS_PER_CU * WORKGROUP // 64 // 4)


def test_multiband2d_kernels_fit_their_launch_bounds_without_scratch(tmp_path):
    text = device_assembly("wn_wavelet_multiband2d", tmp_path)
    found = kernels(text)
    assert found == set(GRID + POINTS), sorted(found ^ set(GRID + POINTS))
    assert VGPR_BUDGET == 64
    for sym in GRID + POINTS:
        d = descriptor(text, sym)
        print(sym, "vgprs", d["next_free_vgpr"], "static LDS", d["group_segment_fixed_size"])
        assert d["private_segment_fixed_size"] == 0, f"{sym} has a private segment"
        assert d["next_free_vgpr"] <= VGPR_BUDGET, (sym, d["next_free_vgpr"])
        assert d["group_segment_fixed_size"] == 0, (sym, d["group_segment_fixed_size"])   # dynamic LDS only


def test_the_lds_form_takes_the_128_tile_twice_per_cu_and_not_the_256_tile():
    src = open(os.path.join(PKG, "csrc", "wn_wavelet_multiband2d.hip")).read()
    m = re.search(r"#define WN_MB2D_LDS_TILE_MAX_BYTES \((\d+) \* 1024\)", src)
    assert m, "the fit threshold is one named constant"
    limit = int(m.group(1)) * 1024
    assert f"#define WN_MB2D_WORKGROUP {WORKGROUP}\n" in src and f"kWorkgroupsPerCu = {WORKGROUPS_PER_CU};" in src
    padded = lambda n: n * (n + 2) * 4                          # noqa: E731  what lds_tile_bytes requests
    assert padded(128) == 66560 and padded(128) <= limit < padded(256)
    assert WORKGROUPS_PER_CU * limit <= CU_LDS
