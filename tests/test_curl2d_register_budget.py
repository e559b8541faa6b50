"""The kernels of csrc/wn_wavelet_curl2d.hip -- the dense kernel, the point kernel and the advection kernel of each method,
each with the tile in LDS or gathered from global memory -- compile for gfx950 without a private segment and within the
register budget their launch bounds declare: kWorkgroupsPerCu workgroups of kWorkgroup lanes share a CU, and a spill would put
vector-memory traffic into every band of every stage of every step.  The LDS forms declare no static LDS: their whole
allocation is the dynamic size the host requests, n * (n + 2) floats.  The file is compiled with the Makefile's own command
line for the device only, and the kernel descriptors are read; no instruction is inspected."""
import os
import re

from _device_asm import PKG, descriptor, device_assembly, kernels

B = {False: "Lb0E", True: "Lb1E"}
GRID = [f"_ZN12_GLOBAL__N_118curl2d_grid_kernelI{B[l]}EEvNS_10Curl2dArgsE" for l in B]
POINTS = [f"_ZN12_GLOBAL__N_120curl2d_points_kernelI{B[l]}EEvNS_10Curl2dArgsE" for l in B]
ADVECT = [f"_ZN12_GLOBAL__N_120curl2d_advect_kernelILi{m}E{B[l]}EEvNS_12Advect2dArgsE" for m in range(3) for l in B]
CU_LDS = 160 * 1024


def shape():
    """(lanes per workgroup, workgroups per CU): the two named constants of the source."""
    src = open(os.path.join(PKG, "csrc", "wn_wavelet_curl2d.hip")).read()
    wg = re.search(r"^#define WN_CURL2D_WORKGROUP (\d+)$", src, re.M)
    per_cu = re.search(r"^#define WN_CURL2D_WORKGROUPS_PER_CU (\d+)$", src, re.M)
    assert wg and per_cu, "the workgroup shape is two named constants"
    assert "__launch_bounds__(kWorkgroup, kWavesPerSimd)" in src and "kWavesPerSimd = kWorkgroupsPerCu * kWorkgroup / 256;" in src
    return int(wg.group(1)), int(per_cu.group(1))


def test_curl2d_kernels_fit_their_launch_bounds_without_scratch(tmp_path):
    text = device_assembly("wn_wavelet_curl2d", tmp_path)
    found = kernels(text)
    want = set(GRID + POINTS + ADVECT)
    assert found == want, sorted(found ^ want)
    workgroup, per_cu = shape()
    # 512 registers per SIMD lane, shared by the waves of per_cu workgroups on 4 SIMDs
    budget = 512 // (per_cu * workgroup // 64 // 4)
    assert budget in (64, 128), budget
    for sym in sorted(want):
        d = descriptor(text, sym)
        print(sym, "vgprs", d["next_free_vgpr"], "static LDS", d["group_segment_fixed_size"])
        assert d["private_segment_fixed_size"] == 0, f"{sym} has a private segment"
        assert d["next_free_vgpr"] <= budget, (sym, d["next_free_vgpr"], budget)
        assert d["group_segment_fixed_size"] == 0, (sym, d["group_segment_fixed_size"])   # dynamic LDS only


def test_the_staged_tiles_of_a_cu_fit_its_lds():
    src = open(os.path.join(PKG, "csrc", "wn_wavelet_curl2d.hip")).read()
    m = re.search(r"constexpr size_t kLdsTileMaxBytes = (\d+) \* 1024;", src)
    assert m, "the fit threshold is one named constant"
    limit = int(m.group(1)) * 1024
    _, per_cu = shape()
    padded = lambda n: n * (n + 2) * 4                          # noqa: E731  what lds_tile_bytes requests
    assert padded(128) == 66560 and padded(128) <= limit < padded(256)
    assert per_cu * limit <= CU_LDS
