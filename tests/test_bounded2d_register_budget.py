"""The kernels of csrc/wn_wavelet_bounded2d.hip -- the dense kernel, the point kernel and the advection kernel of each method,
each with the tile in LDS or gathered from global memory -- compile for gfx950 without a private segment and within the
register budget their own launch bounds declare: kWorkgroupsPerCu workgroups of kWorkgroup lanes share a CU.  The bounded
kernels carry the ramp, its gradient and the stream function's value through every evaluation on top of what the unbounded
kernels of csrc/wn_wavelet_curl2d.hip hold, and a spill would put vector-memory traffic into every band of every stage of
every step.  The LDS forms declare no static LDS: their whole allocation is the dynamic size the host requests.  The file
is compiled with the Makefile's own command line for the device only, and the kernel descriptors are read; no instruction
is inspected."""
import os
import re

from _device_asm import PKG, descriptor, device_assembly, kernels

B = {False: "Lb0E", True: "Lb1E"}
GRID = [f"_ZN12_GLOBAL__N_126curl2d_bounded_grid_kernelI{B[l]}EEvNS_13Bounded2dArgsE" for l in B]
POINTS = [f"_ZN12_GLOBAL__N_128curl2d_bounded_points_kernelI{B[l]}EEvNS_13Bounded2dArgsE" for l in B]
ADVECT = [f"_ZN12_GLOBAL__N_128curl2d_bounded_advect_kernelILi{m}E{B[l]}EEvNS_19BoundedAdvect2dArgsE" for m in range(3) for l in B]
CU_LDS = 160 * 1024


def source():
    return open(os.path.join(PKG, "csrc", "wn_wavelet_bounded2d.hip")).read()


def shape():
    """(lanes per workgroup, workgroups per CU): the two named constants of the source."""
    src = source()
    wg = re.search(r"^#define WN_BOUNDED2D_WORKGROUP (\d+)$", src, re.M)
    per_cu = re.search(r"^#define WN_BOUNDED2D_WORKGROUPS_PER_CU (\d+)$", src, re.M)
    assert wg and per_cu, "the workgroup shape is two named constants"
    assert src.count("__launch_bounds__(kWorkgroup, kWavesPerSimd)") == 3, "every kernel declares the file's shape"
    assert "kWavesPerSimd = kWorkgroupsPerCu * kWorkgroup / 256;" in src
    return int(wg.group(1)), int(per_cu.group(1))


def test_bounded2d_kernels_fit_their_launch_bounds_without_scratch(tmp_path):
    text = device_assembly("wn_wavelet_bounded2d", tmp_path)
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


def test_the_staged_tiles_of_a_cu_fit_its_lds_and_the_thresholds_are_the_unbounded_files():
    src = source()
    m = re.search(r"constexpr size_t kLdsTileMaxBytes = (\d+) \* 1024;", src)
    assert m, "the fit threshold is one named constant"
    limit = int(m.group(1)) * 1024
    _, per_cu = shape()
    padded = lambda n: n * (n + 2) * 4                          # noqa: E731  what lds_tile_bytes requests
    assert padded(128) <= limit < padded(256)
    assert per_cu * limit <= CU_LDS
    # routed as the unbounded kernels are: the same fit threshold and the same two list lengths
    other = open(os.path.join(PKG, "csrc", "wn_wavelet_curl2d.hip")).read()
    assert re.search(r"constexpr size_t kLdsTileMaxBytes = (\d+) \* 1024;", other).group(1) == m.group(1)
    for mine, theirs in (("WN_BOUNDED2D_POINTS_LDS_MIN_POINTS", "WN_CURL2D_POINTS_LDS_MIN_POINTS"),
                         ("WN_BOUNDED2D_ADVECT_LDS_MIN_POINTS", "WN_ADVECT2D_LDS_MIN_POINTS")):
        a = re.search(rf"^#define {mine} (\d+)$", src, re.M)
        b = re.search(rf"^#define {theirs} (\d+)$", other, re.M)
        assert a and b and a.group(1) == b.group(1), (mine, theirs)
