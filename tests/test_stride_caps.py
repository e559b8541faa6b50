"""CPU: the workgroup caps of the grid-stride launches, read out of csrc/, equal their mirrors in
tests/test_gpu_stride_pass.py.  That module sizes every call as P + a few workgroups, P = cap * lanes; after a cap is
raised its calls take one trip again and test nothing of what they are for, so raising a cap must fail here first."""
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import test_gpu_stride_pass as sp  # noqa: E402

CSRC = os.path.join(ROOT, "wavelet-noise-in-ray-tracing_amd", "csrc")


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def product(expr):
    """`256u * 8u * 8u`, `16 * 4096`, `(80 * 1024)`, `2`: a product of unsigned integer literals."""
    expr = expr.strip().strip("()")
    factors = [f.strip() for f in expr.split("*")]
    assert all(re.fullmatch(r"\d+u?", f) for f in factors), expr
    out = 1
    for f in factors:
        out *= int(f.rstrip("u"))
    return out


def constexpr(name, text):
    found = re.findall(r"constexpr\s+(?:size_t|int)\s+" + name + r"\s*=\s*([^;]+);", text)
    assert len(found) == 1, (name, found)
    return product(found[0])


def macro(name, text):
    found = re.findall(r"^#define\s+" + name + r"\s+(.+)$", text, re.M)
    assert len(found) == 1, (name, found)
    return product(found[0])


def test_the_default_cap_of_stride_blocks():
    text = source("wn_internal.hpp")
    assert constexpr("kStrideBlockCap", text) == sp.STRIDE_BLOCK_CAP
    assert re.search(r"stride_blocks\(size_t total, size_t cap = kStrideBlockCap\)", text)
    assert sp.P_DEFAULT == sp.STRIDE_BLOCK_CAP * sp.LANES == 4194304


def test_the_caps_of_the_grid_curl_and_advection_kernels():
    assert constexpr("kBlockCap", source("wn_wavelet_grid.hip")) == sp.BLOCK_CAP
    assert constexpr("kPointBlockCap", source("wn_wavelet_curl.hip")) == sp.POINT_BLOCK_CAP
    assert constexpr("kAdvectBlockCap", source("wn_wavelet_advect.hip")) == sp.ADVECT_BLOCK_CAP
    assert sp.P_GRID == sp.BLOCK_CAP * sp.LANES and sp.P_ADVECT == sp.ADVECT_BLOCK_CAP * sp.LANES


def test_the_multiband2d_launch():
    text = source("wn_wavelet_multiband2d.hip")
    assert macro("WN_MB2D_WORKGROUP", text) == sp.MB2D_WORKGROUP
    assert constexpr("kWorkgroupsPerCu", text) == sp.MB2D_WORKGROUPS_PER_CU
    assert macro("WN_MB2D_POINTS_LDS_MIN_POINTS", text) == sp.MB2D_LDS_MIN_POINTS
    assert macro("WN_MB2D_LDS_TILE_MAX_BYTES", text) == 80 * 1024      # test_multiband2d_lds_tile_boundary's 142 and 144
    # the launch the mirrors describe: min(spans, kWorkgroupsPerCu * CUs) workgroups of kWorkgroup lanes
    assert "cap = (size_t)kWorkgroupsPerCu * wn::device_compute_units(dev)" in text
    assert "dim3 grid((unsigned)(spans < cap ? spans : cap))" in text


def test_every_capped_launch_has_256_lanes():
    """P = cap * 256 for every stride_blocks call site: each launches dim3(256) (kLanes = 256 in wn_perlin_footprint.hip)."""
    sites = 0
    for name in sorted(os.listdir(CSRC)):
        text = source(name)
        for m in re.finditer(r"stride_blocks\(", text):
            if "inline int stride_blocks" in text[max(0, m.start() - 11):m.end()]:
                continue
            sites += 1
            stmt = text[m.start():text.index(";", m.start())]
            if "dim3(256)" in stmt or "dim3(kLanes)" in stmt:
                continue
            # `const dim3 grid(stride_blocks(..)), block(256);`, or a block(256) declared for the launches that follow
            after = text[m.start():m.start() + 400]
            assert "block(256)" in after or "dim3 block(256)" in text, (name, stmt)
    assert sites >= 25, sites
    assert constexpr("kLanes", source("wn_perlin_footprint.hip")) == sp.LANES
