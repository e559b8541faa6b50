"""The host checks that route a dense lattice to a kernel, restated in float64 Python from the C++ planners:

  lattice_step / LatticeStep   csrc/wn_internal.hpp
  multiband_try                csrc/wn_wavelet_multiband.hip   grid3d_mbp_kernel<NB>
  strip_try                    csrc/wn_wavelet_strip.hip       grid3d_strip_kernel
  plan_sep / plan_sep_bz       csrc/wn_wavelet_grid.hip        grid3d_sep_kernel<NB, XW>
  exact_lds_try                csrc/wn_wavelet_exact.hip       grid3d_exact_lds_kernel
  brick_plan                   csrc/wn_brick.hpp               grad3d_ / curl3d_grid_sep_kernel<NB>
  bricks_call + sep_try        csrc/wn_wavelet_bricks.hip      bricks_sep_kernel<NB> (brick lists: bricks_route)
  fields_call + sep_try        csrc/wn_wavelet_brick_fields.hip    grad_ / curl_bricks_sep_kernel<NB>   (fields_bricks_route)
  bounded_bricks_call + sep_try  csrc/wn_wavelet_bounded_bricks.hip  curl_bounded_bricks_sep_kernel<NB>  (fields_bricks_route)

Every *_try returns None when its kernel takes the lattice, else the NAME of the first check that declines it: "static"
for the checks that do not involve a coordinate bound (row width, tile, alignment, z0 < 0, WN_Z_CONST ...), and "gate",
"two_mids", "K", "passes", "rowlen", "box", "step_lo", "cols", "chunk", "rows", "lds" for those that do.
value_route / deriv_route walk the entry points' chains and return (kernel label, {kernel family: declining check}).

SLACK_PER_CELL and GATE are lattice_step's two constants; the mutation checks of tests/test_gpu_far_lattice.py change them
here to see which rows of the far table move.  A plain helper module (not a conftest): the tests import it by name.
"""
import math
import os
import re

import numpy as np

f32 = np.float32

SLACK_PER_CELL = 4.8e-7   # slack = pmax * 4.8e-7: 4 float32 ulp of the largest coordinate
GATE = 1.0e6              # pmax > 1e6 cells: lattice_step refuses

MBP, STRIP, EXACT_LDS, DIRECT = "grid3d_mbp_kernel<{}>", "grid3d_strip_kernel", "grid3d_exact_lds_kernel", "grid3d_direct_kernel"
MAX_BANDS = 8


def SEP(nb, xw):
    return f"grid3d_sep_kernel<{nb},{xw}>"


class Grid:
    """GridArgs (check_grid): WN_Z_CONST calls have z0 = 0, nz = 1."""

    def __init__(self, den, nx, ny, z0, nz, base_range=4.0, octave_scale=1.0, post_scale=1.0, z_const=None):
        self.den, self.nx, self.ny = int(den), int(nx), int(ny)
        self.z_const_mode = z_const is not None
        self.z0, self.nz = (0, 1) if self.z_const_mode else (int(z0), int(nz))
        self.base_range, self.octave_scale, self.post_scale = float(f32(base_range)), float(f32(octave_scale)), float(f32(post_scale))
        self.z_const = float(f32(z_const)) if self.z_const_mode else 0.0


class LatticeStep:
    def __init__(self, step, pmax, slack):
        self.step, self.pmax, self.slack = step, pmax, slack

    def extent(self, samples):
        return int(math.floor((samples - 1) * self.step + self.slack)) + 1 + 3

    def two_mids(self):
        return 3.0 * self.step + self.slack <= 1.0


def lattice_step(g, oscale, with_z_const, signed_step, margin_cells):
    step = g.base_range * float(f32(oscale)) * g.post_scale / g.den
    if signed_step:
        step = abs(step)
    if not (step >= 0.0) or not math.isfinite(step):
        return None
    imax = max(float(g.nx), float(g.ny), abs(float(g.z0)) + g.nz)
    pmax = step * imax + (abs(g.z_const) if with_z_const else 0.0) + 1.0
    if pmax > GATE:
        return None
    return LatticeStep(step, pmax, pmax * SLACK_PER_CELL + margin_cells)


def _pow2(n):
    return n > 0 and n & (n - 1) == 0


# ---- grid3d_mbp_kernel<NB>: kBX 512, kBY 8, kBZ 8, kMaxK 5, kPasses 8, kBoxFloats 6144 -------------------------------------
def multiband_try(g, tile_n, oscales, aligned=True):
    nb = len(oscales)
    if nb < 1 or nb > 5 or not _pow2(tile_n):
        return "static"
    if g.nx <= 256 or g.nx % 4 != 0 or not aligned or g.ny <= 0 or g.nz <= 0 or g.z_const_mode or g.z0 < 0:
        return "static"
    passes = box_off = 0
    for os_ in oscales:
        ls = lattice_step(g, os_, False, False, 0.0)
        if ls is None:
            return "gate"
        if not ls.two_mids():
            return "two_mids"
        K = max(4, ls.extent(8), ls.extent(8))
        if K > 5:
            return "K"
        ex = ls.extent(512) + 1
        np_ = (ex + 63) // 64
        if passes + np_ > 8:
            return "passes"
        passes += np_
        rowlen = (ex + 3 + 3) & ~3
        if rowlen > 256:
            return "rowlen"
        box_off += K * K * rowlen
    if box_off > 6144:
        return "box"
    nbx = (g.nx + 511) // 512
    if nbx * 512 * 10 > g.nx * 11:
        return "static"
    return None


# ---- grid3d_strip_kernel: kCols 96, kPlanes 37, kMaxChunk 128 ----------------------------------------------------------------
def strip_chunk_max(ls):
    return int(min(128.0, math.floor((37 - 5 - ls.slack) / ls.step) + 1.0)) if ls.step > 0.0 else 128


def strip_try(g, tile_n, aligned=True):
    if tile_n < 4 or not _pow2(tile_n) or g.z_const_mode or g.nx <= 0 or g.ny <= 0 or g.nz <= 0 or g.z0 < 0:
        return "static"
    if g.nx % 256 != 0 or not aligned:
        return "static"
    ls = lattice_step(g, g.octave_scale, False, False, 0.0)
    if ls is None:
        return "gate"
    if ls.step < 0.18:
        return "step_lo"
    if not ls.two_mids():
        return "two_mids"
    if 255.0 * ls.step + ls.slack + 7.0 > 96.0:
        return "cols"
    if strip_chunk_max(ls) < 8:
        return "chunk"
    return None


def strip_items(g, cus):
    """(range_len, chunk_len) of a lattice the strip kernel takes: the planes of an owner range, walked in equal items of
    at most chunk_max planes.  chunk_max is the third place where slack enters strip_try."""
    ls = lattice_step(g, g.octave_scale, False, False, 0.0)
    groups = (g.nx // 256) * ((g.ny + 3) // 4)
    nranges = 1
    while groups * nranges < 2 * cus and (g.nz + 2 * nranges - 1) // (2 * nranges) >= 32:
        nranges *= 2
    range_len = (g.nz + nranges - 1) // nranges
    per_range = (range_len + strip_chunk_max(ls) - 1) // strip_chunk_max(ls)
    return range_len, (range_len + per_range - 1) // per_range


# ---- grid3d_sep_kernel<NB, XW> --------------------------------------------------------------------------------------------
def _box_rows_bound(d):
    return 36 if d == 0 else (25 if d == 1 else 16)


def _box_col_groups(d, brick_x):
    return ((brick_x // 3 >> (4 if d > 4 else d)) + 8 + 63) // 64


def _ceil_pow2(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def plan_sep_bz(g, tile_n, oscales, bz_cap):
    """(None, xw) when the brick kernel takes the lattice, else (check, xw)."""
    xw = 2 if g.nx > 256 else 1
    if xw == 2 and float((g.nx + 511) // 512 * 512) > 1.1 * float((g.nx + 255) // 256 * 256):
        xw = 1
    brick_x = 256 * xw
    nb = len(oscales)
    if nb < 1 or nb > MAX_BANDS or not _pow2(tile_n) or g.nx <= 0 or g.ny <= 0 or g.nz <= 0:
        return "static", xw
    if not g.z_const_mode and g.z0 < 0:
        return "static", xw
    BZ = bz_cap if g.nz >= bz_cap else _ceil_pow2(g.nz)
    rows = 8 * BZ
    box_total = r_total = 0
    exs = []
    for b, os_ in enumerate(oscales):
        ls = lattice_step(g, os_, True, False, 0.0)
        if ls is None:
            return "gate", xw
        if not ls.two_mids():
            return "two_mids", xw
        ey, ez = ls.extent(8), 3 if g.z_const_mode else ls.extent(BZ)
        ex = ls.extent(brick_x) + 1
        if ey > 6 or ez > 6:
            return "rows", xw
        d = nb - 1 - b
        if ey * ez > _box_rows_bound(d) or ex > 64 * _box_col_groups(d, brick_x):
            return "rows", xw
        exs.append(ex)
        box_total += ex * 37
    copies = 2 if nb == 1 else 1
    for ex in exs:
        r_total += rows * (ex | 1) + 4
    if (copies * box_total + copies * r_total) * 4 > 120 * 1024:
        return "lds", xw
    return None, xw


def plan_sep(g, tile_n, oscales):
    if len(oscales) == 1 and not g.z_const_mode and g.nz >= 16:
        why, xw = plan_sep_bz(g, tile_n, oscales, 16)
        if why is None and xw == 1:
            return None, xw
    return plan_sep_bz(g, tile_n, oscales, 8)


def sep_brick_planes(g, tile_n, oscales):
    """Planes per brick (BZ) of a lattice the brick kernel takes: 16 where plan_sep's first attempt holds (one band, no
    WN_Z_CONST, nz >= 16, 256-wide bricks, the 16 planes' box within 6 rows: extent(16) uses slack), else 8, or
    ceil_pow2(nz) for thinner slabs.  Both shapes run as grid3d_sep_kernel<1, 1>: a trace does not tell them apart."""
    if len(oscales) == 1 and not g.z_const_mode and g.nz >= 16:
        why, xw = plan_sep_bz(g, tile_n, oscales, 16)
        if why is None and xw == 1:
            return 16
    why, _ = plan_sep_bz(g, tile_n, oscales, 8)
    assert why is None, why
    return 8 if g.nz >= 8 else _ceil_pow2(g.nz)


# ---- grid3d_exact_lds_kernel: bricks of 256 x 8 x 8, 12 K floats -------------------------------------------------------------
def exact_lds_try(g, tile_n):
    if tile_n == 0 or g.nx <= 0 or g.ny <= 0 or g.nz <= 0 or g.nx < 64:
        return "static"
    ls = lattice_step(g, g.octave_scale, True, True, 1.0)
    if ls is None:
        return "gate"
    ez = 3 if g.z_const_mode else ls.extent(8)
    if ls.extent(256) * ls.extent(8) * ez > 12 * 1024:
        return "box"
    return None


def eval3d_route(g, tile_n, exact, aligned=True):
    """wn_eval3d_grid's chain."""
    why = {}
    if not exact:
        why["mbp"] = multiband_try(g, tile_n, [g.octave_scale], aligned)
        if why["mbp"] is None:
            return MBP.format(1), why
        why["strip"] = strip_try(g, tile_n, aligned)
        if why["strip"] is None:
            return STRIP, why
        why["sep"], xw = plan_sep(g, tile_n, [g.octave_scale])
        if why["sep"] is None:
            return SEP(1, xw), why
    why["exact_lds"] = exact_lds_try(g, tile_n)
    if why["exact_lds"] is None:
        return EXACT_LDS, why
    return DIRECT, why


def active_bands(s, first, nbands):
    active = 0
    while active < nbands and float(f32(s) + f32(first) + f32(active)) < 0.0:
        active += 1
    return active


def multiband3d_route(g, tile_n, exact, s, first, nbands, aligned=True):
    """wn_multiband3d_grid's chain: the plane pipeline and the brick kernel at post_scale 2, else the direct kernel."""
    why = {}
    nb = active_bands(s, first, nbands)
    if not exact and nb >= 1 and g.post_scale == 1.0 and not g.z_const_mode:
        oscales = [g.octave_scale * 2.0 ** (first + b) for b in range(nb)]
        gb = Grid(g.den, g.nx, g.ny, g.z0, g.nz, g.base_range, g.octave_scale, 2.0)
        why["mbp"] = multiband_try(gb, tile_n, oscales, aligned)
        if why["mbp"] is None:
            return MBP.format(nb), why
        why["sep"], xw = plan_sep(gb, tile_n, oscales)
        if why["sep"] is None:
            return SEP(nb, xw), why
    return DIRECT, why


# ---- the gradient and curl brick kernels: bricks of 256 x 8 x 8 --------------------------------------------------------------
def brick_plan(g, tile_n, qmuls, boxes, max_floats):
    nb = len(qmuls)
    if tile_n == 0 or nb < 1 or nb > MAX_BANDS or g.nx <= 0 or g.ny <= 0 or g.nz <= 0:
        return "static"
    total = 0
    for q in qmuls:
        ls = lattice_step(g, float(f32(g.octave_scale) * f32(q)), True, False, 0.0)
        if ls is None:
            return "gate"
        if not ls.two_mids():
            return "two_mids"
        total += boxes * (ls.extent(256) + 1) * ls.extent(8) * (3 if g.z_const_mode else ls.extent(8))
        if total > max_floats:
            return "lds"
    return None


def deriv_route(g, tile_n, exact, family, bands=None):
    """wn_eval3d_grad_grid / wn_eval3d_curl_grid (bands None) and the multiband entry points (bands = (s, first, nbands)):
    the brick kernel or the direct kernel (on the padded tile copy every tile that is not empty has)."""
    boxes, cap = (1, 12 * 1024) if family == "grad" else (3, 36 * 1024)
    sep, direct = f"{family}3d_grid_sep_kernel<{{}}>", f"{family}3d_grid_direct_kernel<{'true' if tile_n else 'false'}>"
    why = {}
    nb = 1 if bands is None else active_bands(*bands)
    if not exact and nb >= 1:
        qmuls = [1.0] if bands is None else [2.0 * 2.0 ** (bands[1] + b) for b in range(nb)]
        why["brick"] = brick_plan(g, tile_n, qmuls, boxes, cap)
        if why["brick"] is None:
            return sep.format(nb), why
    return direct, why


# ---- brick lists: bricks_sep_kernel<NB>, else bricks_exact_kernel --------------------------------------------------------------
BRICKS_REGIME_ON_WHOLE_BRICKS = True   # bricks_call checks the regime on gr; the mutation checks set it to False (on g)


def brick_constants():
    """(WN_BRICK, kBoxCap, kSepBlockCap) as include/wnoise_bricks.h and csrc/wn_wavelet_bricks.hip state them."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "wnoise_bricks.h")) as f:
        (edge,) = re.findall(r"^#define WN_BRICK (\d+)\b", f.read(), re.M)
    with open(os.path.join(root, "wavelet-noise-in-ray-tracing_amd", "csrc", "wn_wavelet_bricks.hip")) as f:
        src = f.read()
    caps = []
    for decl in (r"constexpr int kBoxCap = ([^;]+);", r"constexpr size_t kSepBlockCap = ([^;]+);"):
        (expr,) = re.findall(decl, src)
        caps.append(math.prod(int(v.strip().rstrip("u")) for v in expr.split("*")))
    assert "constexpr int kEdge = WN_BRICK" in src
    return int(edge), caps[0], caps[1]


def brick_range(g, edge=8):
    """(nbx, nby, bz0, bz1) of bricks_call: ceil(nx / 8), ceil(ny / 8), floor(z0 / 8), ceil(z1 / 8)."""
    return -(-g.nx // edge), -(-g.ny // edge), g.z0 // edge, -(-(g.z0 + g.nz) // edge)


def bricks_rounded(g, edge=8):
    """gr: the lattice rounded up to whole bricks, on which sep_try checks the regime."""
    nbx, nby, bz0, bz1 = brick_range(g, edge)
    return Grid(g.den, nbx * edge, nby * edge, bz0 * edge, (bz1 - bz0) * edge, g.base_range, g.octave_scale, g.post_scale)


def bricks_band_scales(g, bands):
    """The oscale sep_try passes to lattice_step per active band: (float)(octave_scale * qmul_b), qmul 1 or 2 * 2^(first+b)."""
    if bands is None:
        return [g.octave_scale]
    return [float(f32(g.octave_scale) * f32(2.0 * 2.0 ** (bands[1] + b))) for b in range(active_bands(*bands))]


def bricks_route(g, tile_n, exact, bands=None):
    """bricks_call + sep_try of wn_eval3d_bricks (bands None) / wn_multiband3d_bricks (bands = (s, first, nbands)):
    ("sep<NB>", None), or ("exact", check) with the first check that declines the separable kernel: "flag", "roundable",
    "no active band", "empty tile", "negative step", "gate", "two_mids", "box"; ("nothing", "empty volume") where no brick
    is in range."""
    edge, box_cap, _ = brick_constants()
    if g.nx == 0 or g.ny == 0 or g.nz == 0:
        return "nothing", "empty volume"
    if exact:
        return "exact", "flag"
    nbx, nby, bz0, bz1 = brick_range(g, edge)
    imax, imin = 2 ** 31 - 1, -2 ** 31
    if not (nbx * edge <= imax and nby * edge <= imax and bz0 * edge >= imin and bz1 * edge <= imax):
        return "exact", "roundable"
    oscales = bricks_band_scales(g, bands)
    if not oscales:
        return "exact", "no active band"
    if tile_n == 0:
        return "exact", "empty tile"
    gr = bricks_rounded(g, edge) if BRICKS_REGIME_ON_WHOLE_BRICKS else g
    for os_ in oscales:
        step = gr.base_range * float(f32(os_)) * gr.post_scale / gr.den
        if not (step >= 0.0) or not math.isfinite(step):
            return "exact", "negative step"
        ls = lattice_step(gr, os_, False, False, 0.0)
        if ls is None:
            return "exact", "gate"
        if not ls.two_mids():
            return "exact", "two_mids"
        if (ls.extent(edge) + 1) * ls.extent(edge) ** 2 > box_cap:
            return "exact", "box"
    return f"sep<{len(oscales)}>", None


# ---- gradient, curl and bounded curl brick lists: <family>_bricks_sep_kernel<NB>, else the exact kernels ------------------------
FIELD_SOURCES = {"grad": "wn_wavelet_brick_fields.hip", "curl": "wn_wavelet_brick_fields.hip", "bounded": "wn_wavelet_bounded_bricks.hip"}


def field_box_cap(family):
    """kBoxCap as the family's source file states it (both files state their own)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "wavelet-noise-in-ray-tracing_amd", "csrc", FIELD_SOURCES[family])) as f:
        (expr,) = re.findall(r"constexpr int kBoxCap = ([^;]+);", f.read())
    return math.prod(int(v.strip().rstrip("u")) for v in expr.split("*"))


def fields_bricks_route(g, tile_n, exact, family, bands=None, nobs=0):
    """fields_call + sep_try (csrc/wn_wavelet_brick_fields.hip), bounded_bricks_call + sep_try
    (csrc/wn_wavelet_bounded_bricks.hip), wn::brick_list_plan and wn::brick_sep_args (csrc/wn_brick_list.hpp) of the
    gradient, curl and bounded curl brick lists, single band (bands None) or multiband (bands = (s, first, nbands)):
    bricks_route's pairs, with the checks in the order these sources make them.  A bounded call without obstacles
    (nobs == 0) is forwarded to the curl entry point."""
    assert family in FIELD_SOURCES, family
    if family == "bounded" and nobs == 0:
        family = "curl"
    edge = brick_constants()[0]
    # brick_list_plan: an empty volume launches nothing; the range, the lattice rounded up to whole bricks
    if g.nx == 0 or g.ny == 0 or g.nz == 0:
        return "nothing", "empty volume"
    nbx, nby, bz0, bz1 = brick_range(g, edge)
    imax, imin = 2 ** 31 - 1, -2 ** 31
    roundable = nbx * edge <= imax and nby * edge <= imax and bz0 * edge >= imin and bz1 * edge <= imax
    # fields_call / bounded_bricks_call: the flag; a multiband call with no active band skips sep_try
    if exact:
        return "exact", "flag"
    nb = 1 if bands is None else active_bands(*bands)
    if bands is not None and nb < 1:
        return "exact", "no active band"
    qmul = [1.0] if bands is None else [float(f32(2.0) * f32(2.0 ** (bands[1] + b))) for b in range(nb)]
    # brick_sep_args
    if tile_n == 0:
        return "exact", "empty tile"
    if not roundable:
        return "exact", "roundable"
    if nb > MAX_BANDS:
        return "exact", "bands"
    gr = Grid(g.den, nbx * edge, nby * edge, bz0 * edge, (bz1 - bz0) * edge, g.base_range, g.octave_scale, g.post_scale) \
        if BRICKS_REGIME_ON_WHOLE_BRICKS else g
    box_cap = field_box_cap(family)
    for q in qmul:
        os_ = float(f32(g.octave_scale) * f32(q))
        ls = lattice_step(gr, os_, False, False, 0.0)
        if ls is None:
            step = gr.base_range * os_ * gr.post_scale / gr.den      # lattice_step refuses a negative step and the gate alike
            return "exact", "negative step" if not (step >= 0.0) or not math.isfinite(step) else "gate"
        if not ls.two_mids():
            return "exact", "two_mids"
        if (ls.extent(edge) + 1) * ls.extent(edge) * ls.extent(edge) > box_cap:
            return "exact", "box"
    return f"sep<{nb}>", None
