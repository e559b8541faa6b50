"""Which point-list, texture and Perlin-grid kernel serves which call, and is its answer right on every point.

wn_eval3d_points, wn_multiband3d_points and wn_wavelet_texture_points (csrc/wn_wavelet_points.hip) send a call to the
grid-stride kernels (eval3d_points_kernel<P>, multiband3d_points_kernel<P>, wavelet_texture_kernel<MASKED, PADDED>), to
plane_sorted_points_kernel<Ops, false> for lists of at least kSortMinPoints (65,536) points, or to the pair
plane_sorted_points_kernel<Ops, true> + row_slab_points_kernel<Ops> for unmasked lists of at least kSlabMinPoints
(16,777,216) points on a padded 128^3 tile.  perlin_grid (csrc/wn_perlin.hip) uses perlin_grid_run_kernel<kind, 8 | 16>
for rows of >= 128 samples and 1..8 octaves, else perlin_grid_generic_kernel.  All of them are bit-exact, so a value
test alone passes whichever kernel ran, and a refused LDS opt-in falls back to a slower kernel without an error.

POINT_ROUTES pins the kernel: each row is one ABI call and the kernels the host checks give it, in dispatch order.
test_point_routes_reach_the_kernels_they_name runs every row once in a child process under `rocprofv3 --kernel-trace`.
test_point_route_values compares every row's output with the oracle on every element.  test_row_slab_streams runs
streams built to reach the row-slab kernel's edges (wrapped rows, a row boundary, the third-row plane limit, reloads
and wrong guesses inside the trust window, interleaved kept and deferred chunks, partial last chunks, output that
already holds the defer mark, kept chunks whose NaN inputs put the mark's bits into some of their 16 mark positions);
defer_model, a numpy restatement of the DEFER predicate, proves on the CPU that each stream defers the chunks it is meant
to.

Run as `python tests/test_gpu_point_dispatch.py --child` it is that child: the calls of POINT_ROUTES, one after the other.
"""
import csv
import glob
import importlib
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

SEED32 = 4242                 # the 32^3 tile is generated on the device
CHUNK = 4096                  # kSortChunk
SORT_MIN = 16 * CHUNK         # kSortMinPoints
SLAB_MIN = 16 * 256 * CHUNK   # kSlabMinPoints
SLAB_TRUST = 15               # kSlabTrust
THIRD_PLANES = 55             # kSlabThirdPlanes: (4096 * 4 + 4096 * 4 + 4096 * 2) / (130 * 4)
DEFER_BITS = 0xffc0de42       # kDeferredBits
TEX_CELLS = 32.0              # wavelet_texture at scale 1, octave 4: texture coordinate = 32 * p
SENTINEL_BITS = 0x7fa5a5a5    # a NaN no evaluation produces: what an element no kernel wrote still holds
W5 = [1.0, 0.5, 2.0, 1.0, 0.25]


# ---- kernel labels ---------------------------------------------------------------------------------------------------
def _b(v):
    return "true" if v else "false"


def TEX_OPS(masked, padded):
    return f"TextureOps<{_b(masked)},{_b(padded)}>"


def EV_OPS(padded, multiband):
    return f"Eval3dOps<{_b(padded)},{_b(multiband)}>"


def SORTED(ops, defer=False):
    return f"plane_sorted_points_kernel<{ops},{_b(defer)}>"


def PAIR(ops):
    return (SORTED(ops, True), f"row_slab_points_kernel<{ops}>")


def EV3(padded):
    return f"eval3d_points_kernel<{_b(padded)}>"


def MB3(padded):
    return f"multiband3d_points_kernel<{_b(padded)}>"


def TEXK(masked, padded):
    return f"wavelet_texture_kernel<{_b(masked)},{_b(padded)}>"


def RUN(kind, waves):  # kind: 0 noise, 1 turb, 2 fractal
    return f"perlin_grid_run_kernel<{kind},{waves}>"


GENERIC = "perlin_grid_generic_kernel"
EV2, PROJ_PTS, MB_PROJ = "eval2d_points_kernel", "eval3d_projected_points_kernel", "multiband3d_projected_points_kernel"
GRID2D, PROJ_GRID = "grid2d_direct_kernel", "grid3d_projected_kernel"

KERNEL_BASES = ("eval3d_points_kernel", "eval2d_points_kernel", "eval3d_projected_points_kernel",
                "multiband3d_points_kernel", "multiband3d_projected_points_kernel", "wavelet_texture_kernel",
                "plane_sorted_points_kernel", "row_slab_points_kernel", "perlin_grid_run_kernel",
                "perlin_grid_generic_kernel", "grid2d_direct_kernel", "grid3d_projected_kernel")


# ---- streams: (n, 3) float32 points in the evaluator's cell coordinates (tile period 128) ------------------------------
def _rng(n, salt):
    return np.random.default_rng(1000003 * salt + n)


def scatter(n, salt=1, **_):
    """Uniform in all three dimensions: sorted, never deferred (no dominant row)."""
    return _rng(n, salt).uniform(-320.0, 320.0, (n, 3)).astype(np.float32)


def surface(n, row=0.0, salt=2, zlo=-320.0, zhi=320.0, **_):
    """Hits on the axis-aligned plane y = row, x and z scattered: every full chunk is deferred to the slab kernel."""
    r = _rng(n, salt)
    x = r.uniform(-320.0, 320.0, n)
    z = r.uniform(zlo, zhi, n)
    return np.stack([x, np.full(n, row), z], 1).astype(np.float32)


def boundary(n, row=42, salt=3, **_):
    """y exactly on the middle-row boundary row + 0.5 (middle row `row`), one point in seven one ulp above it (middle
    row `row` + 1) and one in seven one ulp below it (`row`): chunks split between ry and ry + 1."""
    p = surface(n, row + 0.5, salt)
    i = np.arange(n)
    y0 = np.float32(row + 0.5)
    p[i % 7 == 3, 1] = np.nextafter(y0, np.float32(np.inf))
    p[i % 7 == 5, 1] = np.nextafter(y0, np.float32(-np.inf))
    return p


def planes(n, lo=0, hi=127, row=77.0, salt=4, **_):
    """A surface whose z middles are the planes lo..hi only."""
    return surface(n, row, salt, lo - 0.499, hi + 0.5)


def rows_by_visit(n, period=1, rows=(5.0, 90.0, 127.0), cus=256, salt=5, **_):
    """A surface whose row changes with the chunk's place in its slab workgroup's sequence (chunk c is visit c // cus of
    workgroup c % cus): visit j lies on rows[(j // period) % 3].  Visits 0, 16, 32 ... are looked at (each after 15 trusted
    ones) and find another row than the resident one: a reload; the trusted visits in between are wrong guesses."""
    p = surface(n, 0.0, salt)
    visit = (np.arange(n) // CHUNK) // cus
    p[:, 1] = np.asarray(rows, np.float32)[(visit // period) % len(rows)]
    return p


def interleaved(n, row=64.0, salt=6, nan_bits=None, **_):
    """Chunks alternate: even ones coherent (a row of x in stream order, one plane per 512 points: kept and evaluated in
    stream order by the plane-ordered kernel), odd ones scattered on the surface y = row (deferred).  nan_bits: the even
    chunks' points 64 w for the odd w < 16 (none of them in the DEFER sample) get NaN coordinates with these bits."""
    p = surface(n, row, salt)
    i = np.arange(n)
    even = (i // CHUNK) % 2 == 0
    k = i % CHUNK
    p[even, 0] = (-300.0 + 0.125 * k[even]).astype(np.float32)
    p[even, 2] = (np.float32(3.0) + (i[even] // 512) % 128).astype(np.float32)
    if nan_bits is not None:
        p[even & (k % 128 == 64) & (k < 16 * 64)] = np.uint32(nan_bits).view(np.float32)
    return p


def small(n, salt=8, **_):
    """Points of a few cells' extent around the origin (multiband lists scale them by up to 2^(first + nbands))."""
    return _rng(n, salt).uniform(-6.0, 6.0, (n, 3)).astype(np.float32)


STREAMS = {"scatter": scatter, "surface": surface, "boundary": boundary, "planes": planes,
           "rows_by_visit": rows_by_visit, "interleaved": interleaved, "small": small}


def build_stream(spec, n, cus=256):
    name, kw = spec if isinstance(spec, tuple) else (spec, {})
    kw = dict(kw)
    if name == "rows_by_visit":
        kw["cus"] = cus
    return STREAMS[name](n, **kw)


def to_texture(cells):
    """Texture-space points whose texture coordinate (float)(p * 1.0) * 32 is `cells` again, exactly."""
    return (cells / np.float32(TEX_CELLS)).astype(np.float32)


# ---- the table -------------------------------------------------------------------------------------------------------
# A row: (name, entry, tile, stream, n, extra, kernels).  Tiles: t128 (128^3, seed 12345), t32 (generated, seed 4242),
# t8 / t16 / t6 (tests/golden; 6 is not a power of two), empty (no coefficients), null (no tile), t2d (128^2, seed 12345).
# Every 3-D tile with coefficients has a padded copy (wn_tilegen.hip, tile_build_padded): Ops<PADDED = true>.
# Host conditions (wn_wavelet_points.hip): sorted -- n >= kSortMinPoints and a tile with n > 0 (for WMultibandNoise also
# nbands >= 1 after `s`, for textures the 3-D branch); pair -- additionally unmasked, tile n == 128 and n >= kSlabMinPoints,
# and the runtime granting the slab kernel its dynamic LDS (launch_row_slab).  Perlin (wn_perlin.hip, perlin_grid): run
# kernel for nx >= 128 and 1..8 octaves (16 waves above 2 octaves), provided its LDS opt-in is granted; else generic.
POINT_ROUTES = [
    # -- WaveletNoise::evaluate3D
    ("e3_65535", "e3", "t128", "scatter", SORT_MIN - 1, None, (EV3(True),)),
    ("e3_65536", "e3", "t128", "scatter", SORT_MIN, None, (SORTED(EV_OPS(True, False)),)),
    ("e3_slab_below", "e3", "t128", "surface", SLAB_MIN - 1, None, (SORTED(EV_OPS(True, False)),)),
    ("e3_slab_at", "e3", "t128", "surface", SLAB_MIN, None, PAIR(EV_OPS(True, False))),
    ("e3_t32_long", "e3", "t32", "surface", SLAB_MIN, None, (SORTED(EV_OPS(True, False)),)),    # n != 128: no slab
    ("e3_t6_sorted", "e3", "t6", "scatter", SORT_MIN, None, (SORTED(EV_OPS(True, False)),)),    # the POW2 = false form
    ("e3_t8_sorted", "e3", "t8", "scatter", 70000, None, (SORTED(EV_OPS(True, False)),)),
    ("e3_empty_long", "e3", "empty", "scatter", 70000, None, (EV3(False),)),                     # n == 0, no padded copy
    # -- WMultibandNoise (extra: s, first band, nbands, weights)
    ("mb_65535", "mb", "t128", "small", SORT_MIN - 1, (-16.0, -2, 5, W5), (MB3(True),)),
    ("mb_65536", "mb", "t128", "small", SORT_MIN, (-16.0, -2, 5, W5), (SORTED(EV_OPS(True, True)),)),
    ("mb_s_cuts_all", "mb", "t128", "small", 70000, (0.0, 0, 5, W5), (MB3(True),)),              # nbands == 0 after s
    ("mb_t6_sorted", "mb", "t6", "small", 70000, (-16.0, -1, 3, W5[:3]), (SORTED(EV_OPS(True, True)),)),
    # -- wavelet_texture::value (extra: use_3d, masked)
    ("tx_65535", "tex", "t128", "scatter", SORT_MIN - 1, (True, False), (TEXK(False, True),)),
    ("tx_65535_masked", "tex", "t128", "scatter", SORT_MIN - 1, (True, True), (TEXK(True, True),)),
    ("tx_65536", "tex", "t128", "scatter", SORT_MIN, (True, False), (SORTED(TEX_OPS(False, True)),)),
    ("tx_65536_masked", "tex", "t128", "scatter", SORT_MIN, (True, True), (SORTED(TEX_OPS(True, True)),)),
    ("tx_slab", "tex", "t128", "surface", SLAB_MIN, (True, False), PAIR(TEX_OPS(False, True))),
    ("tx_slab_masked", "tex", "t128", "surface", SLAB_MIN, (True, True), (SORTED(TEX_OPS(True, True)),)),
    ("tx_2d", "tex", "t2d", "scatter", 100000, (False, False), (TEXK(False, False),)),          # 2-D branch: never sorted
    ("tx_2d_masked", "tex", "t2d", "scatter", 100000, (False, True), (TEXK(True, False),)),
    ("tx_null", "tex", "null", "scatter", 100000, (True, False), (TEXK(False, False),)),         # no tile: mode 0
    ("tx_t32_long", "tex", "t32", "surface", SLAB_MIN, (True, False), (SORTED(TEX_OPS(False, True)),)),
    # -- Perlin grids (extra: kind, depth, den, nx, ny, z0, z1, octave, misaligned output)
    ("p_noise_nx127", "perlin", "perm", None, 0, ("noise", 0, 128, 127, 9, 0, 3, 4, False), (GENERIC,)),
    ("p_noise_nx128", "perlin", "perm", None, 0, ("noise", 0, 128, 128, 9, 0, 3, 4, False), (RUN(0, 8),)),
    ("p_noise_misaligned", "perlin", "perm", None, 0, ("noise", 0, 200, 256, 9, 1, 4, 3, True), (RUN(0, 8),)),
    ("p_turb_d0", "perlin", "perm", None, 0, ("turb", 0, 512, 512, 8, 0, 2, 0, False), (GENERIC,)),
    ("p_turb_d1", "perlin", "perm", None, 0, ("turb", 1, 512, 512, 8, 0, 2, 0, False), (RUN(1, 8),)),
    ("p_turb_d2", "perlin", "perm", None, 0, ("turb", 2, 512, 512, 8, 0, 2, 0, False), (RUN(1, 8),)),
    ("p_turb_d3", "perlin", "perm", None, 0, ("turb", 3, 512, 512, 8, 0, 2, 0, False), (RUN(1, 16),)),
    ("p_turb_d8", "perlin", "perm", None, 0, ("turb", 8, 512, 600, 11, 3, 6, 0, False), (RUN(1, 16),)),  # largest LDS
    ("p_turb_d9", "perlin", "perm", None, 0, ("turb", 9, 512, 512, 8, 0, 2, 0, False), (GENERIC,)),
    ("p_fractal", "perlin", "perm", None, 0, ("fractal", 0, 256, 256, 9, 2, 4, 0, False), (RUN(2, 16),)),
    # -- single-kernel entry points
    ("e2_points", "e2", "t2d", "scatter", 5000, None, (EV2,)),
    ("proj_points", "proj", "t128", "small", 3000, None, (PROJ_PTS,)),
    ("mb_proj_points", "mbproj", "t128", "small", 2000, (-16.0, -1, 3, [1.0, 0.5, 2.0]), (MB_PROJ,)),
    ("grid2d", "grid2d", "t2d", None, 0, (64, 4), (GRID2D,)),
    ("projected_grid", "pgrid", "t128", None, 0, (48, 3), (PROJ_GRID,)),
]

# Row-slab streams: unmasked lists of >= kSlabMinPoints on t128, for textures and evaluate3D.  (name, stream, n, prefill,
# expected DEFER pattern: a minimum fraction of the full chunks, or "odd" -- exactly the odd chunks).
SLAB_STREAMS = [
    ("row0", ("surface", {"row": 0.0}), SLAB_MIN, None, 0.9),                     # r0 = ry - 1 wraps to 127
    ("row127", ("surface", {"row": 127.0}), SLAB_MIN + 3 * CHUNK + 17, None, 0.9),  # ry + 1 wraps to 0
    ("row_boundary", ("boundary", {"row": 42}), SLAB_MIN, None, 0.9),
    ("planes_all", ("planes", {"lo": 0, "hi": 127}), SLAB_MIN + 100, None, 0.9),
    ("planes_50_60", ("planes", {"lo": 50, "hi": 60}), SLAB_MIN, None, 0.9),      # straddles kSlabThirdPlanes
    ("row_every_visit", ("rows_by_visit", {"period": 1}), 2 * SLAB_MIN, None, 0.9),
    ("row_every_7", ("rows_by_visit", {"period": 7}), 2 * SLAB_MIN, None, 0.9),
    ("interleaved_tail1", "interleaved", SLAB_MIN + 1, None, "odd"),
    ("interleaved_tail4095", "interleaved", SLAB_MIN + CHUNK - 1, None, "odd"),
    ("prefilled_mark", ("surface", {"row": 64.0}), SLAB_MIN + 2 * CHUNK + 5, DEFER_BITS, 0.9),
    ("prefilled_nan", ("surface", {"row": 64.0}), SLAB_MIN, 0x7fc00000, 0.9),
    ("interleaved_nan_in", ("interleaved", {"nan_bits": DEFER_BITS}), SLAB_MIN, None, "odd"),  # marks in kept chunks
]


# ---- the DEFER predicate of plane_sorted_points_kernel<Ops, true> ------------------------------------------------------
def mid_of(c):
    """The coefficient index of a coordinate's middle tap: (int)ceilf(c - 0.5f)."""
    c = np.asarray(c, np.float32)
    with np.errstate(invalid="ignore"):  # (NaN coordinates: their middles are never sampled)
        return np.ceil(c - np.float32(0.5)).astype(np.int64)


def texture_mids(p):
    c = (p.astype(np.float64) * 1.0).astype(np.float32) * np.float32(TEX_CELLS)
    return mid_of(c)


def defer_model(mids, n):
    """Which chunks plane_sorted_points_kernel<Ops, true> leaves to the slab kernel, from the (n, 3) middle indices: whole
    chunks only; wave 0 samples the pairs begin + (lane >> 1) * 128 + (lane & 1); defer when at least 16 of the 32 pairs
    change plane, at most 3 pairs are neighbours in z and x, and one of the first three distinct rows holds >= 48 of 64."""
    full = n // CHUNK
    lane = np.arange(64)
    si = np.arange(full)[:, None] * CHUNK + (lane >> 1) * 128 + (lane & 1)
    kx, ky, kz = mids[si, 0], mids[si, 1], mids[si, 2]
    dz = kz[:, 1::2] - kz[:, 0::2]
    dx = kx[:, 1::2] - kx[:, 0::2]
    changes = (dz != 0).sum(1)
    near = ((np.abs(dz) <= 1) & (np.abs(dx) <= 1)).sum(1)
    top = np.zeros(full, np.int64)
    rest = np.ones_like(ky, bool)
    for _ in range(3):
        has = rest.any(1)
        first = np.argmax(rest, 1)
        r = ky[np.arange(full), first]
        same = (ky == r[:, None]) & has[:, None]
        top = np.maximum(top, same.sum(1))
        rest &= ~same
    defer = (changes >= 16) & (near <= 3) & (top >= 48)
    return np.concatenate([defer, np.zeros(int(n % CHUNK != 0), bool)])


def slab_stream_defers_as_meant(pts_mids, n, want):
    """None when the stream defers what it is meant to, else a message."""
    defer = defer_model(pts_mids, n)
    full = n // CHUNK
    if want == "odd":
        expect = np.arange(defer.size) % 2 == 1
        expect[full:] = False
        bad = np.flatnonzero(defer != expect)
        return None if bad.size == 0 else f"chunks {bad[:10]} differ from the odd pattern"
    frac = float(defer[:full].mean())
    return None if frac >= want else f"defers {frac:.3f} of its chunks, wants >= {want}"


# ---- trace labels ----------------------------------------------------------------------------------------------------
def _mangled_args(s, i):
    """s[i] == 'I': the template arguments up to the matching 'E' -> (list of labels, index after it)."""
    assert s[i] == "I"
    i += 1
    args = []
    while s[i] != "E":
        a, i = _mangled_arg(s, i)
        args.append(a)
    return args, i + 1


def _mangled_arg(s, i):
    if s[i] == "L":  # literal: L <type> <value> E
        t = s[i + 1]
        j = s.index("E", i)
        v = s[i + 2:j].replace("n", "-")
        return ({"0": "false", "1": "true"}[v] if t == "b" else v), j + 1
    if s[i] == "N":  # nested name: components up to 'E'
        i += 1
        last = None
        while s[i] != "E":
            comp, i = _mangled_component(s, i)
            if comp is not None:
                last = comp
        return last, i + 1
    return _mangled_component(s, i)


def _mangled_component(s, i):
    """One source name (with its template arguments) or substitution; None for the anonymous namespace and S_."""
    if s[i] == "S":
        j = s.index("_", i)
        return None, j + 1
    m = re.match(r"\d+", s[i:])
    k = int(m.group())
    i += len(m.group())
    name = s[i:i + k]
    i += k
    if i < len(s) and s[i] == "I":
        args, i = _mangled_args(s, i)
        name = f"{name}<{','.join(args)}>"
    return (None if name.startswith("_GLOBAL__N") else name), i


def kernel_label(name):
    """A traced kernel name, mangled or demangled -> 'plane_sorted_points_kernel<TextureOps<false,true>,true>' (no
    namespaces, no spaces); None for kernels the table does not name."""
    if name.startswith("_Z"):
        s = name[2:]
        if not s.startswith("N"):
            return None
        i = 1
        while i < len(s) and s[i] != "E":
            try:
                comp, i = _mangled_component(s, i)
            except (AttributeError, ValueError, IndexError, KeyError):
                return None
            if comp is not None:
                base = comp.split("<", 1)[0]
                if base in KERNEL_BASES:
                    return comp
        return None
    s = name.replace("(anonymous namespace)::", "")
    for m in re.finditer(r"\b(\w+_kernel)\b", s):
        if m.group(1) not in KERNEL_BASES:
            continue
        j = m.end()
        if j < len(s) and s[j] == "<":
            depth, k = 0, j
            while k < len(s):
                depth += {"<": 1, ">": -1}.get(s[k], 0)
                if depth == 0:
                    break
                k += 1
            return (m.group(1) + s[j:k + 1]).replace(" ", "")
        return m.group(1)
    return None


def test_kernel_label_parses_both_name_forms():
    tex = "_ZN12_GLOBAL__N_126plane_sorted_points_kernelINS_10TextureOpsILb0ELb1EEELb1EEEvT_"
    assert kernel_label(tex) == SORTED(TEX_OPS(False, True), True)
    assert kernel_label("void (anonymous namespace)::plane_sorted_points_kernel<(anonymous namespace)::TextureOps<false, "
                        "true>, true>((anonymous namespace)::TextureOps<false, true>)") == SORTED(TEX_OPS(False, True), True)
    assert kernel_label("_ZN12_GLOBAL__N_122row_slab_points_kernelINS_9Eval3dOpsILb1ELb0EEEEEvT_i") == \
        PAIR(EV_OPS(True, False))[1]
    assert kernel_label("void (anonymous namespace)::row_slab_points_kernel<(anonymous namespace)::Eval3dOps<true, false> >"
                        "((anonymous namespace)::Eval3dOps<true, false>, int)") == PAIR(EV_OPS(True, False))[1]
    assert kernel_label("_ZN12_GLOBAL__N_126plane_sorted_points_kernelINS_9Eval3dOpsILb1ELb1EEELb0EEEvT_") == \
        SORTED(EV_OPS(True, True))
    assert kernel_label("_ZN12_GLOBAL__N_122perlin_grid_run_kernelILi1ELi16EEEvNS_14PerlinGridArgsE") == RUN(1, 16)
    assert kernel_label("void (anonymous namespace)::perlin_grid_run_kernel<2, 16>((anonymous namespace)::PerlinGridArgs)") \
        == RUN(2, 16)
    assert kernel_label("_ZN12_GLOBAL__N_126perlin_grid_generic_kernelENS_14PerlinGridArgsE") == GENERIC
    assert kernel_label("(anonymous namespace)::perlin_grid_generic_kernel((anonymous namespace)::PerlinGridArgs)") == GENERIC
    assert kernel_label("_ZN12_GLOBAL__N_122wavelet_texture_kernelILb1ELb0EEEvNS_7TexArgsE") == TEXK(True, False)
    assert kernel_label("void (anonymous namespace)::eval3d_points_kernel<false>((anonymous namespace)::PointsArgs)") == \
        EV3(False)
    assert kernel_label("_ZN12_GLOBAL__N_120eval2d_points_kernelENS_10PointsArgsE") == EV2
    assert kernel_label("_ZN12_GLOBAL__N_135multiband3d_projected_points_kernelENS_10PointsArgsE.kd") == MB_PROJ
    # tile generation, padding and the dense-grid ladder are not this table's
    assert kernel_label("_ZN12_GLOBAL__N_117padded_copy_kernelEPKfPfi") is None
    assert kernel_label("void (anonymous namespace)::lowpass_lines_kernel((anonymous namespace)::PassArgs)") is None
    assert kernel_label("void (anonymous namespace)::grid3d_sep_kernel<8, 2>((anonymous namespace)::SepArgs)") is None
    assert kernel_label("void at::native::vectorized_elementwise_kernel<4, at::native::FillFunctor<float> >(int)") is None


def test_point_route_table_covers_every_kernel():
    kernels = {k for r in POINT_ROUTES for k in r[6]}
    want = {EV3(False), EV3(True), MB3(True), TEXK(False, False), TEXK(False, True), TEXK(True, False), TEXK(True, True),
            SORTED(EV_OPS(True, False)), SORTED(EV_OPS(True, True)), SORTED(TEX_OPS(False, True)),
            SORTED(TEX_OPS(True, True)), *PAIR(EV_OPS(True, False)), *PAIR(TEX_OPS(False, True)),
            RUN(0, 8), RUN(1, 8), RUN(1, 16), RUN(2, 16), GENERIC, EV2, PROJ_PTS, MB_PROJ, GRID2D, PROJ_GRID}
    assert want <= kernels, want - kernels
    assert all(kernel_label(k) == k for k in kernels)  # the table's labels are what the parser makes of a name
    assert len({r[0] for r in POINT_ROUTES}) == len(POINT_ROUTES)
    assert len({s[0] for s in SLAB_STREAMS}) == len(SLAB_STREAMS)


def test_defer_model_on_hand_made_chunks():
    """The predicate's edges: 16 changes / 15, 3 near pairs / 4, 48 on one row / 47, a partial chunk."""
    n = 5 * CHUNK + 10
    m = np.zeros((n, 3), np.int64)
    lane = np.arange(64)
    pair = np.arange(32)
    for c in range(5):
        si = c * CHUNK + (lane >> 1) * 128 + (lane & 1)
        m[si, 0] = 1000 * pair.repeat(2) + 50 * (lane & 1)      # x: never neighbours
        m[si, 2] = 4 * lane                                      # z: every pair changes plane
        m[si, 1] = 7
    si = 1 * CHUNK + (lane >> 1) * 128 + (lane & 1)
    m[si[1:32:2], 2] = m[si[0:32:2], 2]                          # 16 pairs keep their plane: 16 changes left
    si = 2 * CHUNK + (lane >> 1) * 128 + (lane & 1)
    m[si[1:34:2], 2] = m[si[0:34:2], 2]                          # 17 keep: 15 changes
    si = 3 * CHUNK + (lane >> 1) * 128 + (lane & 1)
    m[si[1:8:2], 2] = m[si[0:8:2], 2] + 1                        # 4 pairs in neighbouring cells ...
    m[si[1:8:2], 0] = m[si[0:8:2], 0] + 1
    m[si[1:8:2][:1], 0] += 5                                     # ... 3 of them neighbours in x too
    si = 4 * CHUNK + (lane >> 1) * 128 + (lane & 1)
    m[si[:17], 1] = np.arange(17) + 20                           # 47 on row 7, but 17 other rows come first
    assert defer_model(m, n).tolist() == [True, True, False, True, False, False]
    m[si[:17], 1] = 20                                           # row 7 is now the second distinct row: 47 < 48
    assert defer_model(m, n)[4] == False  # noqa: E712
    m[si[:16], 1] = 20
    m[si[16], 1] = 7                                             # 48 on row 7
    assert defer_model(m, n)[4] == True  # noqa: E712
    si = 3 * CHUNK + (lane >> 1) * 128 + (lane & 1)
    m[si[1:8:2][:1], 0] -= 5                                     # 4 near pairs: kept
    assert defer_model(m, n)[3] == False  # noqa: E712


@pytest.mark.parametrize("entry", ("tex", "e3"))
@pytest.mark.parametrize("name,spec,n,prefill,want", SLAB_STREAMS, ids=[s[0] for s in SLAB_STREAMS])
def test_slab_streams_defer_the_chunks_they_are_meant_to(entry, name, spec, n, prefill, want):
    """Without this a stream meant for row_slab_points_kernel could test only the plane-ordered kernel."""
    cells = build_stream(spec, n)
    mids = texture_mids(to_texture(cells)) if entry == "tex" else mid_of(cells)
    msg = slab_stream_defers_as_meant(mids, n, want)
    assert msg is None, (name, msg)
    if name == "row_boundary":
        rows = np.unique(mids[:, 1], return_counts=True)
        assert rows[0].tolist() == [42, 43] and 0.1 < rows[1][1] / n < 0.2, rows
    if name == "planes_50_60":
        assert mids[:, 2].min() == 50 and mids[:, 2].max() == 60 and 50 < THIRD_PLANES < 60
    if name.startswith("row_every"):
        # the visits a slab workgroup looks at (after each SLAB_TRUST trusted ones) find another row than the resident
        # one, and trusted visits lie on another row than the one looked at before them
        row_of = mids[:: CHUNK * 256, 1]                         # visit j of workgroup 0 (256 workgroups)
        seen = row_of[:: SLAB_TRUST + 1]
        assert len(seen) >= 2 and (seen[1:] != seen[:-1]).all(), row_of
        assert (row_of[1: SLAB_TRUST + 1] != row_of[0]).any(), row_of
    if name == "planes_all":
        assert np.unique(mids[:, 2]).tolist() == list(range(128))
    if name in ("row0", "row127"):
        assert (mids[:, 1] == (0 if name == "row0" else 127)).all()
    if name == "interleaved_nan_in":
        # NaN inputs with the mark's bits in the kept (even) chunks only, at the marks of the odd waves w < 16
        pts = to_texture(cells) if entry == "tex" else cells
        at = np.flatnonzero(np.isnan(pts).any(1))
        assert at.size == 8 * (n // CHUNK // 2) and (at // CHUNK % 2 == 0).all(), at[:20]
        assert ((at % CHUNK) // 64).tolist() == list(range(1, 16, 2)) * (n // CHUNK // 2), at[:20]
        assert (pts[at].view(np.uint32) == DEFER_BITS).all()


# ---- running a row ---------------------------------------------------------------------------------------------------
class Ctx:
    """Tiles, their coefficients and the Perlin table of the table's rows."""

    def __init__(self, wn):
        import oracle
        self.wn = wn
        self.nm = importlib.import_module("wavelet-noise-in-ray-tracing_amd.noise")
        gold = np.load(os.path.join(HERE, "golden", "ref_vectors.npz"))
        self.obj, self.coef = {}, {}
        for name, n, seed, dims in (("t128", 128, 12345, 3), ("t32", 32, SEED32, 3), ("t2d", 128, 12345, 2)):
            o = wn.WaveletNoise(n, seed)
            o.generateNoiseTile3D() if dims == 3 else o.generateNoiseTile2D()
            self.obj[name], self.coef[name] = o, o.getNoiseCoefficients()
        for name, key in (("t8", "tile3d_8_7"), ("t16", "tile3d_16_12345"), ("t6", "tile3d_5odd_11")):
            self.coef[name] = gold[key]
            self.obj[name] = wn.WaveletNoise.from_coefficients(gold[key], 3)
        self.obj["empty"], self.coef["empty"] = wn.WaveletNoise(128, 0), np.empty(0, np.float32)
        self.obj["null"], self.coef["null"] = None, None
        self.perlin = wn.perlin(12345)
        self.perm = oracle.perlin_perm(12345)
        self.cus = wn.device_info()["compute_units"]

    def handle(self, tile, dims):
        o = self.obj[tile]
        return None if o is None else o._handle(dims)


def row_inputs(ctx, row):
    """The row's points (as the entry point takes them) and active mask, both host arrays."""
    name, entry, tile, spec, n, extra = row[:6]
    if spec is None:
        return None, None
    cells = build_stream(spec, n, ctx.cus if ctx else 256)
    pts = to_texture(cells) if entry == "tex" else cells
    if entry == "e2":
        pts = np.ascontiguousarray(pts[:, :2])
    active = None
    if entry == "tex" and extra[1]:
        r = np.random.default_rng(n)
        active = (r.uniform(size=n) < 0.6).astype(np.uint8)
        active[: 3 * CHUNK] = 1          # whole chunks on and off too: the compaction's full and empty batches
        active[3 * CHUNK: 5 * CHUNK] = 0
    return pts, active


def _normals(n):
    r = np.random.default_rng(n + 99)
    v = r.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _lattice(i, den):
    return (np.float32(i) / np.float32(den)) * np.float32(4.0)


def run_row(ctx, row, pts, active, prefill=SENTINEL_BITS):
    """One call of the table on the current stream; returns the device output (a flat float32 tensor)."""
    import ctypes as C
    import torch
    nm = ctx.nm
    name, entry, tile, spec, n, extra = row[:6]

    def filled(count):
        out = torch.empty(count, dtype=torch.float32, device="cuda")
        out.view(torch.int32).fill_(int(np.uint32(prefill).view(np.int32)))
        return out

    if entry == "perlin":
        kind, depth, den, nx, ny, z0, z1, octave, misaligned = extra
        g = nm.GridSpec(den, nx, ny, z0, z1, octave_scale=nm._octave_scale(octave))
        total = (z1 - z0) * ny * nx
        buf = filled(total + 1)
        out = buf[1:] if misaligned else buf[:total]
        gc, ptr = g.c(), nm._ptr(out)
        if kind == "noise":
            nm.check(nm._lib.wn_perlin_grid(ctx.perlin._h, C.byref(gc), ptr, nm._stream()))
        elif kind == "turb":
            nm.check(nm._lib.wn_perlin_turb_grid(ctx.perlin._h, C.byref(gc), int(depth), ptr, nm._stream()))
        else:
            nm.check(nm._lib.wn_perlin_fractal_grid(ctx.perlin._h, C.byref(gc), ptr, nm._stream()))
        return out
    if entry == "grid2d":
        image, octave = extra
        return ctx.nm.generate2DOctaveBandNoise(image, octave, None, ctx.obj[tile]).reshape(-1)
    if entry == "pgrid":
        image, octave = extra
        return ctx.nm.generate3DProjectedOctaveBandNoise(image, octave, None, ctx.obj[tile]).reshape(-1)
    d_pts = torch.from_numpy(pts).cuda()
    out = filled(n)
    st = nm._stream()
    if entry == "e3":
        nm.check(nm._lib.wn_eval3d_points(ctx.handle(tile, 3), nm._ptr(d_pts), n, nm._ptr(out), st))
    elif entry == "e2":
        nm.check(nm._lib.wn_eval2d_points(ctx.handle(tile, 2), nm._ptr(d_pts), n, nm._ptr(out), st))
    elif entry == "mb":
        s, first, nb, w = extra
        wa = (C.c_float * nb)(*w)
        nm.check(nm._lib.wn_multiband3d_points(ctx.handle(tile, 3), nm._ptr(d_pts), n, float(s), int(first), int(nb), wa,
                                               0.18402, nm._ptr(out), st))
    elif entry == "proj":
        d_nr = torch.from_numpy(_normals(n)).cuda()
        nm.check(nm._lib.wn_eval3d_projected_points(ctx.handle(tile, 3), nm._ptr(d_pts), nm._ptr(d_nr), n, nm._ptr(out), st))
    elif entry == "mbproj":
        s, first, nb, w = extra
        wa = (C.c_float * nb)(*w)
        d_nr = torch.from_numpy(_normals(n)).cuda()
        nm.check(nm._lib.wn_multiband3d_projected_points(ctx.handle(tile, 3), nm._ptr(d_pts), nm._ptr(d_nr), 0, n,
                                                         float(s), int(first), int(nb), wa, 0.296, nm._ptr(out), st))
    else:
        assert entry == "tex", entry
        use_3d = extra[0]
        d_act = torch.from_numpy(active).cuda() if active is not None else None
        h = ctx.handle(tile, 3 if use_3d else 2) if tile != "null" else None
        nm.check(nm._lib.wn_wavelet_texture_points(h, int(use_3d), 1.0, 4, nm._ptr(d_pts), nm._ptr(d_act), n,
                                                   nm._ptr(out), st))
    return out


def row_reference(ctx, row, pts, active, prefill=SENTINEL_BITS):
    """The oracle's answer for every element of the row's output (inactive elements: the prefill pattern)."""
    import oracle as ora
    name, entry, tile, spec, n, extra = row[:6]
    coef = ctx.coef[tile] if tile != "perm" else None
    if entry == "perlin":
        kind, depth, den, nx, ny, z0, z1, octave, _ = extra
        if kind == "noise":
            return ora.grid_perlin_volume(ctx.perm, den, nx, ny, z0, z1, octave).ravel()
        if kind == "turb":
            return ora.grid_turb_volume(ctx.perm, den, nx, ny, z0, z1, depth).ravel()
        z, y, x = np.meshgrid(_lattice(np.arange(z0, z1), den), _lattice(np.arange(ny), den),
                              _lattice(np.arange(nx), den), indexing="ij")
        p = np.stack([x.ravel(), y.ravel(), z.ravel()], 1)
        return ora.perlin_fractal(ctx.perm, p).astype(np.float32)
    if entry == "grid2d":
        image, octave = extra
        out = np.empty(image * image, np.float32)
        ora.lib().wno_grid_wavelet2d(coef, coef.size, image, octave, out)
        return out
    if entry == "pgrid":
        image, octave = extra
        out = np.empty(image * image, np.float32)
        ora.lib().wno_grid_wavelet3d_projected(coef, coef.size, image, octave, out)
        return out
    if entry == "e3":
        return ora.evaluate3d(coef, pts)
    if entry == "e2":
        return ora.evaluate2d(coef, pts)
    if entry == "mb":
        s, first, nb, w = extra
        return ora.multiband3d(coef, pts, s, first, nb, w, 0.18402)
    if entry == "proj":
        return ora.evaluate3d_projected(coef, pts, _normals(n))
    if entry == "mbproj":
        s, first, nb, w = extra
        return ora.multiband3d_projected(coef, pts, _normals(n), s, first, nb, w, 0.296)
    use_3d = extra[0]
    want = ora.wavelet_texture_value(coef, use_3d, 1.0, 4, pts)
    if active is not None:
        want = np.where(active != 0, want, np.uint32(prefill).view(np.float32))
    return want


def _child():
    import torch
    assert torch.cuda.is_available()
    wn = importlib.import_module("wavelet-noise-in-ray-tracing_amd")
    ctx = Ctx(wn)
    torch.cuda.synchronize()
    for row in POINT_ROUTES:
        pts, active = row_inputs(ctx, row)
        run_row(ctx, row, pts, active)
        torch.cuda.synchronize()
    print(f"point dispatch child: {len(POINT_ROUTES)} calls")


# ---- GPU -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU (the product has no CPU path)"
    return Ctx(importlib.import_module("wavelet-noise-in-ray-tracing_amd"))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _first_differences(got, want, k=5, nan_at=None):
    """Elements whose bits differ; where `nan_at` is set, elements that are not NaN in both (NaN payloads may differ
    between the CPU and the GPU)."""
    differ = _bits(got) != _bits(want)
    if nan_at is not None:
        differ[nan_at] = ~(np.isnan(got[nan_at]) & np.isnan(want[nan_at]))
    bad = np.flatnonzero(differ)
    return bad.size, [(int(i), float(got[i]), float(want[i])) for i in bad[:k]]


@pytest.mark.gpu
def test_point_routes_reach_the_kernels_they_name(tmp_path):
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    assert os.path.exists(prof), "rocprofv3 is needed to observe which kernel ran"
    out_dir = tmp_path / "trace"
    cmd = ["timeout", "-k", "10", "600", prof, "--kernel-trace", "--output-format", "csv", "-d", str(out_dir),
           "--", sys.executable, os.path.abspath(__file__), "--child"]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
    assert res.returncode == 0, f"exit {res.returncode}\n{res.stdout[-3000:]}\n{res.stderr[-3000:]}"
    files = glob.glob(str(out_dir / "**" / "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, (files, res.stdout[-2000:])
    with open(files[0], newline="") as f:
        rows = list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    got = [lab for lab in (kernel_label(r["Kernel_Name"]) for r in rows) if lab is not None]
    want = [k for r in POINT_ROUTES for k in r[6]]
    wrong, pos = [], 0
    for r in POINT_ROUTES:
        ran = tuple(got[pos:pos + len(r[6])])
        if ran != tuple(r[6]):
            wrong.append((r[0], r[6], ran))
        pos += len(r[6])
    assert len(got) == len(want) and not wrong, \
        f"{len(got)} kernels traced, {len(want)} expected; calls served otherwise (case, expected, ran): {wrong!r}"


@pytest.mark.gpu
@pytest.mark.parametrize("row", POINT_ROUTES, ids=[r[0] for r in POINT_ROUTES])
def test_point_route_values(ctx, row):
    """Every element of the row's output, bit for bit, against the oracle (masked rows: inactive elements keep the
    prefilled pattern)."""
    import torch
    pts, active = row_inputs(ctx, row)
    got = run_row(ctx, row, pts, active)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    want = row_reference(ctx, row, pts, active)
    assert got.shape == want.shape, (row[0], got.shape, want.shape)
    count, first = _first_differences(got, want)
    assert count == 0, f"{row[0]} ({row[6]}): {count} elements differ from the oracle, first (index, got, want): {first}"


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ("tex", "e3"))
@pytest.mark.parametrize("name,spec,n,prefill,want", SLAB_STREAMS, ids=[s[0] for s in SLAB_STREAMS])
def test_row_slab_streams(ctx, entry, name, spec, n, prefill, want):
    """Unmasked streams on t128 through the pair plane_sorted_points_kernel<Ops, true> + row_slab_points_kernel<Ops>,
    every point against the oracle, from an output that holds `prefill` (by default a NaN no kernel writes); points with a
    NaN coordinate must give a NaN, every other point the oracle's bits."""
    import torch
    row = (name, entry, "t128", spec, n, (True, False) if entry == "tex" else None)
    pts, _ = row_inputs(ctx, row)
    got = run_row(ctx, row, pts, None, SENTINEL_BITS if prefill is None else prefill)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    want = row_reference(ctx, row, pts, None)
    count, first = _first_differences(got, want, nan_at=np.isnan(pts).any(1))
    assert count == 0, f"{entry} {name}: {count} of {n} points differ from the oracle, first (index, got, want): {first}"


if __name__ == "__main__" and "--child" in sys.argv:
    _child()
