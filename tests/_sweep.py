"""Seeded case generators for tests/test_gpu_lattice_sweep.py, and the planner restatements tests/_far_plan.py lacks.

Every generator draws STRATIFIED: the target (kernel label, declining check, shape classes) is chosen first, then the
parameters are drawn from menus that land on it, and the drawn case is classified with the restated planner
(_far_plan.deriv_route, perlin_run_eligible, mb2d_trip).  A case that misses its target is drawn again from the same stream;
a target the generator cannot place raises (a generator bug, never a skip).  No GPU is involved: the CPU tests of that module
assert what the committed seeds reach.

  deriv_cases(family, seed)   gradient / curl bricks: grad3d_ / curl3d_grid_sep_kernel<1..8>, _direct_kernel<true / false>
  perlin_cases(variant, seed) Perlin value / gradient / curl grids: run form and generic kernel
  mb2d_cases(cus, seed)       multiband2d_grid_kernel: the span walk over trips of 2 * cus * 1024 samples
  bricks_cases(seed)          wavelet brick lists: every sep<NB> and every declining check
  perlin_bricks_cases(variant, seed)  Perlin brick lists: perlin_cases' slots on drawn volumes and lists (segment trips 1..8)

A plain helper module (not a conftest): the tests import it by name.
"""
import math
import os
import re
from types import SimpleNamespace

import numpy as np

import _far_plan as fp

f32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "wavelet-noise-in-ray-tracing_amd", "csrc")

CAP = 1_250_000                       # samples per lattice, every family
SEEDS = (20251, 20252)                # the committed seeds of the gradient / curl sweep
PARTS = 3                             # a seed's cases run as this many GPU tests
INV = float(f32(1.0) / np.sqrt(f32(0.18402)))
BRICK = (256, 8, 8)                   # kGX, kGY, kGZ (csrc/wn_brick.hpp)
TILE_N = {"t128": 128, "t32": 32, "t8": 8, "t6": 6, "empty": 0}
BRICK_TILES = ("t128", "t32", "t8", "t6")


def _pow2(n):
    return n > 0 and n & (n - 1) == 0


# ---- gradient and curl bricks ----------------------------------------------------------------------------------------------
def deriv_grid(c):
    return fp.Grid(c.den, c.nx, c.ny, c.z0, c.nz, c.base_range, c.octave_scale, c.post_scale, c.z_const)


def deriv_route(c):
    """(kernel label, the brick planner's declining check or None) of the default tier."""
    label, why = fp.deriv_route(deriv_grid(c), TILE_N[c.tile], False, c.family, None if c.bands is None else c.bands[:3])
    return label, why.get("brick")


def deriv_active(c):
    return 1 if c.bands is None else fp.active_bands(*c.bands[:3])


def top_step(c):
    """The step of the finest active band, in cells per sample."""
    q = 1.0 if c.bands is None else 2.0 * 2.0 ** (c.bands[1] + deriv_active(c) - 1)
    return fp.lattice_step(deriv_grid(c), float(f32(c.octave_scale) * f32(q)), True, False, 0.0).step


def near_third(c):
    """'below': the top band's step within 2 % below 1/3; 'at_above': at 1/3 or within 2 % above it; else None."""
    r = top_step(c) * 3.0
    return "below" if 0.98 <= r < 1.0 else ("at_above" if 1.0 <= r <= 1.02 else None)


def deriv_classes(c):
    """The shape classes of the issue a case belongs to."""
    k = set()
    bx, by, bz = BRICK
    if c.nx % 4:
        k.add("nx%4")
    if c.nx > bx and c.nx % bx:
        k.add("ragged_x")
    if c.ny > by and c.ny % by:
        k.add("ragged_y")
    if c.z_const is None:
        if c.nz > bz and c.nz % bz:
            k.add("ragged_z")
        if c.z0 < 0:
            k.add("z0<0")
    else:
        k.add("z_const")
    if {"ragged_x", "ragged_y", "ragged_z"} <= k:
        k.add("ragged_xyz")
    if not _pow2(c.den):
        k.add("den_np2")
    if c.out_scale < 0:
        k.add("neg_out")
    k.add(f"lead{c.lead}")
    k.add(f"tile_{c.tile}")
    if c.bands is not None:
        s, first, nbands, w = c.bands
        if deriv_active(c) < nbands:
            k.add("s_cut")
        k.add("first_neg" if first < 0 else ("first_pos" if first > 0 else "first_0"))
        if any(x == 0.0 for x in w):
            k.add("zero_w")
    if c.family == "curl":
        if c.offsets is None:
            k.add("off_default")
        else:
            flat = [v for o in c.offsets for v in o]
            if min(flat) < 0:
                k.add("off_neg")
            if max(flat) >= max(TILE_N[c.tile], 1):
                k.add("off_ge_n")
    return k


_MODS = ["nx%4", "ragged_x", "ragged_y", "ragged_z", "z0<0", "z_const", "den_np2", "neg_out", "s_cut", "first_neg", "first_pos",
         "zero_w", "ragged_xyz"]
# den at a top-band numerator of 128 (base_range 4 * 2^4 * post 2): steps .3325 .. .0625
_DEN128 = [385, 400, 512, 512, 640, 777, 1000, 1024, 2048]
_DEN128_NP2 = [385, 400, 640, 777, 1000]


def _effective(mods, nb):
    """The classes a case of nb bands is forced into: `mods` with its contradictions resolved."""
    mods = set(mods)
    if "z_const" in mods:
        mods -= {"ragged_z", "z0<0", "ragged_xyz"}
    if "ragged_xyz" in mods:
        mods |= {"ragged_x", "ragged_y", "ragged_z"}
    if "first_neg" in mods:
        mods -= {"first_pos"}
    if "zero_w" in mods and nb == 1:
        mods |= {"s_cut"}             # a second band, cut by s: the weights are not all zero
    if nb == 8:
        mods -= {"s_cut"}
    return mods


_MULTI_MODS = {"s_cut", "first_neg", "first_pos", "zero_w"}


def _draw_deriv(rng, family, idx, target, near, mods, single=None):
    """One draw at `target`: ("sep", nb), "two_mids" or "static".  single: True for wn_eval3d_*_grid, False for the
    multiband entry point, None for either."""
    nb = target[1] if isinstance(target, tuple) else (1 if single else int(rng.integers(1, 9)))
    mods = _effective(mods, nb)
    if single:
        assert nb == 1 and not mods & _MULTI_MODS
        multi = False
    else:
        multi = single is False or nb > 1 or bool(mods & _MULTI_MODS) or bool(rng.integers(0, 2))
    c = SimpleNamespace(family=family, lead=idx % 4, offsets=None)
    c.tile = "empty" if target == "static" else BRICK_TILES[(idx // 4 + idx) % 4]
    # the top band's numerator: step = num / den
    if multi:
        nbands = nb
        if "s_cut" in mods and nb < 8:
            nbands = nb + int(rng.integers(1, 9 - nb))
        lo, hi = -3, 2
        if "first_neg" in mods:
            hi = -1
        if "first_pos" in mods:
            lo = 1
        first = int(rng.integers(lo, hi + 1))
        s = -16.0 if nbands == nb else -(first + nb) + 0.5
        w = [float(f32(x)) for x in rng.uniform(0.25, 2.0, nbands)]
        if "zero_w" in mods:
            w[int(rng.integers(0, nbands))] = 0.0
            assert nbands >= 2
        c.bands = (s, first, nbands, w)
        c.base_range, c.octave_scale, c.post_scale = 4.0, 1.0, 1.0
        shift = first + nb - 1 - 4          # numerator 8 * 2^(first + nb - 1) = 128 * 2^shift
    else:
        c.bands = None
        c.base_range, c.post_scale = 4.0, 2.0
        octave = int(rng.integers(2, 6))
        c.octave_scale = float(2.0 ** octave)
        shift = octave - 4
    if near == "below":
        den128 = 385
    elif near == "at_above":
        den128 = 384 if single is not None else int(rng.choice([384, 380, 378]))
    elif target == "two_mids":
        den128 = int(rng.choice([64, 200, 300, 350]))
    else:
        den128 = int(rng.choice(_DEN128_NP2 if "den_np2" in mods else _DEN128))
    if shift >= 0:
        c.den = den128 << shift
    else:
        # a divisor that keeps the step exactly when it divides, else the next larger one (a smaller step)
        c.den = max(2, -(-den128 // (1 << -shift)))
        if near is not None or target == "two_mids":
            # keep the step exact: scale the lattice's base_range instead (a power of two: exact in float32)
            c.den, c.base_range = den128, c.base_range * 2.0 ** -shift
    if "ragged_x" in mods:
        c.nx = int(rng.choice([301, 515, 701] if "nx%4" in mods else [300, 515, 700]))
    else:
        c.nx = int(rng.choice([5, 67, 301, 515, 999] if "nx%4" in mods else [5, 64, 100, 256, 260, 300, 512, 515, 700, 998]))
    c.ny = int(rng.choice([9, 13, 20] if "ragged_y" in mods else [1, 3, 5, 8, 9, 13, 16, 27]))
    if "z_const" in mods:
        c.z_const, c.z0, c.nz = float(rng.choice([2.0, 0.37, -1.25])), 0, 1
    else:
        c.z_const = None
        c.nz = int(rng.choice([9, 13, 20] if "ragged_z" in mods else [1, 2, 5, 8, 9, 13, 16, 27]))
        c.z0 = int(rng.choice([-9, -4, -20] if "z0<0" in mods else [0, 0, 3, 100, -5]))
    c.out_scale = float(rng.choice([-1.5, -INV] if "neg_out" in mods else [INV, 1.0, 0.75, -1.5]))
    if family == "curl" and idx % 6 != 5:
        c.offsets = tuple(tuple(int(v) for v in rng.integers(-300, 400, 3)) for _ in range(3))
    return c


def _deriv_slots(seed):
    """(target, near, mods, single) for the cases of a seed: every sep<NB> twice, three two_mids declines, two empty tiles
    and nine more brick cases.  The shape classes rotate over the brick cases, two per case.  The steps next to 1/3: 128 / 385
    once through each kind of entry point, 128 / 384 likewise, and one more just above."""
    slots = [[("sep", nb), None, None] for nb in range(1, 9)] * 2
    slots = [list(x) for x in slots]
    slots[0][1:] = ["below", True]
    slots[9 + seed % 5][1:] = ["below", False]
    slots += [["two_mids", "at_above", True], ["two_mids", "at_above", False], ["two_mids", "at_above" if seed % 2 else None, None],
              ["static", None, None], ["static", None, None]]
    slots += [[("sep", 1 + (seed + 3 * i) % 8), None, None] for i in range(9)]
    out, b = [], 0
    for target, near, single in slots:
        mods = ()
        if isinstance(target, tuple):
            mods = (_MODS[(b + seed) % len(_MODS)], _MODS[(5 * b + 3 + seed) % len(_MODS)])
            if single:
                mods = tuple(m for m in mods if m not in _MULTI_MODS)
            b += 1
        out.append((target, near, mods, single))
    return out


def deriv_cases(family, seed):
    """The cases of (family, seed), each with .name, .label (the kernel the model sends it to) and .why."""
    assert family in ("grad", "curl")
    rng = np.random.default_rng([seed, 0 if family == "grad" else 1])
    cases = []
    for idx, (target, near, mods, single) in enumerate(_deriv_slots(seed)):
        for _attempt in range(400):
            c = _draw_deriv(rng, family, idx, target, near, mods, single)
            label, why = deriv_route(c)
            if isinstance(target, tuple):
                hit = why is None and label == f"{family}3d_grid_sep_kernel<{target[1]}>"
                hit = hit and _effective(mods, target[1]) <= deriv_classes(c)
            else:
                hit = why == target
            if hit and (near is None or near_third(c) == near):
                break
        else:
            raise AssertionError(f"the generator cannot place {family} seed {seed} case {idx}: {target} {near} {mods}")
        assert c.nx * c.ny * c.nz <= CAP, (c.nx, c.ny, c.nz)
        c.label, c.why = label, why
        c.name = f"{family}-{seed}-{idx:02d}"
        cases.append(c)
    return cases


def describe(c):
    return {k: v for k, v in vars(c).items()}


# ---- the brick planner's LDS cap ---------------------------------------------------------------------------------------------
def brick_box_bound(boxes):
    """An upper bound on brick_plan's box floats over every lattice that passes two_mids, for 8 bands.

    two_mids: 3 step + slack <= 1 with slack > 0 (pmax >= 1), so in the top band 255 step + slack < 85 and
    7 step + slack < 7/3 + 1: extent(256) + 1 = floor(255 step + slack) + 5 <= 89 <= 90 and extent(8) = floor(7 step +
    slack) + 4 <= 6 (WN_Z_CONST: ez = 3).  Band k below the top has step / 2^k and a slack no larger than the top band's
    (its pmax is smaller), itself <= 1: extent(256) + 1 <= floor(85 / 2^k + 1) + 5, extent(8) <= floor(7 / (3 * 2^k) + 1) + 4."""
    total = 0
    for k in range(fp.MAX_BANDS):
        ex = 90 if k == 0 else int(math.floor(85.0 / 2 ** k + 1.0)) + 5
        e8 = 6 if k == 0 else int(math.floor(7.0 / (3.0 * 2 ** k) + 1.0)) + 4
        total += boxes * ex * e8 * e8
    return total


def brick_box_floats(g, qmuls, boxes):
    """brick_plan's box_total of a lattice (the sum its `lds` check compares with the cap)."""
    total = 0
    for q in qmuls:
        ls = fp.lattice_step(g, float(f32(g.octave_scale) * f32(q)), True, False, 0.0)
        total += boxes * (ls.extent(256) + 1) * ls.extent(8) * (3 if g.z_const_mode else ls.extent(8))
    return total


def csrc(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def int_product(expr):
    out = 1
    for fct in expr.strip().strip("()").split("*"):
        assert re.fullmatch(r"\s*\d+u?\s*", fct), expr
        out *= int(fct.strip().rstrip("u"))
    return out


def constexpr_int(name, text):
    found = re.findall(r"constexpr\s+(?:size_t|int)\s+" + name + r"\s*=\s*([^;]+);", text)
    assert len(found) == 1, (name, found)
    return int_product(found[0])


# ---- Perlin run form ---------------------------------------------------------------------------------------------------------
RUN_MIN_NX = 128      # perlin_run_eligible: g.nx >= 128
RUN_MAX_DEPTH = 8     # kRunMaxDepth
FRACTAL_OCTAVES = 6   # kFractalOctaves
PERLIN_SEED = 20253
PERLIN_CHANNELS = {"value": 1, "grad": 4, "curl": 3}


def perlin_octaves(kind, depth):
    return 1 if kind == "noise" else (FRACTAL_OCTAVES if kind == "fractal" else depth)


def perlin_run_eligible(nx, ny, nz, octaves):
    """csrc/wn_perlin_frame.hpp: rows of >= 128 samples at 1..kRunMaxDepth octaves (and a launch grid within 65535 blocks
    of 8 rows and of 8 planes)."""
    return nx >= RUN_MIN_NX and 1 <= octaves <= RUN_MAX_DEPTH and (ny + 7) // 8 <= 65535 and (nz + 7) // 8 <= 65535


def perlin_step(c):
    return abs(float(f32(c.base_range)) * float(f32(c.octave_scale)) * float(f32(c.post_scale)) / c.den)


def perlin_step_class(c):
    s = perlin_step(c)
    return "small" if s < 0.125 else ("mid" if s < 1.0 else ("big" if s > 1.0 else "one"))


def perlin_form(c):
    return "run" if perlin_run_eligible(c.nx, c.ny, c.nz, perlin_octaves(c.kind, c.depth)) else "generic"


# (kind, depth, row lengths, step class, flags): flags n = negative base_range, z = WN_Z_CONST, d = non-dyadic octave_scale
_PERLIN_SLOTS = [
    ("noise", 0, (128,), "small", ""), ("turb", 1, (300, 515), "small", "d"), ("fractal", 0, (129, 512), "small", "n"),
    ("turb", 8, (256, 700), "small", "z"),
    ("noise", 0, (129,), "mid", "d"), ("turb", 5, (128, 300), "mid", "n"), ("fractal", 0, (300, 515), "mid", "d"),
    ("turb", 8, (515,), "mid", "d"), ("noise", 0, (700, 512), "mid", "z"),
    ("noise", 0, (300, 512), "big", ""), ("turb", 3, (128, 131), "big", "d"), ("fractal", 0, (260,), "big", "n"),
    ("turb", 1, (129,), "big", "z"),
    # the generic kernel: rows below 128 samples, and 0, 9 or 12 octaves
    ("noise", 0, (127,), "mid", ""), ("turb", 7, (127, 100), "small", "d"), ("fractal", 0, (64, 50), "mid", "n"),
    ("turb", 0, (256, 300), "small", ""), ("turb", 9, (128, 515), "small", "d"), ("turb", 12, (300,), "mid", "z"),
    ("noise", 0, (5, 67), "big", "d"),
]
_STEP_RANGE = {"small": (0.004, 0.11), "mid": (0.15, 0.9), "big": (1.2, 5.0)}


def perlin_cases(variant, seed=PERLIN_SEED):
    assert variant in PERLIN_CHANNELS
    rng = np.random.default_rng([seed, list(PERLIN_CHANNELS).index(variant)])
    cases = []
    for idx, (kind, depth, rows, cls, flags) in enumerate(_PERLIN_SLOTS):
        for _attempt in range(400):
            c = SimpleNamespace(variant=variant, kind=kind, depth=depth, lead=idx % 4, post_scale=1.0, offsets=None)
            c.nx = int(rng.choice(rows))
            c.ny = int(rng.choice([3, 8, 9, 17]))
            c.base_range = float(rng.choice([-4.0, -3.0])) if "n" in flags else float(rng.choice([4.0, 4.0, 2.5]))
            c.octave_scale = float(f32(rng.choice([3.7, 0.6, 5.3]))) if "d" in flags else float(rng.choice([1.0, 2.0, 4.0, 16.0]))
            target = float(rng.uniform(*_STEP_RANGE[cls]))
            c.den = max(2, int(round(abs(c.base_range) * c.octave_scale / target)))
            if "z" in flags:
                c.z_const, c.z0, c.nz = float(rng.choice([0.37, 16.0, -2.75])), 0, 1
            else:
                c.z_const, c.z0, c.nz = None, int(rng.choice([0, 3, -5])), int(rng.choice([1, 3, 9, 10]))
            c.out_scale = float(rng.choice([1.0, 0.75, -2.5]))
            if variant == "curl" and idx % 5 != 4:
                c.offsets = tuple(tuple(int(v) for v in rng.integers(-300, 1100, 3)) for _ in range(3))
            if perlin_step_class(c) == cls:
                break
        else:
            raise AssertionError(f"the generator cannot place perlin {variant} case {idx}")
        assert c.nx * c.ny * c.nz <= CAP
        c.form = perlin_form(c)
        c.name = f"perlin-{variant}-{idx:02d}-{kind}{depth}"
        cases.append(c)
    return cases


# ---- multiband2d grids -------------------------------------------------------------------------------------------------------
MB2D_WORKGROUP = 1024          # WN_MB2D_WORKGROUP
MB2D_WORKGROUPS_PER_CU = 2     # kWorkgroupsPerCu
MB2D_LDS_TILE_MAX_BYTES = 80 * 1024
MB2D_LDS_MIN_POINTS = 16 * 4096
MB2D_SEED = 20254
MB2D_NX = (1, 3, 67, 1023, 1024, 1025, 1500, 4099)
MB2D_TILES = ("t128", "t6", "t16", "t256")
MB2D_FULL = 300_000            # lattices up to this many samples are compared in full


def mb2d_trip(cus):
    return MB2D_WORKGROUPS_PER_CU * cus * MB2D_WORKGROUP


def mb2d_form(tile):
    n = int(tile[1:])
    return "lds" if n * (n + 2) * 4 <= MB2D_LDS_TILE_MAX_BYTES else "gather"


def mb2d_trips(c, cus):
    """(whole trips, samples of the last partial one)."""
    return divmod(c.nx * c.ny, mb2d_trip(cus))


def mb2d_trip_class(c, cus):
    """'one': less than a trip; 'boundary': exactly one; 'multi': more than two and at most three; else 'other'."""
    total, trip = c.nx * c.ny, mb2d_trip(cus)
    if total <= trip:
        return "one" if total < trip else "boundary"
    return "multi" if 2 * trip < total <= 3 * trip else "other"


def mb2d_cases(cus, seed=MB2D_SEED):
    """Every row length at one trip and at 2-3 trips, and the two lattices that end exactly on the trip boundary."""
    rng = np.random.default_rng([seed, cus])
    trip = mb2d_trip(cus)
    plan = [(nx, cls) for nx in MB2D_NX for cls in ("one", "multi")] + [(1024, "boundary"), (1, "boundary")]
    cases = []
    for idx, (nx, cls) in enumerate(plan):
        c = SimpleNamespace(nx=nx, lead=idx % 4, grad=bool((idx + idx // 2) % 2), tile=MB2D_TILES[(idx + idx // 4) % 4])
        if cls == "one":
            # compared in full: at most MB2D_FULL samples, and never past the trip
            c.ny = max(1, min(int(rng.integers(30, 80)) if nx > 100 else int(rng.integers(200, 3000)), min(MB2D_FULL, trip - 1) // nx))
        elif cls == "boundary":
            assert trip % nx == 0
            c.ny = trip // nx
        else:
            c.ny = min(CAP // nx, -(-int(2.3 * trip) // nx))
        c.nbands = 1 + idx % 8
        c.first = int(rng.integers(-2, 3))
        c.s = float(-(c.first + max(1, c.nbands - 1)) + 0.5) if idx % 3 == 0 and c.nbands > 1 else -16.0
        c.w = [float(f32(x)) for x in rng.uniform(0.25, 2.0, c.nbands)]
        c.den = int(rng.choice([4099, 256, 1000, 4096]))
        while 4.0 * max(c.nx, c.ny) / c.den * 2.0 ** (c.first + c.nbands + 1) >= 2.0 ** 23:
            c.den *= 3                # the finest band's coordinate keeps a fraction in float32
        c.out_scale = float(rng.choice([1.0, 0.75, -1.5]))
        total = c.nx * c.ny
        assert total <= CAP, (cus, nx, c.ny)
        if mb2d_trip_class(c, cus) != cls:
            raise AssertionError(f"the generator cannot place multiband2d case {idx} ({nx}, {cls}) at {cus} CUs: {c.ny} rows")
        c.cls, c.form = cls, mb2d_form(c.tile)
        c.name = f"mb2d-{idx:02d}-nx{nx}-{cls}-{'grad' if c.grad else 'value'}-{c.tile}"
        cases.append(c)
    return cases


def mb2d_check_indices(c, cus, seed=MB2D_SEED):
    """The samples compared with the point entry: all of them up to MB2D_FULL, else the 2,048 on either side of every trip
    boundary, the last 2,048 and 8,192 random ones (sorted, unique)."""
    total, trip = c.nx * c.ny, mb2d_trip(cus)
    if total <= MB2D_FULL:
        return np.arange(total)
    parts = [np.arange(max(0, b - 2048), min(total, b + 2048)) for b in range(trip, total, trip)]
    parts.append(np.arange(total - 2048, total))
    parts.append(np.random.default_rng([seed, total]).integers(0, total, 8192))
    return np.unique(np.concatenate(parts))


# ---- brick lists ---------------------------------------------------------------------------------------------------------------
BRICKS_SEEDS = (20255, 20256)
BRICKS_PER_SEED = 30
BRICKS_MAX_LIST = 40
BRICKS_DECLINES = ("flag", "two_mids", "gate", "negative step", "no active band", "empty tile")
_ND = (1.1547005, 0.8862269, 1.0954451, 0.9189385, 1.2533141, 0.8408964)   # full-mantissa factors next to 1


def bricks_grid(c):
    return fp.Grid(c.den, c.nx, c.ny, c.z0, c.z1 - c.z0, c.base_range, c.octave_scale, c.post_scale)


def bricks_route(c):
    return fp.bricks_route(bricks_grid(c), TILE_N[c.tile], c.exact, None if c.bands is None else c.bands[:3])


def bricks_top_step(c):
    """The signed step of the finest active band (None where no band is active)."""
    os_ = fp.bricks_band_scales(bricks_grid(c), None if c.bands is None else c.bands[:3])
    return c.base_range * float(f32(os_[-1])) * c.post_scale / c.den if os_ else None


def bricks_near_third(c):
    st = bricks_top_step(c)
    if st is None:
        return None
    r = 3.0 * st
    return "below" if 0.98 <= r < 1.0 else ("at_above" if 1.0 <= r <= 1.02 else None)


def bricks_in_range(c):
    nbx, nby, bz0, bz1 = fp.brick_range(bricks_grid(c))
    b = np.asarray(c.bricks, np.int64)
    return (b[:, 0] >= 0) & (b[:, 0] < nbx) & (b[:, 1] >= 0) & (b[:, 1] < nby) & (b[:, 2] >= bz0) & (b[:, 2] < bz1)


def bricks_classes(c):
    k = {f"tile_{c.tile}", f"lead{c.lead}"}
    if bricks_near_third(c):
        k.add("third_" + bricks_near_third(c))
    if not _pow2(c.den):
        k.add("den_np2")
    if any(math.frexp(v)[0] not in (0.5, -0.5) for v in (c.base_range, c.octave_scale, c.post_scale)):
        k.add("non_dyadic")
    if c.z0 < 0:
        k.add("z0<0")
    if c.z0 % 8 and c.z1 % 8:
        k.add("ragged_z")
    if c.nx % 8 and c.ny % 8:
        k.add("ragged_xy")
    if c.out_scale < 0:
        k.add("neg_out")
    if c.bands is not None:
        s, first, nbands, w = c.bands
        if 0 < fp.active_bands(s, first, nbands) < nbands:
            k.add("s_cut")
        k.add("first_neg" if first < 0 else ("first_pos" if first > 0 else "first_0"))
        if any(x == 0.0 for x in w):
            k.add("zero_w")
    n = len(c.bricks)
    k.add("len1" if n == 1 else ("len_odd" if n % 2 else "len_even"))
    live = bricks_in_range(c)
    if n % 2 == 0 and live[-2:].sum() == 1:
        k.add("half_dead_tail")
    nbx, nby, bz0, bz1 = fp.brick_range(bricks_grid(c))
    b = np.asarray(c.bricks, np.int64)
    for name, hit in (("out_x_lo", b[:, 0] < 0), ("out_x_hi", b[:, 0] >= nbx), ("out_y_lo", b[:, 1] < 0), ("out_y_hi", b[:, 1] >= nby),
                      ("out_z_lo", b[:, 2] < bz0), ("out_z_hi", b[:, 2] >= bz1)):
        if hit.any():
            k.add(name)
    if len({tuple(r) for r in b.tolist()}) < n:
        k.add("duplicate")
    return k


_BRICKS_SIDES = ("out_x_lo", "out_x_hi", "out_y_lo", "out_y_hi", "out_z_lo", "out_z_hi")


def _bricks_slots(seed):
    """(target, near) of a seed's 30 cases: every sep<NB> twice, each declining check once and three of them twice (the two
    seeds take different halves), and five more sep cases; near: the top band's step next to 1/3."""
    slots = [[("sep", nb), None] for nb in range(1, 9)] * 2
    slots = [list(s) for s in slots]
    slots[seed % 8][1] = "below"
    slots[8 + (seed + 3) % 8][1] = "below"
    extra = BRICKS_DECLINES[:3] if seed % 2 else BRICKS_DECLINES[3:]
    slots += [[d, "at_above" if d == "two_mids" else None] for d in BRICKS_DECLINES + extra]
    slots += [[("sep", 1 + (seed + 3 * i) % 8), None] for i in range(5)]
    assert len(slots) == BRICKS_PER_SEED
    return slots


def _draw_bricks(rng, idx, target, near):
    sep = isinstance(target, tuple)
    c = SimpleNamespace(lead=(idx // 4 + idx) % 4, exact=target == "flag")
    c.tile = "empty" if target == "empty tile" else BRICK_TILES[idx % 4]
    nb = target[1] if sep else int(rng.integers(1, 9))
    multi = nb > 1 or target == "no active band" or bool(rng.integers(0, 2))
    nd = idx % 3 == 0
    if multi:
        nbands = nb if idx % 5 else min(8, nb + int(rng.integers(1, 4)))      # s cuts the band count
        first = int(rng.integers(-3, 3))
        s = -16.0 if nbands == nb else -(first + nb) + 0.5
        if target == "no active band":
            s = float(-first) + 0.25
        w = [float(f32(x)) for x in rng.uniform(0.25, 2.0, nbands)]
        if idx % 4 == 1 and nbands >= 2:
            w[int(rng.integers(0, nbands))] = 0.0
        c.bands = (float(s), first, nbands, w)
        c.base_range, c.octave_scale, c.post_scale = 4.0, 1.0, 1.0
        top = 2.0 * 2.0 ** (first + (nb if target != "no active band" else 1) - 1)
    else:
        c.bands = None
        c.base_range, c.octave_scale, c.post_scale = 4.0, float(2.0 ** int(rng.integers(2, 6))), 2.0
        top = 1.0
    if nd:
        f = rng.permutation(len(_ND))[:3]
        c.base_range, c.octave_scale, c.post_scale = (float(f32(v) * f32(_ND[j])) for v, j in
                                                      zip((c.base_range, c.octave_scale, c.post_scale), f))
    num = c.base_range * float(f32(f32(c.octave_scale) * f32(top))) * c.post_scale     # the top band's step is num / den
    if near == "below":
        step = float(rng.uniform(0.981, 0.9995)) / 3.0
    elif near == "at_above":
        step = float(rng.uniform(1.0005, 1.019)) / 3.0
    elif target == "two_mids":
        step = float(rng.uniform(0.4, 2.0))
    elif target == "gate":
        step = float(rng.uniform(0.1, 0.17))
    else:
        step = float(rng.uniform(0.04, 0.3))
    c.den = max(1, int(round(num / step)))
    if idx % 4 == 2 and near is None:
        c.den = 1 << max(0, int(round(math.log2(num / step))))
    step = num / c.den
    # the volume: each axis near or far, ragged or whole bricks, z0 of either sign
    reach = 1.2e6 / step if target == "gate" else min(3.0e5, 0.5 * (1.0 - min(3.0 * step, 0.99)) / fp.SLACK_PER_CELL) / max(step, 1e-3)
    ext = [int(min(reach, float(np.exp(rng.uniform(np.log(9.0), np.log(4.0e6)))))) for _ in range(3)]
    if target == "gate":
        ext[int(rng.integers(0, 3))] = int(reach)
    ragged = idx % 2 == 0
    c.nx, c.ny, c.z1 = (max(9, e // 8 * 8 + (int(rng.integers(1, 8)) if ragged else 0)) for e in ext)
    zsign = idx % 3
    c.z0 = 0 if zsign == 0 else (-int(rng.choice([1003, 8 * 125, 20, 8 * 40000])) if zsign == 1 else int(rng.choice([3, 8, 21])))
    if ragged and c.z0 % 8 == 0:
        c.z0 -= 3
    if target == "negative step":
        c.base_range = -c.base_range
    c.out_scale = float(f32(rng.choice([INV, 1.0, 0.75, -1.5, -INV])))
    # the list
    nbx, nby, bz0, bz1 = fp.brick_range(bricks_grid(c))
    n = 1 if idx % 3 == 0 else (2 * int(rng.integers(1, 20)) + 1 if idx % 3 == 1 else 2 * int(rng.integers(1, 21)))
    b = np.stack([rng.integers(0, nbx, n), rng.integers(0, nby, n), rng.integers(bz0, bz1, n)], -1)
    b[0] = (nbx - 1, nby - 1, bz1 - 1)                                       # the far corner
    if n >= 3:
        b[n // 2] = (0, 0, min(max(bz0, 0), bz1 - 1))                        # next to the origin
        b[1] = b[int(rng.integers(2, n))]                                   # a duplicate
        side = _BRICKS_SIDES[(idx // 3) % 6]
        out = {"out_x_lo": (-1, 0, bz0), "out_x_hi": (nbx, 0, bz0), "out_y_lo": (0, -1, bz0), "out_y_hi": (0, nby, bz0),
               "out_z_lo": (0, 0, bz0 - 1), "out_z_hi": (0, 0, bz1)}[side]
        b[n - 1 - (idx // 2) % 2 if n % 2 == 0 else 2] = out                  # even lists: in the last pair
    c.bricks = np.ascontiguousarray(b, np.int32)
    return c


def bricks_cases(seed):
    """A seed's cases, each with .name, .route (bricks_route's label and declining check)."""
    rng = np.random.default_rng([seed, 7])
    cases = []
    for idx, (target, near) in enumerate(_bricks_slots(seed)):
        for _attempt in range(400):
            c = _draw_bricks(rng, idx, target, near)
            label, why = bricks_route(c)
            hit = (why is None and label == f"sep<{target[1]}>") if isinstance(target, tuple) else why == target
            if hit and (near is None or bricks_near_third(c) == near) and (why is not None or bricks_in_range(c).any()):
                break
        else:
            raise AssertionError(f"the generator cannot place bricks seed {seed} case {idx}: {target} {near}")
        c.route, c.name = (label, why), f"bricks-{seed}-{idx:02d}"
        assert 1 <= len(c.bricks) <= BRICKS_MAX_LIST
        cases.append(c)
    return cases


# ---- Perlin brick lists --------------------------------------------------------------------------------------------------------
PERLIN_BRICKS_SEED = 20257
PERLIN_BRICKS_MAX_LIST = 40
PERLIN_COORD_LIMIT = 2.0 ** 30         # the finest octave's coordinate (tests/test_gpu_far_lattice.py's far point sets keep it)
PERLIN_DEFAULT_OFFSETS = ((0, 0, 0), (85, 85, 85), (170, 170, 170))
_PB_POST = (1.0, 2.0, 0.75, 1.3)
_PB_EXTENTS = (9, 21, 40, 133, 4099, 8 * 50000 + 3, 8 << 17)      # short, ragged and very long
_PB_Z0 = (0, 3, -5, -4099)
_PB_NZ = (1, 9, 24, 70, 4100, 8 * 30000 + 5)


def perlin_finest(kind, depth):
    """The factor of the finest octave's coordinate (0: the call evaluates no octave)."""
    return 1.0 if kind == "noise" else (32.0 if kind == "fractal" else (2.0 ** (depth - 1) if depth >= 1 else 0.0))


def perlin_octave_cells(p, kind, depth):
    """Per octave, the lattice cell (floor, before & 255) of the float32 coordinates p, as RunOctaveWalker::step
    (csrc/wn_perlin_frame.hpp) forms it: noise reads p, turb doubles the FLOAT per octave, fractal_noise multiplies the float
    by a double frequency."""
    p = np.asarray(p, f32)
    if kind == "noise":
        return [np.floor(p.astype(np.float64)).astype(np.int64)]
    if kind == "fractal":
        return [np.floor(p.astype(np.float64) * 2.0 ** i).astype(np.int64) for i in range(FRACTAL_OCTAVES)]
    out, cur = [], p.copy()
    for _ in range(depth):
        out.append(np.floor(cur.astype(np.float64)).astype(np.int64))
        cur = cur * f32(2.0)
    return out


def perlin_row_trips(cells8):
    """Segment trips of one brick row and octave (csrc/wn_perlin_bricks.hip): segments are matched on the cell BYTE
    (cell_at(q) == X), so the loop takes one trip per distinct byte."""
    return len(set((np.asarray(cells8) & 255).tolist()))


def perlin_row_has_hole(cells8):
    """Two samples share a cell byte and a sample between them does not: the mask `mine` is no run of adjacent samples."""
    b = (np.asarray(cells8) & 255).tolist()
    return any(b[i] == b[j] and any(b[k] != b[i] for k in range(i + 1, j)) for i in range(8) for j in range(i + 2, 8))


def perlin_trip_counts(x_rows, calls):
    """(the set of segment-trip counts over the (n, 8) float32 x rows, the calls and their octaves, whether a mask has a hole)."""
    counts, hole = set(), False
    for kind, depth in calls:
        for cells in perlin_octave_cells(x_rows, kind, depth):
            for c8 in cells:
                counts.add(perlin_row_trips(c8))
                hole = hole or perlin_row_has_hole(c8)
    return counts, hole


def perlin_bricks_coords(c, bricks):
    """(n, 512, 3) float32 coordinates of the bricks' samples in slot order, in lattice_coord's order of operations from the
    int64 index."""
    b = np.asarray(bricks, np.int64).reshape(-1, 3)
    l = np.arange(512)
    idx = np.stack([8 * b[:, None, 0] + (l & 7), 8 * b[:, None, 1] + ((l >> 3) & 7), 8 * b[:, None, 2] + (l >> 6)], -1)
    p = (idx.astype(f32) / f32(c.den)) * f32(c.base_range)
    p = p * f32(c.octave_scale)
    return p * f32(c.post_scale)


def perlin_bricks_live(c):
    nbx, nby, bz0, bz1 = fp.brick_range(fp.Grid(c.den, c.nx, c.ny, c.z0, c.z1 - c.z0))
    b = np.asarray(c.bricks, np.int64)
    return (b[:, 0] >= 0) & (b[:, 0] < nbx) & (b[:, 1] >= 0) & (b[:, 1] < nby) & (b[:, 2] >= bz0) & (b[:, 2] < bz1)


def perlin_bricks_box(c):
    """(nx, ny, z0, z1) of the bounding lattice of the in-range bricks, whole bricks from x = y = 0; None beyond CAP samples."""
    b = np.asarray(c.bricks, np.int64)[c.live]
    box = (8 * int(b[:, 0].max() + 1), 8 * int(b[:, 1].max() + 1), 8 * int(b[:, 2].min()), 8 * int(b[:, 2].max() + 1))
    return box if box[0] * box[1] * (box[3] - box[2]) <= CAP else None


def _draw_perlin_brick_list(rng, c, idx):
    """1 to 40 bricks, odd counts at odd idx: in-range bricks drawn over the whole volume with the far corner first; from 2
    bricks on the last is out of range (every sixth list holds a second); from 3 on one has bz = bz0; from 4 on one is a
    duplicate."""
    nbx, nby, bz0, bz1 = fp.brick_range(fp.Grid(c.den, c.nx, c.ny, c.z0, c.z1 - c.z0))
    n = 2 * int(rng.integers(1, PERLIN_BRICKS_MAX_LIST // 2 + 1)) - idx % 2
    b = np.stack([rng.integers(0, nbx, n), rng.integers(0, nby, n), rng.integers(bz0, bz1, n)], -1)
    b[0] = (nbx - 1, nby - 1, bz1 - 1)
    sides = [(-1, 0, bz0), (nbx, 0, bz0), (0, -1, bz0), (0, nby, bz0), (0, 0, bz0 - 1), (0, 0, bz1)]
    if n >= 3:
        b[2, 2] = bz0
    if n >= 4:
        free = [j for j in range(2, n - 1) if j != n // 2 or n < 6]
        b[1] = b[int(rng.choice(free))]
    if n >= 6 and idx % 6 == 0:
        b[n // 2] = sides[(idx // 6 + 3) % 6]
    if n >= 2:
        b[n - 1] = sides[idx % 6]
    return np.ascontiguousarray(b, np.int32)


def perlin_bricks_cases(variant, seed=PERLIN_BRICKS_SEED):
    """One case per slot of _PERLIN_SLOTS (kind, depth, step class, flags n and d; a slot flagged z draws a lattice z range like
    every other: bricks refuse WN_Z_CONST).  A case whose finest octave would see a coordinate past 2^30 is drawn again from
    the same stream."""
    assert variant in PERLIN_CHANNELS
    rng = np.random.default_rng([seed, list(PERLIN_CHANNELS).index(variant)])
    cases = []
    for idx, (kind, depth, _rows, cls, flags) in enumerate(_PERLIN_SLOTS):
        for _attempt in range(400):
            c = SimpleNamespace(variant=variant, kind=kind, depth=depth, lead=idx % 4, seed=12345, calls=[(kind, depth)])
            c.base_range = float(rng.choice([-4.0, -3.0])) if "n" in flags else float(rng.choice([4.0, 4.0, 2.5]))
            c.octave_scale = float(f32(rng.choice([3.7, 0.6, 5.3]))) if "d" in flags else float(rng.choice([1.0, 2.0, 4.0, 16.0]))
            c.post_scale = float(f32(rng.choice(_PB_POST)))
            target = float(rng.uniform(*_STEP_RANGE[cls]))
            c.den = max(1, int(round(abs(c.base_range) * c.octave_scale * c.post_scale / target)))
            c.nx, c.ny = int(rng.choice(_PB_EXTENTS)), int(rng.choice(_PB_EXTENTS))
            c.z0 = int(rng.choice(_PB_Z0))
            c.z1 = c.z0 + int(rng.choice(_PB_NZ))
            c.bounds = (c.nx, c.ny, c.z0, c.z1)
            c.out_scale = float(rng.choice([1.0, 0.75, -2.5]))
            c.offsets = PERLIN_DEFAULT_OFFSETS
            if variant == "curl" and idx % 5 != 4:
                c.offsets = tuple(tuple(int(v) for v in rng.integers(-300, 1100, 3)) for _ in range(3))
            c.bricks = _draw_perlin_brick_list(rng, c, idx)
            c.live = perlin_bricks_live(c)
            c.pmax = float(np.abs(perlin_bricks_coords(c, c.bricks[c.live])).max())
            if perlin_step_class(c) == cls and c.pmax * perlin_finest(kind, depth) <= PERLIN_COORD_LIMIT:
                break
        else:
            raise AssertionError(f"the generator cannot place perlin bricks {variant} case {idx}")
        c.name = f"perlin-bricks-{variant}-{idx:02d}-{kind}{depth}"
        cases.append(c)
    return cases
