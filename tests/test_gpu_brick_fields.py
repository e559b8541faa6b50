"""Gradient and curl brick lists of the 3-D wavelet volume (include/wnoise_brick_fields.h): wn_eval3d_grad_bricks,
wn_multiband3d_grad_bricks, wn_eval3d_curl_bricks and wn_multiband3d_curl_bricks evaluate the lattices of the dense
derivative grids on a device list of 8^3 bricks, into CH consecutive slot arrays, out[(ch n + i) 512 + lx + 8 (ly + 8 lz)];
CH = 4 {value, d/dx, d/dy, d/dz} or 3 {vx, vy, vz}.

The fixtures are those of tests/test_gpu_bricks.py, by import: the volume 40 x 24 x [8, 32), LIST (23 bricks, 19 in range),
ONE, RAGGED, the lattices in and out of the separable kernels' regime, and tests/_frame.py frames whose `lead` walks 0..3.
The references are computed once per lattice and shared: the dense derivative grids over the bounding lattice in both tiers
(wavelet_gradient_volume / curl_volume and their multiband forms), gathered brick by brick; the point entries at the samples'
float coordinates; the float64 references of tests/_ref64_grad.py and tests/_ref64_curl.py with their tolerance() -- G =
1e-5 |out_scale| (multiband: * sum_b |w_b| 2^(first_band+b+1) / out_div) for the gradient, 2 G for the curl.  The curl calls
use tests/test_gpu_curl.py's MIXED offsets, and the library's default offsets once.

This module stays within 5 bricks of the origin in x and y; its one far test moves the volume in z on den 512, where every
coordinate is exact in float32.  Far from the origin on all three axes, on lattices that round, at the planner's edges and
on drawn lattices: tests/test_gpu_brick_fields_far.py and the field-bricks family of tests/test_gpu_lattice_sweep.py."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _ref64  # noqa: E402
import _ref64_curl as RC  # noqa: E402
import _ref64_grad as RG  # noqa: E402
import test_gpu_bounded as tb  # noqa: E402
import test_gpu_bricks as tbr  # noqa: E402
import test_gpu_curl as tc  # noqa: E402
import test_gpu_stride_pass as sp  # noqa: E402
from _frame import SENTINEL_BITS, Frame  # noqa: E402
from test_gpu_bricks import (BOUNDS, FALLBACK_LATTICES, LIST, MB_FALLBACK, MB_SEP, ONE, RAGGED, SEP_LATTICES, VAR, case_id,  # noqa: E402
                             in_range, same_bits, weights)

PKG = tbr.PKG
f32 = np.float32
KINDS = ("grad", "curl")
CH = {"grad": 4, "curl": 3}
MIXED = tc.MIXED
FAR_Z = 100000                      # a multiple of 8: the volume moved to z in [100008, 100032)
SINGLE = [(k, i, c) for k in KINDS for i, c in enumerate(SEP_LATTICES + FALLBACK_LATTICES)]
MULTI = [(k, i, c) for k in KINDS for i, c in enumerate(MB_SEP + MB_FALLBACK)]


def ids(v):
    return case_id(v) if isinstance(v, tuple) else None


def fgather(vol, bricks):
    """(CH, n, 512): the bricks' slots out of the bounding lattice's (CH, 24, 24, 40) volumes, channel by channel."""
    return np.stack([tbr.gather(v, bricks) for v in vol])


def brick_coords(g, den, bricks):
    """(n * 512, 3) float32 coordinates of the samples of `bricks`, in slot order, formed as the header forms them."""
    l = np.arange(512)
    b = np.asarray(bricks, np.int64)
    idx = np.stack([8 * b[:, None, 0] + (l & 7), 8 * b[:, None, 1] + ((l >> 3) & 7), 8 * b[:, None, 2] + (l >> 6)], -1)
    return np.ascontiguousarray(_ref64.lattice_coords(idx, den, g.base_range, g.octave_scale, g.post_scale).reshape(-1, 3))


class Env(tbr.Env):
    def __init__(self, wn):
        super().__init__(wn)
        self.field_vol = functools.lru_cache(maxsize=None)(self._field_vol)
        self.ref64 = functools.lru_cache(maxsize=None)(self._ref64)

    def symbol(self, kind, mb):
        return f"wn_{'eval3d' if mb is None else 'multiband3d'}_{kind}_bricks"

    def fcall(self, kind, tile, g, bricks_ptr, n, out_ptr, mb=None, offsets=MIXED):
        """The status of one C-ABI call."""
        nm, obj = self.nm, self.objs[tile]
        argv = [obj._handle(3), C.byref(g) if g is not None else None, bricks_ptr, n]
        if kind == "curl":
            argv.append(obj._curl_offsets(offsets) if offsets != "null" else None)
        if mb is not None:
            s, first, nb = mb
            argv += [float(s), int(first), int(nb), (C.c_float * max(1, nb))(*weights(nb)), VAR]
        return getattr(nm._lib, self.symbol(kind, mb))(*argv, out_ptr, nm._stream())

    def frun(self, kind, tile, den, bricks, lead, octave=None, mb=None, exact=False, bounds=BOUNDS, offsets=MIXED):
        """One call into a frame of CH channel arrays: the (CH, n, 512) payload, after the checks of what was written -- the
        guards intact, every in-range slot of every channel written, every other still the sentinel, the list unchanged."""
        import torch
        n, ch = len(bricks), CH[kind]
        dev = torch.from_numpy(np.ascontiguousarray(bricks)).cuda()
        frame = Frame(ch * 512 * n, lead)
        rc = self.fcall(kind, tile, self.grid(den, bounds, octave, exact), self.nm._ptr(dev), n, frame.ptr, mb, offsets)
        assert rc == 0, self.nm._lib.wn_last_error()
        live = in_range(bricks, bounds)
        got = frame.result(written=np.tile(np.repeat(live, 512), ch), what=f"{kind} {tile} den {den}").reshape(ch, n, 512)
        assert (dev.cpu().numpy() == bricks).all(), "the brick list was written"
        assert (got[:, ~live].view(np.uint32) == SENTINEL_BITS).all()
        return got

    def _field_vol(self, kind, tile, den, octave, mb, exact, default_offsets=False, zshift=0):
        """The dense derivative grid over the bounding lattice 40 x 24 x [8, 32) (+ zshift), on the host: (CH, 24, 24, 40)."""
        nx, ny, z0, z1 = BOUNDS
        wn, obj, off = self.wn, self.objs[tile], None if default_offsets else MIXED
        z0, z1 = z0 + zshift, z1 + zshift
        if mb is None:
            v = wn.wavelet_gradient_volume(obj, den, nx, ny, z0, z1, octave, exact=exact) if kind == "grad" else \
                wn.curl_volume(obj, den, nx, ny, z0, z1, octave, offsets=off, exact=exact)
        else:
            s, first, nb = mb
            v = wn.multiband_gradient_volume(obj, den, nx, ny, z0, z1, s, first, nb, weights(nb), exact=exact) if kind == "grad" else \
                wn.multiband_curl_volume(obj, den, nx, ny, z0, z1, s, first, nb, weights(nb), offsets=off, exact=exact)
        return v.cpu().numpy()

    def out_scale(self, octave):
        return float(self.grid(512, BOUNDS, octave).out_scale)

    def _ref64(self, kind, tile, den, octave, mb, default_offsets=False):
        """The float64 reference over the bounding lattice: (CH, 24, 24, 40)."""
        nx, ny, z0, z1 = BOUNDS
        coef = self.coefs[tile]
        if coef.size == 0:
            return np.zeros((CH[kind], z1 - z0, ny, nx))
        g = self.grid(den, BOUNDS, octave)
        px, py, pz = (_ref64.lattice_coords(np.arange(a, b), den, g.base_range, g.octave_scale, g.post_scale)
                      for a, b in ((0, nx), (0, ny), (z0, z1)))
        off = RC.default_offsets(RC.tile_size(coef)) if default_offsets else MIXED
        if mb is None:
            v = RG.evaluate_lattice_grad(coef, px, py, pz) if kind == "grad" else RC.evaluate_lattice_curl(coef, px, py, pz, off)
            return v * float(g.out_scale)
        s, first, nb = mb
        if kind == "grad":
            return RG.multiband_lattice_grad(coef, px, py, pz, s, first, nb, weights(nb), VAR)
        return RC.multiband_lattice_curl(coef, px, py, pz, off, s, first, nb, weights(nb), VAR)

    def ref64_points(self, kind, tile, pts, octave, mb):
        """The float64 reference at float32 points: (N, CH)."""
        coef = self.coefs[tile]
        if mb is None:
            v = RG.evaluate3d_grad_points(coef, pts) if kind == "grad" else RC.evaluate3d_curl_points(coef, pts, MIXED)
            return v * self.out_scale(octave)
        s, first, nb = mb
        if kind == "grad":
            return RG.multiband_grad_points(coef, pts, s, first, nb, weights(nb), VAR)
        return RC.multiband_curl_points(coef, pts, MIXED, s, first, nb, weights(nb), VAR)

    def tol(self, kind, octave, mb):
        t = RG.tolerance(self.out_scale(octave)) if mb is None else RG.tolerance(1.0, (mb[0], mb[1], mb[2], weights(mb[2]), VAR))
        return t if kind == "grad" else 2.0 * t

    def fpoints(self, kind, tile, den, bricks, octave, mb, offsets=MIXED):
        """The point entry at the float coordinates of every sample of `bricks`, times out_scale: (CH, n, 512)."""
        import torch
        g = self.grid(den, BOUNDS, octave)
        pts = torch.from_numpy(brick_coords(g, den, bricks)).cuda()
        obj = self.objs[tile]
        if mb is None:
            v = obj.evaluate3DGradient(pts) if kind == "grad" else obj.evaluate3DCurl(pts, offsets)
        else:
            s, first, nb = mb
            v = obj.WMultibandNoiseGradient(pts, s, first, nb, weights(nb), VAR) if kind == "grad" else \
                obj.WMultibandNoiseCurl(pts, s, first, nb, weights(nb), VAR, offsets)
        v = v.cpu().numpy().astype(f32) * f32(g.out_scale)
        return np.ascontiguousarray(v.reshape(len(bricks), 512, CH[kind]).transpose(2, 0, 1))


@pytest.fixture(scope="module")
def env():
    import importlib
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU (the product has no CPU path)"
    return Env(importlib.import_module("wavelet-noise-in-ray-tracing_amd"))


def differs(a, b):
    return bool((np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).any())


# ---- exact tier ----------------------------------------------------------------------------------------------------------------
def exact_tier(env, i, kind, tile, den, octave, mb):
    live = in_range(LIST, BOUNDS)
    got = env.frun(kind, tile, den, LIST, i % 4, octave=octave, mb=mb, exact=True)
    vol = env.field_vol(kind, tile, den, octave, mb, True)
    same_bits(got[:, live], fgather(vol, LIST[live]), "against the exact dense grid")
    same_bits(got[:, live], env.fpoints(kind, tile, den, LIST[live], octave, mb), "against the point entry")
    if kind == "grad":
        same_bits(got[0][live], env.run(tile, den, LIST, (i + 3) % 4, octave=octave, mb=mb, exact=True)[live],
                  "channel 0 against the exact value bricks")
    one = env.frun(kind, tile, den, ONE, (i + 1) % 4, octave=octave, mb=mb, exact=True)
    same_bits(one, fgather(vol, ONE), "the one-brick list")
    # boundary bricks are whole: a ragged volume with the same bricks writes the same bits
    ragged = env.frun(kind, tile, den, LIST, (i + 2) % 4, octave=octave, mb=mb, exact=True, bounds=RAGGED)
    same_bits(ragged[:, live], got[:, live], "ragged bounds")
    if tile == "empty" or mb == tb.MB_CASES[-1]:
        assert (got[:, live] == 0.0).all()       # the empty tile; no active band
    else:
        assert all(np.abs(got[ch][live]).max() > 1e-3 for ch in range(CH[kind]))


@pytest.mark.gpu
@pytest.mark.parametrize("kind,i,case", SINGLE, ids=ids)
def test_exact_tier_single_band(env, kind, i, case):
    tile, den, octave = case
    exact_tier(env, i, kind, tile, den, octave, None)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,i,case", MULTI, ids=ids)
def test_exact_tier_multiband(env, kind, i, case):
    exact_tier(env, i, kind, case[0], case[1], None, case[2:])


# ---- default tier --------------------------------------------------------------------------------------------------------------
def default_tier(env, i, kind, tile, den, octave, mb, fallback):
    live = in_range(LIST, BOUNDS)
    fast = env.frun(kind, tile, den, LIST, i % 4, octave=octave, mb=mb)
    exact_vol = env.field_vol(kind, tile, den, octave, mb, True)
    exact = fgather(exact_vol, LIST[live])
    want = fgather(env.ref64(kind, tile, den, octave, mb), LIST[live])
    tol = env.tol(kind, octave, mb)
    assert np.isfinite(fast[:, live]).all()
    for ch in range(CH[kind]):
        e_ref = float(np.abs(fast[ch][live].astype(np.float64) - want[ch]).max())
        e_ex = float(np.abs(fast[ch][live].astype(np.float64) - exact[ch]).max())
        print(f"{kind} {tile} den {den} octave {octave} bands {mb} channel {ch}: |default - ref64| {e_ref:.3g}, "
              f"|default - exact| {e_ex:.3g}, tolerance {tol:.3g}")
        assert e_ref <= tol and e_ex <= tol, (ch, e_ref, e_ex, tol)
    one = env.frun(kind, tile, den, ONE, (i + 1) % 4, octave=octave, mb=mb)
    assert np.abs(one.astype(np.float64) - fgather(env.ref64(kind, tile, den, octave, mb), ONE)).max() <= tol
    if fallback:
        same_bits(fast[:, live], exact, "an out-of-regime lattice runs the exact kernel")
    else:
        assert differs(fast[:, live], exact), "the separable kernel did not run"
        if kind == "grad":
            same_bits(fast[0][live], env.run(tile, den, LIST, (i + 3) % 4, octave=octave, mb=mb)[live],
                      "channel 0 against the default value bricks")
        dense = env.field_vol(kind, tile, den, octave, mb, False)
        assert differs(dense, exact_vol), "the dense call did not run its separable kernel"
        same_bits(fast[:, live], fgather(dense, LIST[live]), "against the dense default-tier grid")
    # the bits do not depend on where the output lies, nor on the volume's extent inside its boundary bricks
    same_bits(env.frun(kind, tile, den, LIST, (i + 1) % 4, octave=octave, mb=mb)[:, live], fast[:, live], "another output alignment")
    same_bits(env.frun(kind, tile, den, LIST, (i + 2) % 4, octave=octave, mb=mb, bounds=RAGGED)[:, live], fast[:, live], "ragged bounds")


@pytest.mark.gpu
@pytest.mark.parametrize("kind,i,case", SINGLE, ids=ids)
def test_default_tier_single_band(env, kind, i, case):
    tile, den, octave = case
    default_tier(env, i, kind, tile, den, octave, None, case in FALLBACK_LATTICES)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,i,case", MULTI, ids=ids)
def test_default_tier_multiband(env, kind, i, case):
    default_tier(env, i, kind, case[0], case[1], None, case[2:], case in MB_FALLBACK)


@pytest.mark.gpu
@pytest.mark.parametrize("mb", [None, tb.MB_CASES[1]], ids=["one_band", "five_bands"])
@pytest.mark.parametrize("kind", KINDS)
def test_default_tier_far_in_z_has_the_dense_grids_bits(env, kind, mb):
    """The volume moved to z in [100008, 100032) and the bricks' z with it: absolute z indices and the dense grid's z0 agree."""
    octave = 4 if mb is None else None
    live = in_range(LIST, BOUNDS)
    far = LIST + np.array([0, 0, FAR_Z // 8], np.int32)
    bounds = (BOUNDS[0], BOUNDS[1], BOUNDS[2] + FAR_Z, BOUNDS[3] + FAR_Z)
    assert (in_range(far, bounds) == live).all()
    dense = env.field_vol(kind, "t128", 512, octave, mb, False, False, FAR_Z)
    assert differs(dense, env.field_vol(kind, "t128", 512, octave, mb, True, False, FAR_Z)), "the dense call did not run its separable kernel"
    assert differs(dense, env.field_vol(kind, "t128", 512, octave, mb, False))               # another part of the volume
    got = env.frun(kind, "t128", 512, far, 0, octave=octave, mb=mb, bounds=bounds)
    same_bits(got[:, live], fgather(dense, LIST[live]), "against the dense default-tier grid, far in z")


@pytest.mark.gpu
@pytest.mark.parametrize("exact", [False, True], ids=["default", "exact"])
def test_default_offsets(env, exact):
    """offsets=None: the library's (0, 0, 0), (n/3,)*3, (2n/3,)*3, as curl_volume takes them."""
    live = in_range(LIST, BOUNDS)
    for mb in (None, tb.MB_CASES[1]):
        octave = 4 if mb is None else None
        got = env.frun("curl", "t128", 512, LIST, 0, octave=octave, mb=mb, exact=exact, offsets=None)
        same_bits(got[:, live], fgather(env.field_vol("curl", "t128", 512, octave, mb, exact, True), LIST[live]), "against the dense grid")
        assert np.abs(got[:, live].astype(np.float64) - fgather(env.ref64("curl", "t128", 512, octave, mb, True), LIST[live])).max() \
            <= env.tol("curl", octave, mb)
        assert differs(got[:, live], env.frun("curl", "t128", 512, LIST, 0, octave=octave, mb=mb, exact=exact)[:, live])


# ---- placement -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mb", [None, tb.MB_CASES[1]], ids=["one_band", "five_bands"])
@pytest.mark.parametrize("kind", KINDS)
def test_a_bricks_bits_do_not_depend_on_its_place(env, kind, mb):
    """The same brick first, last and alone, and as a duplicate, in the default tier."""
    octave = 4 if mb is None else None
    brick = np.array([(3, 1, 2)], np.int32)
    rest = LIST[(LIST != brick[0]).any(1)]
    run = lambda bricks, lead: env.frun(kind, "t128", 512, bricks, lead, octave=octave, mb=mb)   # noqa: E731
    alone = run(brick, 0)[:, 0]
    first = run(np.concatenate([brick, rest]), 1)[:, 0]
    last = run(np.concatenate([rest, brick]), 2)[:, -1]
    even = run(np.concatenate([rest[:5], brick, rest[5:], brick]), 3)
    for got, what in ((first, "first"), (last, "last"), (even[:, 5], "sixth"), (even[:, -1], "duplicate")):
        same_bits(got, alone, what)
    dup = run(LIST, 0)
    same_bits(dup[:, 10], dup[:, 14], "the list's duplicate")


def caps():
    """One pass of each launch, in bricks: read from the kernels' source."""
    src = open(os.path.join(PKG, "csrc", "wn_wavelet_brick_fields.hip")).read()

    def cap(name):
        (expr,) = re.findall(r"constexpr size_t %s = ([^;]+);" % name, src)
        value = 1
        for f in expr.split("*"):
            value *= int(f.strip().rstrip("u"))
        return value

    assert "stride_blocks((n + 1) / 2 * 256, kSepBlockCap)), block(256);" in src
    assert "wn::stride_blocks(d.count * kSamples, kCurlExactBlockCap) : wn::stride_blocks(d.count * kSamples)), block(256);" in src
    sep = 2 * cap("kSepBlockCap")
    return {("grad", False): sep, ("curl", False): sep, ("grad", True): sp.STRIDE_BLOCK_CAP * sp.LANES // 512,
            ("curl", True): cap("kCurlExactBlockCap") * 256 // 512}


@pytest.mark.gpu
@pytest.mark.parametrize("exact", [False, True], ids=["separable", "exact"])
@pytest.mark.parametrize("mb", [None, tb.MB_CASES[1]], ids=["one_band", "five_bands"])
@pytest.mark.parametrize("kind", KINDS)
def test_a_second_grid_stride_trip(env, kind, mb, exact):
    """A list a few workgroups longer than one pass of the launch cap.  The head is random bricks of the 512^3 volume, 64 of
    them checked against the point entry (exact tier: bits) or the float64 reference (default tier: the tolerance); the
    tail -- LIST, whose bricks the second trip serves -- is checked against the exact dense grid."""
    per_pass = caps()[(kind, exact)]
    assert per_pass == ((8192 if kind == "grad" else 1024) if exact else 4096)
    octave = 4 if mb is None else None
    head = np.random.default_rng(5).integers(0, 64, (per_pass, 3)).astype(np.int32)
    bricks = np.concatenate([head, LIST])
    bounds = (512, 512, 0, 512)
    live = in_range(LIST, bounds)
    assert live.sum() == 22                       # only (-1, 0, 1) is out of range of the whole volume
    inside = live & in_range(LIST, BOUNDS)        # ... but not in the reference lattice
    got = env.frun(kind, "t128", 512, bricks, 1 if exact else 0, octave=octave, mb=mb, exact=exact, bounds=bounds)
    tail = got[:, per_pass:]
    want = fgather(env.field_vol(kind, "t128", 512, octave, mb, True), LIST[inside])
    tol = env.tol(kind, octave, mb)
    if exact:
        same_bits(tail[:, inside], want, "the second trip's bricks")
    else:
        assert np.abs(tail[:, inside].astype(np.float64) - want).max() <= tol
        same_bits(tail[:, inside], env.frun(kind, "t128", 512, LIST, 2, octave=octave, mb=mb)[:, inside],
                  "the second trip against a short list")
    assert np.isfinite(got[:, :per_pass]).all() and np.abs(got[:, :per_pass]).max() > 0.1
    pick = np.sort(np.random.default_rng(11).choice(per_pass, 64, replace=False))
    if exact:
        same_bits(got[:, pick], env.fpoints(kind, "t128", 512, head[pick], octave, mb), "the first trip's bricks against the point entry")
    else:
        pts = brick_coords(env.grid(512, bounds, octave), 512, head[pick])
        ref = env.ref64_points(kind, "t128", pts, octave, mb).reshape(64, 512, CH[kind]).transpose(2, 0, 1)
        assert np.abs(got[:, pick].astype(np.float64) - ref).max() <= tol


# ---- argument checks -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_argument_checks(env):
    import torch
    nm, lib = env.nm, env.nm._lib
    n = len(LIST)
    dev = torch.from_numpy(LIST).cuda()
    frame = Frame(4 * 512 * n, 0)
    bp = nm._ptr(dev)
    h = env.objs["t128"]._handle(3)

    def err():
        return lib.wn_last_error().decode()

    def four(g, bricks, count, out, offsets=MIXED):
        """The status of the four entry points (five valid bands), which agree, as do their messages."""
        seen = []
        for kind in KINDS:
            for mb in (None, (-16.0, 0, 5)):
                rc = env.fcall(kind, "t128", g, bricks, count, out, mb, offsets)
                seen.append((rc, err() if rc else ""))
        assert len(set(seen)) == 1, seen
        return seen[0][0]

    good = env.grid(512, BOUNDS, 4)
    for kind in KINDS:
        for mb in (None, (-16.0, 0, 5)):
            fr = Frame(CH[kind] * 512 * n, 0)
            assert env.fcall(kind, "t128", good, bp, n, fr.ptr, mb) == 0
            fr.result(written=np.tile(np.repeat(in_range(LIST, BOUNDS), 512), CH[kind]))
    # wn_eval3d_grid's checks on g, with its messages
    assert four(None, bp, n, frame.ptr) == 1 and err() == "wn_grid is NULL"
    assert four(env.grid(0, BOUNDS, 4), bp, n, frame.ptr) == 1 and "wn_grid.den must be > 0" in err()
    assert four(env.grid(512, (-1, 24, 8, 32), 4), bp, n, frame.ptr) == 1 and "nx/ny must be >= 0" in err()
    assert four(env.grid(512, (40, 24, 32, 8), 4), bp, n, frame.ptr) == 1 and "z1 < z0" in err()
    # bricks are three-dimensional; n == 0 comes after that check and before the pointers'
    zc = env.grid(512, BOUNDS, 4)
    zc.z_mode = nm.WN_Z_CONST
    assert four(zc, bp, n, frame.ptr) == 1 and "three-dimensional" in err()
    assert lib.wn_eval3d_bricks(h, C.byref(zc), bp, n, frame.ptr, nm._stream()) == 1
    value_message = err()
    assert four(zc, bp, n, frame.ptr) == 1 and err() == value_message
    assert four(zc, None, 0, None) == 1
    assert four(good, None, 0, None) == 0
    assert four(good, None, n, frame.ptr) == 1 and err() == "bricks_dev is NULL"
    assert four(good, bp, n, None) == 1 and err() == "out_dev is NULL"
    # CH * n * 512 overflows where n * 512 does not yet
    for kind in KINDS:
        most = ((1 << 64) - 1) // 512 // CH[kind]
        for mb in (None, (-16.0, 0, 5)):
            assert env.fcall(kind, "t128", good, bp, most + 1, frame.ptr, mb) == 1 and "overflows size_t" in err()
    assert lib.wn_eval3d_bricks(h, C.byref(env.grid(512, (0, 24, 8, 32), 4)), bp, ((1 << 64) - 1) // 512 // 3 + 1, frame.ptr, nm._stream()) == 0
    # the curl's offsets, checked as wn_eval3d_curl_grid checks them
    for mb in (None, (-16.0, 0, 5)):
        assert env.fcall("curl", "t128", good, bp, n, frame.ptr, mb, "null") == 1
        assert err() == f"{env.symbol('curl', mb)}: offsets9_host is NULL"
    assert lib.wn_eval3d_curl_grid(h, C.byref(good), None, frame.ptr, nm._stream()) == 1 and err() == "wn_eval3d_curl_grid: offsets9_host is NULL"
    # the bands' checks of wn_multiband3d_grid
    off = env.objs["t128"]._curl_offsets(MIXED)
    for kind in KINDS:
        fn = getattr(lib, f"wn_multiband3d_{kind}_bricks")
        lead = (h, C.byref(good), bp, n) + ((off,) if kind == "curl" else ())
        assert fn(*lead, -16.0, 0, 9, (C.c_float * 9)(), VAR, frame.ptr, nm._stream()) == 1 and "nbands must be in 0..8" in err()
        assert fn(*lead, -16.0, 0, 3, None, VAR, frame.ptr, nm._stream()) == 1 and err() == "w_host is NULL"
    # a 2-D tile is refused as wn_eval3d_grid refuses it
    t2 = env.wn.WaveletNoise(128, 12345)
    t2.generateNoiseTile2D()
    assert lib.wn_eval3d_grid(t2._handle(2), C.byref(good), frame.ptr, nm._stream()) == 1
    want = err().replace("wn_eval3d_grid", "X")
    for kind in KINDS:
        for mb in (None, (-16.0, 0, 5)):
            name = env.symbol(kind, mb)
            argv = [t2._handle(2), C.byref(good), bp, n] + ([off] if kind == "curl" else [])
            if mb is not None:
                argv += [-16.0, 0, 5, (C.c_float * 5)(*weights(5)), VAR]
            assert getattr(lib, name)(*argv, frame.ptr, nm._stream()) == 1 and err().replace(name, "X") == want, err()
    # an empty volume has no brick in range
    for empty in ((0, 24, 8, 32), (40, 0, 8, 32), (40, 24, 8, 8)):
        assert four(env.grid(512, empty, 4), bp, n, frame.ptr) == 0
    frame.result(written=np.zeros(4 * 512 * n, bool), what="refused calls and empty volumes write nothing")


# ---- above the ABI -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_python_wrappers(env):
    import torch
    wn, t = env.wn, env.objs["t128"]
    dev = torch.from_numpy(LIST).cuda()
    live = in_range(LIST, BOUNDS)
    mb = tb.MB_CASES[1]
    for exact in (False, True):
        for kind, ch in CH.items():
            if kind == "grad":
                one = wn.wavelet_gradient_bricks(t, 512, dev, 4, bounds=BOUNDS, exact=exact)
                five = wn.multiband_gradient_bricks(t, 512, dev, mb[0], mb[1], mb[2], weights(mb[2]), bounds=BOUNDS, exact=exact)
            else:
                one = wn.curl_bricks(t, 512, dev, 4, offsets=MIXED, bounds=BOUNDS, exact=exact)
                five = wn.multiband_curl_bricks(t, 512, dev, mb[0], mb[1], mb[2], weights(mb[2]), offsets=MIXED, bounds=BOUNDS, exact=exact)
            for out, octave, bands in ((one, 4, None), (five, None, mb)):
                assert out.shape == (ch, 23, 8, 8, 8) and out.dtype == torch.float32 and out.is_cuda
                same_bits(out.cpu().numpy().reshape(ch, 23, 512)[:, live],
                          env.frun(kind, "t128", 512, LIST, 0, octave=octave, mb=bands, exact=exact)[:, live], f"{kind} wrapper")
    # [channel][brick][z][y][x]; bounds default to den on each axis; offsets default to the library's
    pair = torch.tensor([[1, 0, 4], [0, 1, 0]], dtype=torch.int32, device="cuda")
    vol = wn.wavelet_gradient_volume(t, 512, 16, 16, 0, 40, 4, exact=True).cpu().numpy()
    got = wn.wavelet_gradient_bricks(t, 512, pair, 4, exact=True).cpu().numpy()
    same_bits(got[:, 0], vol[:, 32:40, 0:8, 8:16], "gradient brick (1, 0, 4)")
    same_bits(got[:, 1], vol[:, 0:8, 8:16, 0:8], "gradient brick (0, 1, 0)")
    cvol = wn.curl_volume(t, 512, 16, 16, 0, 40, 4, exact=True).cpu().numpy()
    cgot = wn.curl_bricks(t, 512, pair, 4, exact=True).cpu().numpy()
    same_bits(cgot[:, 0], cvol[:, 32:40, 0:8, 8:16], "curl brick (1, 0, 4)")
    same_bits(cgot[:, 1], cvol[:, 0:8, 8:16, 0:8], "curl brick (0, 1, 0)")
    # out= is written in place; a wrong list or output is refused
    mine = torch.zeros(4 * 2 * 512, dtype=torch.float32, device="cuda")
    back = wn.wavelet_gradient_bricks(t, 512, pair, 4, exact=True, out=mine)
    assert back.data_ptr() == mine.data_ptr() and back.shape == (4, 2, 8, 8, 8)
    same_bits(mine.cpu().numpy(), got, "out=")
    back = wn.curl_bricks(t, 512, pair, 4, exact=True, out=mine[:3 * 2 * 512])
    assert back.data_ptr() == mine.data_ptr() and back.shape == (3, 2, 8, 8, 8)
    same_bits(mine[:3 * 2 * 512].cpu().numpy(), cgot, "out=")
    assert wn.wavelet_gradient_bricks(t, 512, pair[:0], 4).shape == (4, 0, 8, 8, 8)
    assert wn.multiband_curl_bricks(t, 512, pair[:0]).shape == (3, 0, 8, 8, 8)
    for wrong in (pair.to(torch.int64), pair.cpu(), pair.reshape(-1), pair.t(), LIST):
        with pytest.raises(ValueError):
            wn.wavelet_gradient_bricks(t, 512, wrong, 4)
        with pytest.raises(ValueError):
            wn.curl_bricks(t, 512, wrong, 4)
    with pytest.raises(ValueError):
        wn.wavelet_gradient_bricks(t, 512, pair, 4, out=mine[:2 * 512])       # one channel's worth
    with pytest.raises(ValueError):
        wn.curl_bricks(t, 512, pair, 4, out=mine)                             # four channels' worth
    with pytest.raises(ValueError):
        wn.multiband_gradient_bricks(t, 512, pair, out=mine.double())
    with pytest.raises(ValueError):
        wn.curl_bricks(t, 512, pair, 4, offsets=((0, 0, 0), (1, 1, 1)))


@pytest.mark.gpu
def test_host_classes_match_the_c_abi(tmp_path):
    exe = tmp_path / "brick_fields_api_check"
    src = os.path.join(HERE, "host_src", "brick_fields_api_check.cpp")
    build = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                            "-I" + os.path.join(PKG, "host"), src, "-o", str(exe), "-L" + PKG, "-lwnoise_host",
                            "-lwnoise_hip", "-Wl,-rpath," + PKG], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run(["timeout", "-k", "10", "300", str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "mismatches 0" in run.stdout, run.stdout
