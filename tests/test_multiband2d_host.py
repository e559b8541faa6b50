"""CPU checks of WMultibandNoise on a 2-D tile (include/wnoise_multiband2d.h): the host evaluator
wnhost_multiband2d_footprint (host/scalar_eval.h, in libwnoise_host.so; csrc/wn_eval.hpp compiled for the host, the bits of
the kernels) against the float64 reference of tests/_ref64_multiband2d.py, and the new header's symbols.  Nothing touches a
device.

Bound: the per-point, per-channel bound derived in tests/_ref64_multiband2d.py from evaluate2D's operation count, the
chain-rule factors sum_b |w_b f_b| [2^(first_band+b+1)] / out_div and the tile's largest coefficient.  The largest
error / bound ratio observed over all cases and both tiles (printed by test_host_evaluator_matches_ref64) is 0.078 (value
channel 0.078, gradient channels 0.064): a worst-case bound against the tile's largest coefficient is an order of magnitude
above typical rounding.
"""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

from conftest import ROOT, bits

import _ref64_footprint as F
import _ref64_multiband2d as M

PKG = os.path.join(ROOT, "wavelet-noise-in-ray-tracing_amd")
VAR = M.VAR_2D


@pytest.fixture(scope="module")
def host():
    path = os.path.join(PKG, "libwnoise_host.so")
    if not os.path.exists(path):
        import __graft_entry__
        __graft_entry__.build()
    return M.bind_host(C.CDLL(path))


@pytest.fixture(scope="module")
def tiles():
    """2-D tiles 128 (seed 12345) and 6 (not a power of two: the wrap is a modulo), filtered in float64."""
    return {n: M.tile2d(n) for n in (128, 6)}


def test_reference_is_the_sum_of_single_bands(tiles):
    """The float64 reference against its definition written out by hand: s = -2.5 on five bands runs three, the third
    faded by 0.5; the value is sum w_b f_b evaluate2D(2 p 2^b) / sqrt(sum w^2 var)."""
    import _ref64
    coef, w = tiles[128], M.weights(5, 0)
    pts = M.points(0, 5, 64, 1)
    got = M.multiband2d_footprint_points(coef, pts, np.float32(-2.5), 0, 5, w, VAR, 1)
    f = [1.0, 1.0, 0.5]
    want = sum(float(np.float32(w[b])) * f[b] * _ref64.evaluate2d_points(coef, (np.float32(2) * pts) * np.float32(2.0 ** b))
               for b in range(3))
    div = np.sqrt(sum(float(np.float32(x)) ** 2 for x in w) * float(np.float32(VAR)))
    assert np.abs(got[:, 0] - want / div).max() <= 1e-14 * np.abs(want / div).max()


@pytest.mark.parametrize("nb,first,fade", M.CASES, ids=M.CASE_IDS)
@pytest.mark.parametrize("n", [128, 6])
def test_host_evaluator_matches_ref64(host, tiles, n, nb, first, fade):
    coef, w = tiles[n], M.weights(nb, first)
    pts = M.points(first, nb, 1200, 40 + nb + first)
    s = M.footprints(first, nb, len(pts), 50 + nb + first)
    got, val = M.host_multiband2d(host, coef, pts, s, first, nb, w, VAR, fade)
    assert (bits(got[:, 0]) == bits(val)).all()               # the gradient form's value has the value form's bits
    want = M.multiband2d_footprint_points(coef, pts, s, first, nb, w, VAR, fade)
    err = np.abs(got.astype(np.float64) - want)
    tol = M.tolerance(coef, s, first, nb, w, VAR, fade)
    ratio = (err / np.maximum(tol, 1e-300)).max(0)
    print(f"tile {n} nb {nb} first {first} fade {fade}: max error / bound per channel {ratio}")
    assert (err <= tol).all(), (ratio, err.max(0))
    # the draws hold every kind of footprint
    count = F.active_count(s, first, nb)
    none = count == 0
    assert none.any() and np.isnan(s).any() and np.isposinf(s).any() and none[np.isnan(s) | np.isposinf(s)].all()
    assert (got[none] == 0.0).all()                           # no active band: 0 in every channel
    assert np.isneginf(s).any() and (count[np.isneginf(s)] == nb).all() and (count == nb).any()
    integer = np.isfinite(s) & (s == np.round(s))
    assert integer.any()
    # uniform vs footprint: where every f_b == 1 the fade does not enter, so the bits are those of the hard cut at that s,
    # which is what the uniform-s entry points evaluate
    same = M.unfaded(s, first, nb, fade)
    assert same[integer].all() and (same.all() if not fade else True)
    hard, _ = M.host_multiband2d(host, coef, pts[same], s[same], first, nb, w, VAR, 0, value_form=False)
    assert (bits(got[same]) == bits(hard)).all()


def test_point_draws_stay_below_two_to_the_24(tiles):
    for nb, first, _ in M.CASES:
        pts = M.points(first, nb, 1200, 40 + nb + first)
        for b in range(nb):
            assert np.abs((np.float32(2) * pts) * np.float32(2.0 ** (first + b))).max() < 2.0 ** 24


@pytest.mark.parametrize("fade", [0, 1])
def test_zero_weights_and_empty_tile_give_zero(host, tiles, fade):
    pts = M.points(0, 5, 300, 3)
    s = M.footprints(0, 5, len(pts), 4)
    got, val = M.host_multiband2d(host, tiles[128], pts, s, 0, 5, [0.0] * 5, VAR, fade)
    assert (got == 0.0).all() and (val == 0.0).all()         # the sum of w^2 is 0: no division either
    got, val = M.host_multiband2d(host, None, pts, s, 0, 5, F.W8, VAR, fade)
    assert (got == 0.0).all() and (val == 0.0).all()
    got, val = M.host_multiband2d(host, tiles[6], pts, s, 0, 9, F.W8 + [1.0], VAR, fade)   # nbands out of range
    assert (got == 0.0).all() and (val == 0.0).all()


def test_one_unit_band_is_evaluate2d(host, tiles):
    """One band, w = [1], var_per_band = 1: out_div is 1 and the value has the bits of evaluate2D at 2 p 2^first_band."""
    host.wnhost_eval2d.restype = C.c_float
    host.wnhost_eval2d.argtypes = [M.FP, C.c_int, M.FP]
    coef = tiles[128]
    pts = M.points(4, 1, 400, 5)
    got, _ = M.host_multiband2d(host, coef, pts, np.float32(-np.inf), 4, 1, [1.0], 1.0, 0)
    q = np.ascontiguousarray((np.float32(2) * pts) * np.float32(16.0))
    want = np.array([host.wnhost_eval2d(coef.ctypes.data_as(M.FP), 128, q[i].ctypes.data_as(M.FP)) for i in range(len(q))],
                    np.float32)
    assert (bits(got[:, 0]) == bits(want)).all()


def test_multiband2d_header_symbols_all_exported_and_bound():
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(PKG, "libwnoise_hip.so")):
        ge.build()
    capi = importlib.import_module("wavelet-noise-in-ray-tracing_amd._capi")
    lib = capi.load()
    text = open(os.path.join(ROOT, "include", "wnoise_multiband2d.h")).read()
    names = sorted(set(re.findall(r"WN_API\s+[\w\s\*]+?\b(wn_\w+)\s*\(", text)))
    assert len(names) == 6, names
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/wnoise_multiband2d.h but not exported"
    assert set(capi.MULTIBAND2D_SIGNATURES) == set(names)
