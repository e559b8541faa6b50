"""CPU checks of WMultibandNoise with a footprint per sample (include/wnoise_footprint.h): the host evaluator
wnhost_multiband3d_footprint (host/scalar_eval.h, in libwnoise_host.so; csrc/wn_eval.hpp compiled for the host, the bits of
the kernels) against the float64 reference of tests/_ref64_footprint.py, and the new header's symbols.  Nothing touches a
device.

Bounds: the evaluate3D bands lie within _ref64_grad.tolerance(1.0, (s_i, first_band, nbands, w, var_per_band)) of the
reference per point and channel (the weights enter it unfaded: f_b <= 1); the projected bands within the per-point bound
that _ref64_grad_surface.multiband_projected_grad_points forms (sum_b |w_b f_b| * the band's bound, divided like the sum).
"""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

from conftest import ROOT, bits

import _ref64
import _ref64_footprint as F

PKG = os.path.join(ROOT, "wavelet-noise-in-ray-tracing_amd")
VAR, VAR_PROJ = 0.18402, 0.296


@pytest.fixture(scope="module")
def host():
    path = os.path.join(PKG, "libwnoise_host.so")
    if not os.path.exists(path):
        import __graft_entry__
        __graft_entry__.build()
    return F.bind_host(C.CDLL(path))


@pytest.fixture(scope="module")
def tiles():
    """Tiles 128 (seed 12345) and 6 (not a power of two), filtered in float64 from Gaussian fields."""
    return {n: _ref64.tile(_ref64.tile_fields(n, 3, 12345)["gauss"], n, 3).astype(np.float32) for n in (128, 6)}


def test_band_factors_follow_the_definition():
    """The reference's own band logic on hand-computed footprints (first_band 0, 5 bands)."""
    s = np.float32([-np.inf, np.inf, np.nan, 0.0, -1.0, -1.5, -5.0, -4.75, np.nextafter(np.float32(-2), np.float32(0))])
    active, f = F.band_factors(s, 0, 5, 1)
    assert active.sum(1).tolist() == [5, 0, 0, 0, 1, 2, 5, 5, 2]
    assert f[0].tolist() == [1.0] * 5
    assert f[4].tolist() == [1.0, 0, 0, 0, 0]                 # integer s: no band fades
    assert f[5].tolist() == [1.0, 0.5, 0, 0, 0]
    assert f[7].tolist() == [1.0, 1.0, 1.0, 1.0, 0.75]
    assert (F.band_factors(s, 0, 5, 0)[1] == active).all()    # hard cut: f_b = 1 on every band that runs
    assert F.band_factors(s, 3, 0, 1)[0].shape == (9, 0)


@pytest.mark.parametrize("nb,first,fade", F.CASES, ids=F.CASE_IDS)
@pytest.mark.parametrize("n", [128, 6])
def test_host_evaluator_matches_ref64(host, tiles, n, nb, first, fade):
    coef, w = tiles[n], F.weights(nb, first)
    pts = F.points(first, nb, 1200, 40 + nb + first)
    s = F.footprints(first, nb, len(pts), 50 + nb + first)
    got, val = F.host_footprint(host, coef, pts, None, s, first, nb, w, VAR, fade)
    assert (bits(got[:, 0]) == bits(val)).all()               # the gradient form's value has the value form's bits
    want, _ = F.multiband_footprint_points(coef, pts, None, s, first, nb, w, VAR, fade)
    err = np.abs(got.astype(np.float64) - want)
    tol = F.tolerance(s, first, nb, w, VAR)
    assert (err <= tol[:, None]).all(), (err.max(0), tol.max())
    none = F.active_count(s, first, nb) == 0
    assert none.any() and (got[none] == 0.0).all()            # no active band (NaN and +inf among them): 0 in every channel
    if nb:
        assert (F.active_count(s, first, nb) == nb).any() and np.isneginf(s).any()


@pytest.mark.parametrize("nb,first,fade", F.CASES, ids=F.CASE_IDS)
def test_host_evaluator_projected_matches_ref64(host, tiles, nb, first, fade):
    n = 6 if (nb + first + fade) % 2 else 128
    coef, w = tiles[n], F.weights(nb, first)
    pts = F.points(first, nb, 240, 60 + nb + first)
    s = F.footprints(first, nb, len(pts), 70 + nb + first)
    nrs = F.normals(len(pts), 80 + nb)
    got, val = F.host_footprint(host, coef, pts, nrs, s, first, nb, w, VAR_PROJ, fade)
    assert (bits(got[:, 0]) == bits(val)).all()
    want, bound = F.multiband_footprint_points(coef, pts, nrs, s, first, nb, w, VAR_PROJ, fade)
    err = np.abs(got.astype(np.float64) - want)
    assert (err <= bound).all(), (err / np.maximum(bound, 1e-300)).max(0)
    assert (got[F.active_count(s, first, nb) == 0] == 0.0).all()


@pytest.mark.parametrize("fade", [0, 1])
def test_zero_weights_and_empty_tile_give_zero(host, tiles, fade):
    pts = F.points(0, 5, 300, 3)
    s = F.footprints(0, 5, len(pts), 4)
    nrs = F.normals(len(pts), 5)
    for normals in (None, nrs):
        got, val = F.host_footprint(host, tiles[128], pts, normals, s, 0, 5, [0.0] * 5, VAR, fade)
        assert (got == 0.0).all() and (val == 0.0).all()     # the sum of w^2 is 0: no division either
        got, val = F.host_footprint(host, None, pts, normals, s, 0, 5, F.W8, VAR, fade)
        assert (got == 0.0).all() and (val == 0.0).all()
    grey = F.host_texture(host, None, 2.0, pts, s, 0, 5, F.W8, VAR, fade)
    assert (grey == 0.5).all()


@pytest.mark.parametrize("fade", [0, 1])
def test_host_texture_is_the_composition(host, tiles, fade):
    """wnhost_wavelet_multiband_texture_value: the evaluator at (float)((double)p * scale), through the grey level."""
    scale, first, nb = 3.7, 0, 5
    w = F.weights(nb, first)
    pts = np.random.default_rng(6).uniform(-20.0, 20.0, (600, 3)).astype(np.float32)
    s = F.footprints(first, nb, len(pts), 7)
    pos = (pts.astype(np.float64) * scale).astype(np.float32)
    _, val = F.host_footprint(host, tiles[128], pos, None, s, first, nb, w, VAR, fade)
    grey = F.host_texture(host, tiles[128], scale, pts, s, first, nb, w, VAR, fade)
    assert (bits(grey) == bits(F.texture_grey(val))).all()
    assert grey.min() >= 0.0 and grey.max() <= 1.0 and np.ptp(grey) > 0.2


def test_footprint_header_symbols_all_exported_and_bound():
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(PKG, "libwnoise_hip.so")):
        ge.build()
    capi = importlib.import_module("wavelet-noise-in-ray-tracing_amd._capi")
    lib = capi.load()
    text = open(os.path.join(ROOT, "include", "wnoise_footprint.h")).read()
    names = sorted(set(re.findall(r"WN_API\s+[\w\s\*]+?\b(wn_\w+)\s*\(", text)))
    assert len(names) == 5, names
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/wnoise_footprint.h but not exported"
    assert set(capi.FOOTPRINT_SIGNATURES) == set(names)
