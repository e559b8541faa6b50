"""The float64 references (tests/_ref64.py) against the oracle's float32 operations.

The GPU tests check the kernels against _ref64; this checks _ref64 itself, on the tiles, lattices and band sets those
tests use (power-of-two and odd tiles, negative planes, divisions that are not exact, 1..8 bands, `s` cut-offs, unequal
weights), and at the edge coordinates and normals of _ref64.edge_coords / normal_set.  Measured max |oracle - ref64|
(the oracle's float32 rounding):
  * evaluate3D: 9.1e-7 for single-band lattices, 1.2e-6 for band sums on lattices, 2.5e-6 for band sums at random
    points whose band coordinates reach 160; bound REF64_TOL = 4e-6.
  * evaluate2D: 2.5e-7 at points and on lattices, edge coordinates included; bound REF64_TOL.
  * evaluate3DProjected: per point, 8.4e-7 where |p| <= 4 and 1.1e-6 + 3.9 ulp32(max |p_a|) everywhere; bound
    _ref64.projected_bound = 1.5e-6 + 5 ulp32(max |p_a|) (summed over the bands for WMultibandNoise).
  * tile generation: 2.3e-7 * max |field| (Gaussian, impulse, constant and mixed-magnitude fields); bound
    TILE_REL = 4e-7 times max |field|.
"""
import numpy as np
import pytest

import _ref64

REF64_TOL = 4e-6
TILE_REL = 4e-7

TILES = ("tile3d_128", "tile3d_32", "tile3d_8_7", "tile3d_16_12345", "tile3d_5odd_11")


@pytest.fixture(scope="module")
def tiles(ora, gold, tile3d_128):
    t = {key: gold[key] for key in TILES[2:]}
    t["tile3d_128"] = tile3d_128
    t["tile3d_32"] = ora.tile3d(32, 77)
    return t


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("den,nx,ny,z0,z1,octave", [
    (512, 512, 9, 3, 7, 4),
    (1000, 333, 5, -4, 3, 4),          # negative planes, inexact division
    (449, 260, 7, 100, 104, 4),
    (2048, 2000, 4, 1000, 1003, 4),
    (384, 256, 5, 0, 3, 5),            # step 2/3
])
def test_ref64_single_band_vs_oracle(ora, tiles, tile, den, nx, ny, z0, z1, octave):
    coef = tiles[tile]
    want = ora.grid_wavelet3d_volume(coef, den, nx, ny, z0, z1, octave).astype(np.float64)
    got = _ref64.wavelet_volume(coef, den, nx, ny, z0, z1, octave)
    assert got.shape == want.shape
    err = float(np.abs(got - want).max())
    assert err <= REF64_TOL, err
    # the comparison discriminates: the neighbouring planes are far off
    shifted = _ref64.wavelet_volume(coef, den, nx, ny, z0 + 1, z1 + 1, octave)
    assert float(np.abs(shifted - want).max()) > 1e-2


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("den,nx,ny,z0,z1,s,first,nb,w", [
    (512, 512, 9, 3, 7, -16.0, 0, 5, [1.0, 0.5, 2.0, 1.0, 0.25]),
    (4096, 500, 5, 0, 3, -16.0, 0, 8, [1.0] * 8),
    (1000, 300, 6, -3, 2, -3.0, 0, 5, [1.0] * 5),                     # s stops after 3 bands, variance over 5
    (2048, 257, 4, 9, 12, -16.0, -2, 7, [0.3, 1.0, 2.0, 1.0, 0.7, 1.0, 1.0]),
    (512, 200, 3, 0, 2, -16.0, 0, 6, [1.0] * 6),
    (960, 128, 3, 5, 7, -1.0, 0, 3, [1.0, 2.0, 3.0]),                 # one active band
])
def test_ref64_multiband_vs_oracle(ora, tiles, tile, den, nx, ny, z0, z1, s, first, nb, w):
    coef = tiles[tile]
    want = ora.grid_multiband3d_volume(coef, den, nx, ny, z0, z1, s, first, nb, w, 0.18402).astype(np.float64)
    got = _ref64.multiband_volume(coef, den, nx, ny, z0, z1, s, first, nb, w, 0.18402)
    assert got.shape == want.shape
    err = float(np.abs(got - want).max())
    assert err <= REF64_TOL, err


def test_ref64_points_vs_oracle(ora, tile3d_128):
    rng = np.random.default_rng(3)
    pts = rng.uniform(-40.0, 40.0, (200, 3)).astype(np.float32)
    for nb in (1, 5, 8):
        w = rng.uniform(0.2, 2.0, nb).astype(np.float32)
        want = ora.multiband3d(tile3d_128, pts, -16.0, -3, nb, w, 0.18402).astype(np.float64)
        got = _ref64.multiband_points(tile3d_128, pts, -16.0, -3, nb, w, 0.18402)
        assert float(np.abs(got - want).max()) <= REF64_TOL, nb


# ---- evaluate2D ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiles2d(ora, gold, tile2d_128):
    return {"t128": tile2d_128, "t16": gold["tile2d_16_99"], "t2": ora.tile2d(2, 5), "t6": ora.tile2d(6, 21),
            "t130": ora.tile2d(130, 8)}


@pytest.mark.parametrize("tile", ("t128", "t16", "t2", "t6", "t130"))
def test_ref64_evaluate2d_points_vs_oracle(ora, tiles2d, tile):
    coef = tiles2d[tile]
    rng = np.random.default_rng(11)
    pts = np.concatenate([_ref64.edge_points(2, 3000, 7), rng.uniform(-300.0, 300.0, (1000, 2))]).astype(np.float32)
    want = ora.evaluate2d(coef, pts).astype(np.float64)
    got = _ref64.evaluate2d_points(coef, pts)
    err = float(np.abs(got - want).max())
    assert err <= REF64_TOL, err
    assert float(np.abs(_ref64.evaluate2d_points(coef, pts + np.float32(1)) - want).max()) > 1e-2


@pytest.mark.parametrize("tile", ("t128", "t6", "t130"))
@pytest.mark.parametrize("den,nx,ny,rng_,oscale,post", [
    (512, 512, 9, 4.0, 16.0, 2.0),
    (1000, 333, 17, 4.0, 8.0, 2.0),       # inexact division
    (7, 40, 3, 3.0, 1.0, 0.5),
    (96, 5, 200, 4.0, 32.0, 2.0),         # nx < ny
])
def test_ref64_evaluate2d_lattice_vs_oracle(ora, tiles2d, tile, den, nx, ny, rng_, oscale, post):
    coef = tiles2d[tile]
    px = _ref64.lattice_coords(np.arange(nx), den, rng_, oscale, post)
    py = _ref64.lattice_coords(np.arange(ny), den, rng_, oscale, post)
    yy, xx = np.meshgrid(py, px, indexing="ij")
    want = ora.evaluate2d(coef, np.stack([xx.ravel(), yy.ravel()], 1)).reshape(ny, nx).astype(np.float64)
    got = _ref64.evaluate2d_lattice(coef, px, py)
    err = float(np.abs(got - want).max())
    assert err <= REF64_TOL, err


def test_ref64_spline_just_above_negative_powers_of_two(ora, tiles2d, tile3d_128):
    """p = -2^k + u, u in [0, 0.5): p - 0.5f rounds into the next binade; the weights must follow the rounded pm."""
    k = np.arange(0, 21)
    u = np.array([0.001, 0.1, 0.25, 0.4, 0.4999], np.float32)
    p = (np.float32(-1) * np.float32(2.0) ** k.astype(np.float32))[:, None] + u[None, :]
    p = p.astype(np.float32).ravel()
    q = np.roll(p, 7)
    pts2 = np.stack([p, q], 1)
    err = float(np.abs(_ref64.evaluate2d_points(tiles2d["t128"], pts2) - ora.evaluate2d(tiles2d["t128"], pts2)).max())
    assert err <= REF64_TOL, err
    want = ora.evaluate3d(tile3d_128, np.stack([p, q, np.roll(p, 3)], 1)).astype(np.float64)
    got = np.array([_ref64.evaluate_lattice(tile3d_128, a[0:1], a[1:2], a[2:3])[0, 0, 0]
                    for a in np.stack([p, q, np.roll(p, 3)], 1)])
    err = float(np.abs(got - want).max())
    assert err <= REF64_TOL, err
    assert float(np.abs(_ref64.evaluate3d_points(tile3d_128, np.stack([p, q, np.roll(p, 3)], 1)) - got).max()) <= 1e-12


# ---- evaluate3DProjected -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiles3d(ora, gold, tile3d_128):
    return {"t128": tile3d_128, "t16": gold["tile3d_16_12345"], "t2": ora.tile3d(2, 3), "t6": ora.tile3d(6, 4),
            "t130": ora.tile3d(130, 9)}


@pytest.mark.parametrize("tile", ("t128", "t16", "t2", "t6", "t130"))
def test_ref64_projected_vs_oracle(ora, tiles3d, tile):
    coef = tiles3d[tile]
    normals = _ref64.normal_set()
    rng = np.random.default_rng(13)
    for i, nr in enumerate(normals):
        pts = np.concatenate([_ref64.edge_points(3, 160, 100 + i), rng.uniform(-300.0, 300.0, (40, 3)),
                              rng.uniform(-4.0, 4.0, (40, 3))]).astype(np.float32)
        want = ora.evaluate3d_projected(coef, pts, nr).astype(np.float64)
        got = _ref64.projected_points(coef, pts, nr)
        err = np.abs(got - want)
        bound = _ref64.projected_bound(pts)
        worst = int(np.argmax(err - bound))
        assert err[worst] <= bound[worst], (nr.tolist(), pts[worst].tolist(), float(err[worst]), float(bound[worst]))
    # one normal per point gives the same as the normals one at a time
    pts = rng.uniform(-20.0, 20.0, (normals.shape[0], 3)).astype(np.float32)
    per = _ref64.projected_points(coef, pts, normals)
    one = np.array([_ref64.projected_points(coef, p[None], nr)[0] for p, nr in zip(pts, normals)])
    assert float(np.abs(per - one).max()) <= 1e-12          # the same cells; only the float64 summation order differs
    assert float(np.abs(per - ora.evaluate3d_projected(coef, pts, normals)).max()) <= float(
        _ref64.projected_bound(pts).min())


@pytest.mark.parametrize("s,first,nb,w", [
    (-16.0, -2, 5, [1.0, 0.5, 2.0, 1.0, 0.25]),
    (-3.0, 0, 5, [1.0] * 5),                                          # s stops after 3 bands, variance over 5
    (-16.0, -4, 8, [0.3, 1.0, 2.0, 1.0, 0.7, 1.0, 1.0, 0.5]),
    (-1.0, 0, 3, [1.0, 2.0, 3.0]),                                     # one active band
])
def test_ref64_multiband_projected_vs_oracle(ora, tiles3d, s, first, nb, w):
    coef = tiles3d["t128"]
    rng = np.random.default_rng(17)
    pts = np.concatenate([rng.uniform(-30.0, 30.0, (60, 3)), _ref64.edge_points(3, 60, 3)]).astype(np.float32)
    pts = pts[np.abs(pts).max(1) <= 2.0 ** 12]
    normals = _ref64.normal_set(4)[:: 2]
    for nr in normals:
        want = ora.multiband3d_projected(coef, pts, nr, s, first, nb, w, 0.296).astype(np.float64)
        got, bound = _ref64.multiband_projected_points(coef, pts, nr, s, first, nb, w, 0.296)
        err = np.abs(got - want)
        worst = int(np.argmax(err - bound))
        assert err[worst] <= bound[worst], (nr.tolist(), pts[worst].tolist(), float(err[worst]), float(bound[worst]))
    per_point = np.resize(normals, (pts.shape[0], 3))
    want = ora.multiband3d_projected(coef, pts, per_point, s, first, nb, w, 0.296).astype(np.float64)
    got, bound = _ref64.multiband_projected_points(coef, pts, per_point, s, first, nb, w, 0.296)
    assert (np.abs(got - want) <= bound).all()


# ---- tile generation -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,dims", [(2, 3), (6, 3), (16, 3), (128, 3), (130, 3), (2, 2), (6, 2), (130, 2), (258, 2),
                                    (1024, 2)])
def test_ref64_tile_vs_oracle(ora, n, dims):
    for name, field in _ref64.tile_fields(n, dims, n + dims).items():
        if n >= 128 and dims == 3 and name not in ("gauss", "mixed"):
            continue
        want = ora.filter_tile(field, n, dims).astype(np.float64)
        got = _ref64.tile(field, n, dims)
        err = float(np.abs(got - want).max())
        assert err <= TILE_REL * float(np.abs(field).max()), (name, err)
        planes = [0, n // 2, n - 1]
        sub = _ref64.tile(field, n, dims, planes)
        assert float(np.abs(sub - got.reshape((n,) * dims)[planes].ravel()).max()) <= 1e-12 * float(np.abs(field).max())
