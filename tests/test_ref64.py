"""The float64 lattice reference (tests/_ref64.py) against the oracle's float32 evaluate3D / WMultibandNoise.

The GPU tests check whole lattices of the fast dense-grid kernels against _ref64; this checks _ref64 itself, on
the tiles, lattices and band sets those tests use (power-of-two and odd tiles, negative planes, divisions that are
not exact, 1..8 bands, `s` cut-offs, unequal weights).  Measured max |oracle - ref64| over these cases (the oracle's
float32 rounding): 9.1e-7 for single-band lattices, 1.2e-6 for band sums on lattices, 2.5e-6 for band sums at random
points whose band coordinates reach 160; bound 4e-6.
"""
import numpy as np
import pytest

import _ref64

REF64_TOL = 4e-6

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
