"""A float64 reference for curl noise: the curl of the vector potential (psi0, psi1, psi2) whose component k is evaluate3D
(or its WMultibandNoise composition) of the tile rolled by the whole-cell offset o_k = (ox, oy, oz)_k,

    T_k = np.roll(c3, shift=(-oz, -oy, -ox), axis=(0, 1, 2))        T_k[z][y][x] = C[z+oz][y+oy][x+ox] (mod n)
    v   = (d psi2/dy - d psi1/dz,  d psi0/dz - d psi2/dx,  d psi1/dx - d psi0/dy)

built on tests/_ref64_grad.py applied to the rolled tiles (its conventions: float32 coordinates and mids, float64 weights,
derivatives and sums).  A plain helper module (not a conftest): the tests import it by name.
"""
import numpy as np

import _ref64_grad


def default_offsets(n):
    """The library's default: (0, 0, 0), (n//3,)*3, (2*n//3,)*3."""
    return ((0, 0, 0), (n // 3,) * 3, (2 * n // 3,) * 3)


def tile_size(coef):
    coef = np.asarray(coef)
    n = int(round(coef.size ** (1.0 / 3.0))) if coef.size else 0
    assert n ** 3 == coef.size, coef.size
    return n


def rolled(coef, offset):
    """The tile T with T[z][y][x] = C[z+oz][y+oy][x+ox] (mod n), flat float32, x fastest; offset = (ox, oy, oz)."""
    coef = np.asarray(coef, np.float32)
    if coef.size == 0:
        return coef
    n = tile_size(coef)
    ox, oy, oz = (int(v) for v in offset)
    return np.ascontiguousarray(np.roll(coef.reshape(n, n, n), shift=(-oz, -oy, -ox), axis=(0, 1, 2))).ravel()


def rolled_tiles(coef, offsets):
    return [rolled(coef, o) for o in np.asarray(offsets, np.int64).reshape(3, 3)]


def curl_of(g0, g1, g2, axis):
    """The curl from the three potentials' {value, d/dx, d/dy, d/dz} arrays, whose channels lie along `axis`."""
    d = lambda g, ch: np.take(g, ch, axis=axis)   # noqa: E731
    return np.stack([d(g2, 2) - d(g1, 3), d(g0, 3) - d(g2, 1), d(g1, 1) - d(g0, 2)], axis=axis)


def evaluate3d_curl_points(coef, pts, offsets):
    """(N, 3) float64; an empty tile gives 0."""
    return curl_of(*[_ref64_grad.evaluate3d_grad_points(t, pts) for t in rolled_tiles(coef, offsets)], axis=1)


def evaluate_lattice_curl(coef, px, py, pz, offsets):
    """[3, len(pz), len(py), len(px)] float64 on the lattice px x py x pz."""
    return curl_of(*[_ref64_grad.evaluate_lattice_grad(t, px, py, pz) for t in rolled_tiles(coef, offsets)], axis=0)


def multiband_curl_points(coef, pts, offsets, s, first_band, nbands, w, var_per_band):
    return curl_of(*[_ref64_grad.multiband_grad_points(t, pts, s, first_band, nbands, w, var_per_band)
                     for t in rolled_tiles(coef, offsets)], axis=1)


def multiband_lattice_curl(coef, px, py, pz, offsets, s, first_band, nbands, w, var_per_band):
    return curl_of(*[_ref64_grad.multiband_lattice_grad(t, px, py, pz, s, first_band, nbands, w, var_per_band)
                     for t in rolled_tiles(coef, offsets)], axis=0)


def tolerance(out_scale=1.0, multiband=None):
    """2 G: a component is the difference of two gradient channels that each carry _ref64_grad.tolerance's bound G."""
    return 2.0 * _ref64_grad.tolerance(out_scale, multiband)
