"""A float64 reference for dense 3-D wavelet-noise lattices: WaveletNoise::evaluate3D (oracle/wn_oracle.c
wno_evaluate3d) and its WMultibandNoise composition (wno_multiband3d), evaluated independently of any HIP code.

What stays float32 is what decides WHICH coefficients a sample reads: the lattice coordinate, computed as
lattice_coord does it (((float)i / den) * range, then * octave_scale, then * post_scale), and the B-spline mid,
ceilf(p - 0.5f).  The spline weights, the 27-tap sum, the band sum and the 1/sqrt(variance * var_per_band)
normalisation are float64.  A lattice is axis-aligned, so the 27-tap sum is contracted one axis at a time
(z, then y, then x): a few million samples take about a second.

A plain helper module (not a conftest): the tests import it by name.
"""
import numpy as np

f32 = np.float32


def lattice_coords(idx, den, base_range=4.0, octave_scale=1.0, post_scale=1.0):
    """float32 coordinates of lattice indices, in lattice_coord's order of operations."""
    i = np.asarray(idx, np.float32)
    c = (i / f32(den)) * f32(base_range)
    c = c * f32(octave_scale)
    return c * f32(post_scale)


def spline_axis(p):
    """Mids (float32 arithmetic, as bspline / bspline_axis) and float64 weights of the three taps of each coordinate."""
    p = np.asarray(p, np.float32)
    mid = np.ceil(p - f32(0.5)).astype(np.int64)
    t = mid.astype(np.float64) - (p.astype(np.float64) - 0.5)
    w = np.stack([t * t / 2.0, 0.75 - (t - 0.5) ** 2, (1.0 - t) ** 2 / 2.0], axis=-1)
    return mid, w


def evaluate_lattice(coef, px, py, pz):
    """evaluate3D at every (px[x], py[y], pz[z]) in float64: array [len(pz), len(py), len(px)].
    coef is the tile's n^3 float32 coefficients, x fastest (any n, the wrap is a modulo)."""
    coef = np.asarray(coef, np.float32)
    n = int(round(coef.size ** (1.0 / 3.0)))
    assert n ** 3 == coef.size, coef.size
    c = coef.reshape(n, n, n).astype(np.float64)           # [z][y][x]
    taps = np.arange(-1, 2)
    (mx, wx), (my, wy), (mz, wz) = spline_axis(px), spline_axis(py), spline_axis(pz)
    ix, iy, iz = (mx[:, None] + taps) % n, (my[:, None] + taps) % n, (mz[:, None] + taps) % n
    a = np.einsum("zk,zkyx->zyx", wz, c[iz])                # collapse z: [nz, n, n]
    a = np.einsum("yj,zyjx->zyx", wy, a[:, iy])             # ... y: [nz, ny, n]
    return np.einsum("xi,zyxi->zyx", wx, a[:, :, ix])       # ... x: [nz, ny, nx]


def wavelet_volume(coef, den, nx, ny, z0, z1, octave):
    """The lattice of oracle.grid_wavelet3d_volume / wavelet_volume: evaluate3D(((i/den)*4)*2^octave*2) / sqrt(0.18402f)."""
    oscale = f32(2.0 ** octave)
    px = lattice_coords(np.arange(nx), den, 4.0, oscale, 2.0)
    py = lattice_coords(np.arange(ny), den, 4.0, oscale, 2.0)
    pz = lattice_coords(np.arange(z0, z1), den, 4.0, oscale, 2.0)
    return evaluate_lattice(coef, px, py, pz) / np.sqrt(np.float64(f32(0.18402)))


def multiband_lattice(coef, px, py, pz, s, first_band, nbands, w, var_per_band):
    """WMultibandNoise (Cook & DeRose Appendix 2) on the lattice px x py x pz: bands b run while
    s + first_band + b < 0, band b is evaluate3D(2 * p * 2^(first_band + b)), the variance sums all nbands weights."""
    w = np.asarray(w, np.float32)[:nbands].astype(np.float64)
    px, py, pz = (np.asarray(p, np.float32) for p in (px, py, pz))
    out = np.zeros((pz.size, py.size, px.size))
    for b in range(nbands):
        if not float(f32(s) + f32(first_band) + f32(b)) < 0.0:
            break
        bs = f32(2.0 ** (first_band + b))                    # powers of two: the float32 products are exact
        out += w[b] * evaluate_lattice(coef, (f32(2) * px) * bs, (f32(2) * py) * bs, (f32(2) * pz) * bs)
    variance = float(np.sum(w * w))
    if variance != 0.0:
        out /= np.sqrt(variance * float(f32(var_per_band)))
    return out


def multiband_volume(coef, den, nx, ny, z0, z1, s, first_band, nbands, w, var_per_band):
    """The lattice of oracle.grid_multiband3d_volume / multiband_volume: p = (i/den)*4 on all three axes."""
    px, py, pz = (lattice_coords(np.arange(a, b), den) for a, b in ((0, nx), (0, ny), (z0, z1)))
    return multiband_lattice(coef, px, py, pz, s, first_band, nbands, w, var_per_band)


def multiband_points(coef, pts, s, first_band, nbands, w, var_per_band):
    """WMultibandNoise at arbitrary points (a list of 1 x 1 x 1 lattices, for small lists)."""
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    return np.array([multiband_lattice(coef, p[0:1], p[1:2], p[2:3], s, first_band, nbands, w, var_per_band)[0, 0, 0]
                     for p in pts])
