"""A float64 reference for the analytic gradient of evaluate3D and of its WMultibandNoise composition, with the conventions
of tests/_ref64.py: the coordinates, pm = p - 0.5f and the B-spline mid = ceilf(pm) are float32 (they decide which
coefficients a sample reads); the weights, their derivatives and every sum are float64.

Per axis t = mid - pm, the weights are (t^2/2, 3/4 - (t - 1/2)^2, (1 - t)^2/2) and, as dt/dp = -1, their derivatives
(-t, 2t - 1, 1 - t).  d/dx contracts x with the derivatives and y, z with the weights, and so on.  Returned arrays carry
four channels: value, d/dx, d/dy, d/dz.

A plain helper module (not a conftest): the tests import it by name.
"""
import numpy as np

import _ref64

f32 = np.float32


def spline_axis_grad(p):
    """Mids, float64 weights and float64 derivatives of the three taps of each coordinate."""
    mid, w = _ref64.spline_axis(p)
    p = np.asarray(p, np.float32)
    t = mid.astype(np.float64) - (p - f32(0.5)).astype(np.float64)
    d = np.stack([-t, 2.0 * t - 1.0, 1.0 - t], axis=-1)
    return mid, w, d


def _tile(coef):
    coef = np.asarray(coef, np.float32)
    n = int(round(coef.size ** (1.0 / 3.0)))
    assert n ** 3 == coef.size, coef.size
    return n, coef.reshape(n, n, n).astype(np.float64)     # [z][y][x]


def evaluate3d_grad_points(coef, pts):
    """evaluate3D and its gradient at every point of an (N, 3) float32 list: (N, 4) float64.  An empty tile gives 0."""
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    if coef is None or np.asarray(coef).size == 0:
        return np.zeros((pts.shape[0], 4))
    n, c = _tile(coef)
    taps = np.arange(-1, 2)
    (mx, wx, dx), (my, wy, dy), (mz, wz, dz) = (spline_axis_grad(pts[:, a]) for a in range(3))
    ix, iy, iz = (mx[:, None] + taps) % n, (my[:, None] + taps) % n, (mz[:, None] + taps) % n
    g = c[iz[:, :, None, None], iy[:, None, :, None], ix[:, None, None, :]]   # [N, 3 (z), 3 (y), 3 (x)]
    out = np.empty((pts.shape[0], 4))
    for ch, (az, ay, ax) in enumerate(((wz, wy, wx), (wz, wy, dx), (wz, dy, wx), (dz, wy, wx))):
        out[:, ch] = np.einsum("nk,nj,ni,nkji->n", az, ay, ax, g)
    return out


def evaluate_lattice_grad(coef, px, py, pz):
    """evaluate3D and its gradient at every (px[x], py[y], pz[z]): array [4, len(pz), len(py), len(px)], contracted one
    axis at a time (z, then y, then x)."""
    n, c = _tile(coef)
    taps = np.arange(-1, 2)
    (mx, wx, dx), (my, wy, dy), (mz, wz, dz) = spline_axis_grad(px), spline_axis_grad(py), spline_axis_grad(pz)
    ix, iy, iz = (mx[:, None] + taps) % n, (my[:, None] + taps) % n, (mz[:, None] + taps) % n
    cz = c[iz]
    zw = np.einsum("zk,zkyx->zyx", wz, cz)                   # collapse z with the weights ...
    zd = np.einsum("zk,zkyx->zyx", dz, cz)                   # ... and with the derivatives
    a = np.einsum("yj,zyjx->zyx", wy, zw[:, iy])             # y: A = wy.Z, B = dy.Z, D = wy.Z'
    b = np.einsum("yj,zyjx->zyx", dy, zw[:, iy])
    d = np.einsum("yj,zyjx->zyx", wy, zd[:, iy])
    return np.stack([np.einsum("xi,zyxi->zyx", wx, a[:, :, ix]),
                     np.einsum("xi,zyxi->zyx", dx, a[:, :, ix]),
                     np.einsum("xi,zyxi->zyx", wx, b[:, :, ix]),
                     np.einsum("xi,zyxi->zyx", wx, d[:, :, ix])])


INV_STDDEV = 1.0 / np.sqrt(np.float64(f32(0.18402)))


def wavelet_gradient_volume(coef, den, nx, ny, z0, z1, octave):
    """The lattice of wavelet_gradient_volume: evaluate3D(((i/den)*4)*2^octave*2) and its gradient with respect to that
    coordinate, all four times 1/sqrt(0.18402f): [4, nz, ny, nx]."""
    oscale = f32(2.0 ** octave)
    px = _ref64.lattice_coords(np.arange(nx), den, 4.0, oscale, 2.0)
    py = _ref64.lattice_coords(np.arange(ny), den, 4.0, oscale, 2.0)
    pz = _ref64.lattice_coords(np.arange(z0, z1), den, 4.0, oscale, 2.0)
    return evaluate_lattice_grad(coef, px, py, pz) * INV_STDDEV


def active_bands(s, first_band, nbands):
    """The bands WMultibandNoise evaluates: b < nbands while s + first_band + b < 0 (float32)."""
    b = 0
    while b < nbands and float(f32(s) + f32(first_band) + f32(b)) < 0.0:
        b += 1
    return b


def out_div(w, nbands, var_per_band):
    """sqrt(sum w^2 * var_per_band) over all nbands weights, or 1 when that sum is 0 (no division)."""
    w = np.asarray(w, np.float32)[:nbands].astype(np.float64)
    variance = float(np.sum(w * w))
    return np.sqrt(variance * float(f32(var_per_band))) if variance != 0.0 else 1.0


def multiband_lattice_grad(coef, px, py, pz, s, first_band, nbands, w, var_per_band):
    """WMultibandNoise and its gradient with respect to p on the lattice px x py x pz: band b adds
    w_b * evaluate3D(q_b) and w_b * 2 * 2^(first_band+b) * grad evaluate3D(q_b), q_b = 2 * p * 2^(first_band+b)."""
    wv = np.asarray(w, np.float32)[:nbands].astype(np.float64)
    px, py, pz = (np.asarray(p, np.float32) for p in (px, py, pz))
    out = np.zeros((4, pz.size, py.size, px.size))
    for b in range(active_bands(s, first_band, nbands)):
        bs = f32(2.0 ** (first_band + b))
        e = evaluate_lattice_grad(coef, (f32(2) * px) * bs, (f32(2) * py) * bs, (f32(2) * pz) * bs)
        out[0] += wv[b] * e[0]
        out[1:] += wv[b] * 2.0 * float(bs) * e[1:]
    return out / out_div(w, nbands, var_per_band)


def multiband_gradient_volume(coef, den, nx, ny, z0, z1, s, first_band, nbands, w, var_per_band):
    """The lattice of multiband_gradient_volume: p = (i/den)*4 on all three axes."""
    px, py, pz = (_ref64.lattice_coords(np.arange(a, b), den) for a, b in ((0, nx), (0, ny), (z0, z1)))
    return multiband_lattice_grad(coef, px, py, pz, s, first_band, nbands, w, var_per_band)


def multiband_grad_points(coef, pts, s, first_band, nbands, w, var_per_band):
    """WMultibandNoise and its gradient at every point of an (N, 3) float32 list: (N, 4) float64."""
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    wv = np.asarray(w, np.float32)[:nbands].astype(np.float64)
    out = np.zeros((pts.shape[0], 4))
    for b in range(active_bands(s, first_band, nbands)):
        bs = f32(2.0 ** (first_band + b))
        e = evaluate3d_grad_points(coef, (f32(2) * pts) * bs)
        out[:, 0] += wv[b] * e[:, 0]
        out[:, 1:] += wv[b] * 2.0 * float(bs) * e[:, 1:]
    return out / out_div(w, nbands, var_per_band)


def tolerance(out_scale=1.0, multiband=None):
    """G: 1e-5 * |out_scale| for one band; multiband = (s, first_band, nbands, w, var_per_band) multiplies by
    sum_b |w_b| * 2^(first_band+b+1) / out_div over the active bands (0 when none is active or every weight is 0)."""
    g = 1e-5 * abs(float(out_scale))
    if multiband is None:
        return g
    s, first_band, nbands, w, var_per_band = multiband
    wv = np.asarray(w, np.float32)[:nbands].astype(np.float64)
    k = sum(abs(wv[b]) * 2.0 ** (first_band + b + 1) for b in range(active_bands(s, first_band, nbands)))
    return g * k / out_div(w, nbands, var_per_band)
