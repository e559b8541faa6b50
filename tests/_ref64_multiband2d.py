"""A float64 reference for WMultibandNoise on a 2-D tile (include/wnoise_multiband2d.h), built on the band logic of
tests/_ref64_footprint.py and the per-band reference of tests/_ref64_grad_surface.py (evaluate2D and its gradient), with the
error bound of the float32 evaluator and the inputs that the CPU and GPU tests of that feature share.

What stays float32 is what decides WHICH coefficients and bands a sample reads: t_b = (s + first_band) + b, f_b =
min(1, -t_b), the band coordinate q_b = (2 * p) * 2^(first_band+b) (exact: powers of two), pm = q - 0.5f and mid =
ceilf(pm).  The weights, the product w_b * f_b, the band sums and the division are float64.

The bound (tolerance()).  u = 2^-24, C = max |coefficient|.  Per axis t = mid - pm is exact in float32, so:
  w0 = fl(fl(t t) / 2): one rounding, |dw0| <= u/2;  w2 = fl(fl(a a) / 2), a = fl(1 - t): |dw2| <= 3u/2;
  w1 = fl(fl(1 - w0) - w2): the two inherited errors and two roundings of numbers <= 1, |dw1| <= 4u;  sum |dw| <= 6u;
  d0 = -t exact, d1 = fl(2t - 1), d2 = fl(1 - t): sum |dd| <= 2u;  sum w = 1, sum |d| <= 2.
evaluate2D = sum over 9 taps of fl(fl(wx wy) c), accumulated from 0 (8 roundings of partial sums <= C):
  value:    12u (weights) + 2u (the two products) + 8u (sums)                   = 22 u C
  gradient: 2u + 2 * 6u (d and w) + 2u * 2 (products, sum |d w| <= 2) + 8u * 2  = 34 u C, and |grad| <= 2C.
WMultibandNoise: wb = fl(w_b f_b) (u), a term fl(wb e_b) (u), k - 1 <= nbands - 1 roundings of the band sum, and the
division by out_div = sqrtf(fl(sum fl(w w)) * var), itself within (nbands + 1.5) u of the float64 one, rounding once more:
  value    <= sum_b |w_b f_b| / out_div                     * C u (22 +     (2 + 2 nbands + 1.5)) <= K_v C u (26 + 2 nbands)
  gradient <= sum_b |w_b f_b| 2^(first_band+b+1) / out_div  * C u (34 + 2 * (2 + 2 nbands + 1.5)) <= K_g C u (41 + 4 nbands)
The scaling of wb by 2 * 2^(first_band+b) is exact.  These are first-order bounds; GUARD covers the second-order terms.
Below the smallest normal float32 a product rounds to a multiple of 2^-149 whatever its size (f_b reaches 2^-149 one
step under a band's threshold), so the bound has an absolute floor proportional to _ref64_footprint.F32_TINY.

A plain helper module (not a conftest): the tests import it by name.
"""
import ctypes as C

import numpy as np

import _ref64
import _ref64_footprint as F
import _ref64_grad
import _ref64_grad_surface

f32 = np.float32
FP = C.POINTER(C.c_float)
U = 2.0 ** -24
GUARD = 1.01
VAR_2D = 0.19686                                            # experient/main.cpp:16, texture.h:98

# the (nbands, first_band, fade) cases of _ref64_footprint, which include eight bands from first_band -2
CASES = list(F.CASES) + [c for c in ((8, -2, 0), (8, -2, 1)) if c not in F.CASES]
CASE_IDS = [f"nb{nb}_first{first}_{'fade' if fade else 'hard'}" for nb, first, fade in CASES]


def tile2d(n, seed=12345):
    """An n x n tile filtered in float64 from a Gaussian field, as float32 coefficients (x fastest)."""
    return _ref64.tile(_ref64.tile_fields(n, 2, seed)["gauss"], n, 2).astype(np.float32)


def multiband2d_footprint_points(coef, pts, s, first_band, nbands, w, var_per_band, fade):
    """WMultibandNoise with evaluate2D bands and footprint s[i] at point i, and its gradient with respect to p:
    (N, 3) float64 of {value, d/dx, d/dy}.  s: one footprint per point, or a scalar for all."""
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    s = np.broadcast_to(np.asarray(s, np.float32).reshape(-1), (pts.shape[0],))
    wv = np.asarray(w, np.float32)[:nbands].astype(np.float64)
    active, f = F.band_factors(s, first_band, nbands, fade)
    out = np.zeros((pts.shape[0], 3))
    for b in range(nbands):
        m = active[:, b]
        if not m.any():
            break
        bs = f32(2.0 ** (first_band + b))                    # powers of two: the float32 products are exact
        e = _ref64_grad_surface.evaluate2d_grad_points(coef, (f32(2) * pts[m]) * bs)
        wb = wv[b] * f[m, b]
        out[m, 0] += wb * e[:, 0]
        out[m, 1:] += (wb * 2.0 * float(bs))[:, None] * e[:, 1:]
    return out / _ref64_grad.out_div(w, nbands, var_per_band)


def tolerance(coef, s, first_band, nbands, w, var_per_band, fade, count=None):
    """The (N, 3) per-point bound of the module docstring on |float32 evaluator - multiband2d_footprint_points|."""
    s = np.asarray(s, np.float32).reshape(-1)
    if count is not None:
        s = np.broadcast_to(s, (count,))
    cmax = float(np.abs(np.asarray(coef, np.float64)).max()) if coef is not None and np.size(coef) else 0.0
    wv = np.abs(np.asarray(w, np.float32)[:nbands].astype(np.float64))
    _, f = F.band_factors(s, first_band, nbands, fade)       # 0 where the band does not run
    div = _ref64_grad.out_div(w, nbands, var_per_band)
    chain = 2.0 ** (first_band + np.arange(nbands) + 1.0)
    k_v = (f * wv[None, :]).sum(1) / div
    k_g = (f * (wv * chain)[None, :]).sum(1) / div
    floor = F.F32_TINY * (1.0 + cmax) * (1.0 + nbands / div) * (1.0 + (chain.max() if nbands else 0.0))
    tol_v = GUARD * k_v * cmax * U * (26 + 2 * nbands) + floor
    tol_g = GUARD * k_g * cmax * U * (41 + 4 * nbands) + floor
    return np.stack([tol_v, tol_g, tol_g], axis=1)


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def points(first_band, nbands, count, seed):
    """(count, 2) float32 points: half edge points (_ref64.edge_points), half uniform ones in [-300, 300]^2 and
    [-4, 4]^2, with |q_b| < 2^24 on every band: the finest band evaluates at p * 2^(first_band + nbands), and past 2^24
    a float32 coordinate has no fraction left to interpolate with."""
    rng = np.random.default_rng(seed)
    half = count // 2
    edges = _ref64.edge_points(2, 16 * half, seed + 1)
    limit = 2.0 ** 24 / 2.0 ** (first_band + max(nbands, 1))
    edges = edges[np.abs(edges).max(1) < limit][:half]
    assert edges.shape[0] == half, edges.shape
    rest = count - half
    uniform = np.concatenate([rng.uniform(-300.0, 300.0, (rest - rest // 4, 2)), rng.uniform(-4.0, 4.0, (rest // 4, 2))])
    pts = np.concatenate([edges, uniform.astype(np.float32)])[rng.permutation(count)].astype(np.float32)
    assert (np.abs(pts).max() * 2.0 ** (first_band + max(nbands, 1))) < 2.0 ** 24
    return pts


footprints = F.footprints
weights = F.weights


def unfaded(s, first_band, nbands, fade):
    """True where every band that runs has f_b == 1: the points whose bits do not depend on `fade`."""
    active, f = F.band_factors(s, first_band, nbands, fade)
    return np.where(active, f == 1.0, True).all(1)


def lattice_points(den, nx, ny, base_range=4.0, octave_scale=1.0, post_scale=1.0):
    """The (ny * nx, 2) float32 lattice coordinates of a wn_grid, x fastest."""
    px = _ref64.lattice_coords(np.arange(nx), den, base_range, octave_scale, post_scale)
    py = _ref64.lattice_coords(np.arange(ny), den, base_range, octave_scale, post_scale)
    return np.stack([np.tile(px, ny), np.repeat(py, nx)], axis=1).astype(np.float32)


# ---- the host evaluator (libwnoise_host.so) --------------------------------------------------------------------------------
def bind_host(lib):
    lib.wnhost_multiband2d_footprint.restype = C.c_float
    lib.wnhost_multiband2d_footprint.argtypes = [FP, C.c_int, FP, C.c_float, C.c_int, C.c_int, C.c_int, FP, C.c_float, FP]
    return lib


def host_multiband2d(lib, coef, pts, s, first_band, nbands, w, var_per_band, fade, value_form=True):
    """wnhost_multiband2d_footprint at every point: ((N, 3) float32 of the gradient form, (N,) float32 of the value form,
    or None with value_form=False).  s: one footprint per point, or a scalar for all."""
    if coef is None or np.asarray(coef).size == 0:
        cp, n, keep = None, 0, None
    else:
        keep = np.ascontiguousarray(coef, np.float32)
        cp, n = keep.ctypes.data_as(FP), int(round(keep.size ** 0.5))
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    s = np.broadcast_to(np.asarray(s, np.float32).reshape(-1), (len(pts),))
    wa = (C.c_float * max(1, nbands))(*[float(x) for x in w[:nbands]])
    out = np.empty((len(pts), 3), np.float32)
    val = np.empty(len(pts), np.float32) if value_form else None
    g = np.empty(2, np.float32)
    gp = g.ctypes.data_as(FP)
    fn = lib.wnhost_multiband2d_footprint
    for i in range(len(pts)):
        p = pts[i].ctypes.data_as(FP)
        out[i, 0] = fn(cp, n, p, s[i], fade, first_band, nbands, wa, var_per_band, gp)
        out[i, 1:] = g
        if value_form:
            val[i] = fn(cp, n, p, s[i], fade, first_band, nbands, wa, var_per_band, None)
    return out, val
