"""A float64 reference for the analytic gradients of evaluate2D and evaluate3DProjected (and its WMultibandNoise
composition), with the conventions of tests/_ref64.py and tests/_ref64_grad.py.

evaluate2D: the coordinates, pm = p - 0.5f and mid = ceilf(pm) are float32 (they decide which coefficients a sample
reads); the weights (t^2/2, 3/4 - (t - 1/2)^2, (1 - t)^2/2), their derivatives (-t, 2t - 1, 1 - t) and every sum are
float64.  Returned arrays carry three channels: value, d/dx, d/dy.

evaluate3DProjected: the point and the normal are float32 inputs; everything after that is float64.  A cell c has
t_i = (c_i + n_i dot / 2) - (p_i - 1.5), dot = sum_k n_k (p_k - c_k), weight prod_i B(t_i) and, with
G_i = B'(t_i) prod_{k!=i} B(t_k) and S = sum_i n_i G_i, d weight / dp_j = (n_j / 2) S - G_j.  The cells are those of the
support box (3|n_a| + 3 sqrt((1 - n_a^2) / 2) around p_a) with one cell of margin on each side; a cell counts when
0 < t < 3 on all three axes.  The value channel applies the reference's weight > 1e-6 cut (as _ref64.projected_points);
the gradient never does.  Returned arrays carry four channels: value, d/dx, d/dy, d/dz.

A plain helper module (not a conftest): the tests import it by name.
"""
import numpy as np

import _ref64
import _ref64_grad

f32 = np.float32


# ---- evaluate2D ------------------------------------------------------------------------------------------------------------
def evaluate2d_grad_points(coef, pts):
    """evaluate2D and its gradient at every (x, y) of an (N, 2) float32 list: (N, 3) float64.  An empty tile gives 0."""
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    if coef is None or np.asarray(coef).size == 0:
        return np.zeros((pts.shape[0], 3))
    n, c = _ref64._tile2d(coef)
    taps = np.arange(-1, 2)
    (mx, wx, dx), (my, wy, dy) = (_ref64_grad.spline_axis_grad(pts[:, a]) for a in range(2))
    ix, iy = (mx[:, None] + taps) % n, (my[:, None] + taps) % n
    g = c[iy[:, :, None], ix[:, None, :]]                    # [N, 3 (y), 3 (x)]
    out = np.empty((pts.shape[0], 3))
    for ch, (ay, ax) in enumerate(((wy, wx), (wy, dx), (dy, wx))):
        out[:, ch] = np.einsum("nj,ni,nji->n", ay, ax, g)
    return out


def evaluate2d_lattice_grad(coef, px, py):
    """evaluate2D and its gradient at every (px[x], py[y]): array [3, len(py), len(px)] (y contracted first, then x)."""
    if coef is None or np.asarray(coef).size == 0:
        return np.zeros((3, np.size(py), np.size(px)))
    n, c = _ref64._tile2d(coef)
    taps = np.arange(-1, 2)
    (mx, wx, dx), (my, wy, dy) = _ref64_grad.spline_axis_grad(px), _ref64_grad.spline_axis_grad(py)
    ix, iy = (mx[:, None] + taps) % n, (my[:, None] + taps) % n
    a = np.einsum("yj,yjx->yx", wy, c[iy])                   # collapse y with the weights ...
    b = np.einsum("yj,yjx->yx", dy, c[iy])                   # ... and with the derivatives
    return np.stack([np.einsum("xi,yxi->yx", wx, a[:, ix]),
                     np.einsum("xi,yxi->yx", dx, a[:, ix]),
                     np.einsum("xi,yxi->yx", wx, b[:, ix])])


INV_STDDEV_2D = 1.0 / np.sqrt(np.float64(f32(0.19686)))


def wavelet2d_gradient_image(coef, den, nx, ny, octave):
    """The lattice of wavelet2d_gradient_image: evaluate2D(((i/den)*4)*2^octave*2) and its gradient with respect to that
    coordinate, all three times 1/sqrt(0.19686f): [3, ny, nx]."""
    oscale = f32(2.0 ** octave)
    px = _ref64.lattice_coords(np.arange(nx), den, 4.0, oscale, 2.0)
    py = _ref64.lattice_coords(np.arange(ny), den, 4.0, oscale, 2.0)
    return evaluate2d_lattice_grad(coef, px, py) * INV_STDDEV_2D


# Bound on |float32 - float64| of every channel of the 2-D gradient: the 9-tap sums of _ref64_grad.tolerance.
TOL_2D = 1e-5


# ---- evaluate3DProjected ---------------------------------------------------------------------------------------------------
def _bspline_dt(t):
    """B' of _ref64._bspline_t: t, (2 - t) - (t - 1), -(3 - t) on the three pieces."""
    return np.where(t < 1.0, t, np.where(t < 2.0, (2.0 - t) - (t - 1.0), -(3.0 - t)))


def projected_grad_points(coef, pts, normals, cut_value=True, chunk=1024):
    """evaluate3DProjected and its gradient with respect to p at every point of an (N, 3) float32 list: (N, 4) float64.
    `normals`: one float32 normal per point, or one for the whole list.  cut_value=False drops the 1e-6 cut from the
    value channel too (the function whose gradient the other channels are).  An empty tile gives 0."""
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    nr = np.broadcast_to(np.asarray(normals, np.float32).reshape(-1, 3), pts.shape)
    if coef is None or np.asarray(coef).size == 0:
        return np.zeros((pts.shape[0], 4))
    coef = np.asarray(coef, np.float32)
    n = int(round(coef.size ** (1.0 / 3.0)))
    assert n ** 3 == coef.size, coef.size
    flat = coef.astype(np.float64)
    out = np.empty((pts.shape[0], 4))
    for b in range(0, pts.shape[0], chunk):
        p = pts[b:b + chunk].astype(np.float64)              # [m, 3]
        nv = nr[b:b + chunk].astype(np.float64)
        m = p.shape[0]
        support = 3.0 * np.abs(nv) + 3.0 * np.sqrt((1.0 - nv * nv) / 2.0)
        lo = np.ceil(p - support).astype(np.int64) - 1
        hi = np.floor(p + support).astype(np.int64) + 1
        k = [np.arange(int((hi[:, a] - lo[:, a]).max()) + 1) for a in range(3)]
        cells = (lo[:, 0, None, None, None] + k[0][None, None, None, :],
                 lo[:, 1, None, None, None] + k[1][None, None, :, None],
                 lo[:, 2, None, None, None] + k[2][None, :, None, None])
        inside = (cells[0] <= hi[:, 0, None, None, None]) & (cells[1] <= hi[:, 1, None, None, None]) & \
                 (cells[2] <= hi[:, 2, None, None, None])
        P = [p[:, a, None, None, None] for a in range(3)]
        N = [nv[:, a, None, None, None] for a in range(3)]
        dot = sum(N[a] * (P[a] - cells[a]) for a in range(3))
        B, D = [], []
        for a in range(3):
            t = (cells[a] + N[a] * dot / 2.0) - (P[a] - 1.5)
            inside &= (t > 0.0) & (t < 3.0)
            tc = np.clip(t, 0.0, 3.0)
            B.append(_ref64._bspline_t(tc))
            D.append(_bspline_dt(tc))
        weight = B[0] * B[1] * B[2]
        G = [D[0] * B[1] * B[2], B[0] * D[1] * B[2], B[0] * B[1] * D[2]]
        S = N[0] * G[0] + N[1] * G[1] + N[2] * G[2]
        idx = (cells[0] % n) + (cells[1] % n) * n + (cells[2] % n) * (n * n)
        c = np.where(inside, flat[idx], 0.0)
        keep = (weight > 1e-6) if cut_value else True
        out[b:b + chunk, 0] = np.where(keep, weight * c, 0.0).reshape(m, -1).sum(1)
        for j in range(3):
            out[b:b + chunk, 1 + j] = ((N[j] / 2.0 * S - G[j]) * c).reshape(m, -1).sum(1)
    return out


def multiband_projected_grad_points(coef, pts, normals, s, first_band, nbands, w, var_per_band):
    """WMultibandNoise (normal != NULL) and its gradient with respect to p: band b adds w_b * evaluate3DProjected(q_b)
    and w_b * 2 * 2^(first_band+b) * its gradient, q_b = 2 * p * 2^(first_band+b).  Returns ((N, 4) float64, the
    per-point bound of every channel)."""
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    wv = np.asarray(w, np.float32)[:nbands].astype(np.float64)
    out = np.zeros((pts.shape[0], 4))
    bound = np.zeros((pts.shape[0], 4))
    for b in range(_ref64_grad.active_bands(s, first_band, nbands)):
        bs = f32(2.0 ** (first_band + b))                    # powers of two: the float32 products are exact
        q = (f32(2) * pts) * bs
        e = projected_grad_points(coef, q, normals)
        out[:, 0] += wv[b] * e[:, 0]
        out[:, 1:] += wv[b] * 2.0 * float(bs) * e[:, 1:]
        bound[:, 0] += abs(wv[b]) * _ref64.projected_bound(q)
        bound[:, 1:] += (abs(wv[b]) * 2.0 * float(bs) * projected_grad_bound(q))[:, None]
    d = _ref64_grad.out_div(w, nbands, var_per_band)
    return out / d, bound / d


# Measured |float32 - float64| of the three gradient channels of wnhost_eval3d_projected_grad (the bits of the point
# kernel) over tiles 128 and 6, 40,000 points per set (uniform in [-4, 4]^3, [-300, 300]^3 and [-1e4, 1e4]^3, and the
# edge points of _ref64.edge_points) with the normals of _ref64.normal_set, per point: at most 2.2e-6 where |p| <= 4,
# and at most 4e-6 + 6.6 * ulp32(max_a |p_a|) everywhere (the float32 rounding of t, about one ulp of |p|, times B'' of
# the cells).  PROJ_GRAD_A = 4e-6 and PROJ_GRAD_B = 10 cover that with room.
PROJ_GRAD_A, PROJ_GRAD_B = 4e-6, 10.0


def projected_grad_bound(pts):
    """Per-point bound on |gradient(float32) - projected_grad_points| (unscaled: multiply by |out_scale|)."""
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    return PROJ_GRAD_A + PROJ_GRAD_B * _ref64.ulp32(np.abs(pts).max(1))


def projected_bounds(pts):
    """(N, 4): the value channel's bound (_ref64.projected_bound) and the gradient channels' (projected_grad_bound)."""
    v = _ref64.projected_bound(pts)
    g = projected_grad_bound(pts)
    return np.stack([v, g, g, g], axis=1)


INV_STDDEV_PROJ = 1.0 / np.sqrt(np.float64(f32(0.296)))
