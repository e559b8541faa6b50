"""A float64 reference for curl noise on a 2-D tile with solid boundaries and a background stream
(include/wnoise_bounded2d.h), built on tests/_ref64_multiband2d.py: the positions, the obstacles' fields and the stream are
the float32 values the library receives, every distance, ramp, product and sum is float64.

    psi_t = psi + (ux y - uy x),   v = (d(A psi_t)/dy, -d(A psi_t)/dx) = A (gy_t, -gx_t) + psi_t (G_1, -G_0),
    A = prod_j alpha(d_j / d0_j) over the obstacles with d_j < d0_j,   G = grad A   (analytic)

A point with some d_j <= 0 is inside (v = 0), a point with every d_j >= d0_j is far (A = 1, G = 0).  An obstacle is the
tuple of tests/_bounded2d.py.  A plain helper module (not a conftest): the tests import it by name.
"""
import numpy as np

import _ref64_multiband2d as M

FAR, NEAR, INSIDE = 0, 1, 2
EPS = 2.0 ** -24


def _fields(obstacle):
    kind, c, r, d0 = obstacle
    return kind, np.asarray(c, np.float32).astype(np.float64), float(np.float32(r)), float(np.float32(d0))


def distance(obstacle, x):
    """d (N,), its gradient nrm (N, 2), and the magnitude scale (N,) that the float32 rounding of d is relative to:
    max(l, r) for the disc kinds, sum |n_c x_c| + |o| for a half-plane."""
    kind, c, r, _ = _fields(obstacle)
    x = np.asarray(x, np.float32).astype(np.float64)
    if kind == "halfplane":
        return x @ c - r, np.broadcast_to(c, x.shape), np.abs(x) @ np.abs(c) + abs(r)
    dx = x - c
    ln = np.sqrt((dx * dx).sum(1))
    with np.errstate(divide="ignore", invalid="ignore"):
        m = np.where(ln[:, None] == 0.0, 0.0, dx / ln[:, None])
    scale = np.maximum(ln, r)
    return (ln - r, m, scale) if kind == "disc" else (r - ln, -m, scale)


def ramp(obstacles, x, rounding=False):
    """where (N,), A (N,), G (N, 2).  rounding=True: also dA (N,) and dG (N,), bounds on the error of a float32 evaluation of
    A and of every component of G: the derivation of tests/test_bounded_host.py::test_host_twin_against_float64, whose
    distance bound 8 e S covers the two-component sums a fortiori (tests/test_bounded2d_host.py restates it)."""
    x = np.asarray(x, np.float32)
    n = len(x)
    inside, near = np.zeros(n, bool), np.zeros(n, bool)
    alphas, betas, nrms, dal, dbe, norms = [], [], [], [], [], []
    for ob in obstacles:
        d0 = _fields(ob)[3]
        d, nrm, scale = distance(ob, x)
        inside |= d <= 0.0
        act = d < d0
        near |= act
        r = np.where(act, d / d0, 1.0)
        r2 = r * r
        alphas.append(np.where(act, r * (1.875 + r2 * (-1.25 + r2 * 0.375)), 1.0))
        betas.append(np.where(act, 1.875 * (1.0 - r2) ** 2 / d0, 0.0))
        nrms.append(nrm)
        dr = 8.0 * EPS * scale / d0 + EPS
        dal.append(np.where(act, 1.875 * dr + 8.0 * EPS, 0.0))
        dbe.append(np.where(act, (3.0 * dr + 16.0 * EPS) / d0, 0.0))
        norms.append(np.sqrt((nrm * nrm).sum(1)))
    Ar, G = np.ones(n), np.zeros((n, 2))
    for al, be, nrm in zip(alphas, betas, nrms):
        G = G * al[:, None] + (Ar * be)[:, None] * nrm
        Ar = Ar * al
    where = np.where(inside, INSIDE, np.where(near, NEAR, FAR))
    Ar[inside], G[inside] = 0.0, 0.0        # v = 0 there
    if not rounding:
        return where, Ar, G
    total = sum(dal) if obstacles else np.zeros(n)
    count = sum((a > 0).astype(np.float64) for a in dal) if obstacles else np.zeros(n)
    dA = total + 2.0 * EPS * count
    dG = np.zeros(n)
    for be, db, da, nn in zip(betas, dbe, dal, norms):
        dG += db * nn + be * nn * (8.0 * EPS + (total - da) + 4.0 * EPS * count)
    return where, Ar, G, dA, dG


def stream(coef, pts, bands, flow):
    """(N, 3) float64 {psi_t, gx_t, gy_t}: the stream function with the background stream, and its gradient."""
    s, first, nb, w, var = bands
    g = M.multiband2d_footprint_points(coef, pts, np.float32(s), first, nb, w, var, 0)
    if flow is not None:
        x = np.asarray(pts, np.float32).astype(np.float64)
        ux, uy = (float(np.float32(v)) for v in flow)
        g = g + np.stack([ux * x[:, 1] - uy * x[:, 0], np.full(len(x), -uy), np.full(len(x), ux)], axis=1)
    return g


def velocity(where, Ar, G, g):
    v = np.stack([Ar * g[:, 2] + G[:, 1] * g[:, 0], -(Ar * g[:, 1] + G[:, 0] * g[:, 0])], axis=1)
    v[where == INSIDE] = 0.0
    return v


def curl_bounded_points(coef, pts, bands, obstacles, flow):
    return velocity(*ramp(obstacles, pts), stream(coef, pts, bands, flow))


def trace_rk4(coef, pts, bands, obstacles, flow, h, steps):
    """Float64 RK4 through the twin (gain 1, no drift): the positions after every step, (steps + 1, N, 2) float64.  The twin
    evaluates at float32 positions, so a stage point is rounded where it enters the evaluator: 2^-24 relative per stage, far
    below the integrator's own error."""
    def v(q):
        return curl_bounded_points(coef, q.astype(np.float32), bands, obstacles, flow)
    p = np.asarray(pts, np.float64)
    path = [p]
    for _ in range(steps):
        k1 = v(p)
        k2 = v(p + 0.5 * h * k1)
        k3 = v(p + 0.5 * h * k2)
        k4 = v(p + h * k3)
        p = p + (h / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
        path.append(p)
    return np.stack(path)
