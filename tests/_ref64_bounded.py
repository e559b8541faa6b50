"""A float64 reference for curl noise with solid boundaries (include/wnoise_bounded.h), built on tests/_ref64_curl.py and
tests/_ref64.py: the positions and the obstacles' fields are the float32 values the library receives, every distance,
ramp, product and sum is float64.

    v = A (curl Psi) + G x Psi,   A = prod_j alpha(d_j / d0_j) over the obstacles with d_j < d0_j,   G = grad A

A point with some d_j <= 0 is inside (v = 0), a point with every d_j >= d0_j is far (A = 1, G = 0).  An obstacle is the
tuple of tests/_bounded.py.  A plain helper module (not a conftest): the tests import it by name.
"""
import numpy as np

import _ref64_curl
import _ref64_grad

FAR, NEAR, INSIDE = 0, 1, 2
EPS = 2.0 ** -24


def _fields(obstacle):
    kind, c, r, d0 = obstacle
    return kind, np.asarray(c, np.float32).astype(np.float64), float(np.float32(r)), float(np.float32(d0))


def distance(obstacle, x):
    """d (N,), its gradient nrm (N, 3), and the magnitude scale (N,) that the float32 rounding of d is relative to:
    max(l, r) for the sphere kinds, sum |n_c x_c| + |o| for a half-space."""
    kind, c, r, _ = _fields(obstacle)
    x = np.asarray(x, np.float32).astype(np.float64)
    if kind == "halfspace":
        return x @ c - r, np.broadcast_to(c, x.shape), np.abs(x) @ np.abs(c) + abs(r)
    dx = x - c
    ln = np.sqrt((dx * dx).sum(1))
    with np.errstate(divide="ignore", invalid="ignore"):
        m = np.where(ln[:, None] == 0.0, 0.0, dx / ln[:, None])
    scale = np.maximum(ln, r)
    return (ln - r, m, scale) if kind == "sphere" else (r - ln, -m, scale)


def ramp(obstacles, x, rounding=False):
    """where (N,), A (N,), G (N, 3).  rounding=True: also dA (N,) and dG (N,), bounds on the error of a float32 evaluation of
    A and of every component of G (the derivation is in tests/test_bounded_host.py)."""
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
    Ar, G = np.ones(n), np.zeros((n, 3))
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


def potential_values(coef, pts, offsets):
    """(N, 3) float64: evaluate3D of the three rolled tiles."""
    return np.stack([_ref64_grad.evaluate3d_grad_points(t, pts)[:, 0] for t in _ref64_curl.rolled_tiles(coef, offsets)], axis=1)


def parts(coef, pts, offsets, obstacles, rounding=False):
    """where, A, G (, dA, dG), the unbounded curl c and the potential values Psi at the points."""
    return (*ramp(obstacles, pts, rounding), _ref64_curl.evaluate3d_curl_points(coef, pts, offsets),
            potential_values(coef, pts, offsets))


def velocity(where, Ar, G, c, psi):
    v = Ar[:, None] * c + np.cross(G, psi)
    v[where == INSIDE] = 0.0
    return v


def evaluate3d_curl_bounded_points(coef, pts, offsets, obstacles):
    return velocity(*parts(coef, pts, offsets, obstacles))
