"""A long-double restatement of the curl of three Perlin potentials (include/wnoise_perlin_curl.h), independent of the
product's code and in a DIFFERENT order of operations: the expanded corner weights of tests/_ref64_perlin_grad.py (whose
fade, dfade, GVEC and corner_hashes it uses) where the product lerps axis by axis.

psi_k is noise / the signed turb sum / fractal_noise with the INTEGER CELL shifted by the whole-cell offset o_k: the hashes
are corner_hashes(perm, cell + o_k), everything else is the unshifted point's.  v = (d psi2/dy - d psi1/dz,
d psi0/dz - d psi2/dx, d psi1/dx - d psi0/dy).

Every function takes its points in the dtype it is asked to compute in (default np.longdouble), so that difference
quotients can be taken at points that are not float32 or float64 numbers.

A plain helper module (not a conftest): the tests import it by name.
"""
import numpy as np

import _ref64_perlin_grad as G

LD = np.longdouble

DEFAULT_OFFSETS = ((0, 0, 0), (85, 85, 85), (170, 170, 170))


def noise_jacobian(perm, pts, offsets, dtype=LD):
    """The gradients of the three shifted noise potentials at every row of pts: [N, 3 (potential), 3 (axis)]."""
    p = np.asarray(pts, dtype).reshape(-1, 3)
    off = np.asarray(offsets, np.int64).reshape(3, 3)
    fl = np.floor(p)
    f = p - fl
    cell = fl.astype(np.int64)
    u, du = G.fade(f), G.dfade(f)
    w = np.stack([1 - u, u], axis=-1)                           # [N, axis, corner]
    dw = np.stack([-du, du], axis=-1)
    corner = np.array([0, 1], dtype)
    d = f[:, :, None] - corner[None, None, :]                   # f - c per axis and corner
    wx, wy, wz = w[:, 0][:, None, None, :], w[:, 1][:, None, :, None], w[:, 2][:, :, None, None]
    dwx, dwy, dwz = dw[:, 0][:, None, None, :], dw[:, 1][:, None, :, None], dw[:, 2][:, :, None, None]
    W = wx * wy * wz
    out = np.empty((len(p), 3, 3), dtype)
    for k in range(3):
        h = G.corner_hashes(perm, cell + off[k][None, :]) & 15
        gv = G.GVEC.astype(dtype)[h]                            # [N, cz, cy, cx, 3]
        a = (gv[..., 0] * d[:, 0][:, None, None, :] + gv[..., 1] * d[:, 1][:, None, :, None]
             + gv[..., 2] * d[:, 2][:, :, None, None])
        out[:, k, 0] = (W * gv[..., 0] + dwx * wy * wz * a).sum(axis=(1, 2, 3))
        out[:, k, 1] = (W * gv[..., 1] + wx * dwy * wz * a).sum(axis=(1, 2, 3))
        out[:, k, 2] = (W * gv[..., 2] + wx * wy * dwz * a).sum(axis=(1, 2, 3))
    return out


def jacobian(perm, kind, pts, depth=0, offsets=DEFAULT_OFFSETS, dtype=LD):
    """[N, 3, 3] of d psi_k / d axis for `kind` in "noise", "turb" (the signed sum of `depth` octaves), "fractal".
    For float32 points 2^i p is the float doubling the product does."""
    p = np.asarray(pts, dtype).reshape(-1, 3)
    if kind == "noise":
        return noise_jacobian(perm, p, offsets, dtype)
    J = np.zeros((len(p), 3, 3), dtype)
    if kind == "turb":
        for i in range(depth):
            scale = dtype(2.0) ** i
            J += noise_jacobian(perm, p * scale, offsets, dtype) * ((1 / scale) * scale)
        return J
    amplitude, frequency, max_value = dtype(1), dtype(1), dtype(0)
    for _ in range(6):
        J += noise_jacobian(perm, p * frequency, offsets, dtype) * (amplitude * frequency)
        max_value += amplitude
        amplitude = amplitude / 2
        frequency = frequency * 2
    return J / max_value


def curl_of(J):
    return np.stack([J[:, 2, 1] - J[:, 1, 2], J[:, 0, 2] - J[:, 2, 0], J[:, 1, 0] - J[:, 0, 1]], axis=-1)


def velocity(perm, kind, pts, depth=0, offsets=DEFAULT_OFFSETS, dtype=LD):
    """v at every row of pts: [N, 3] in `dtype`."""
    return curl_of(jacobian(perm, kind, pts, depth, offsets, dtype))


def bound(kind, depth=0):
    """A component is the difference of two gradient channels, each within the project's Perlin tolerance of 1e-12 per
    octave summed."""
    return 2 * G.bound(kind, depth)
