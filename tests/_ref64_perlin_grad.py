"""A float64 / long-double restatement of perlin::noise, RTOW turb and perlin::fractal_noise with their analytic
gradients, evaluated independently of the product's code and in a DIFFERENT order of operations: the product lerps the
corner dot products and corner vectors axis by axis (z, y, then x for the gradient); this module expands the eight
corner weights W_c = wx[cx] * wy[cy] * wz[cz], wx = (1 - u, u), and sums

    value = sum_c W_c a_c,            a_c = G_c . (f - c)
    d/dk  = sum_c W_c G_c[k] + sum_c (dW_c/dk) a_c,     dW_c/dx = (-u', u')[cx] * wy[cy] * wz[cz]

with u = fade(f_x) = f^3 (f (6 f - 15) + 10) and u' = 30 f^2 (f - 1)^2.  Agreement between the two is then evidence and
not a copy.  What decides WHICH cell a point reads (floor, & 255, the permutation look-ups) is integer arithmetic and is
the same anywhere.

Every function takes its points in the dtype it is asked to compute in (default np.longdouble), so that difference
quotients can be taken at points that are not float32 or float64 numbers.

A plain helper module (not a conftest): the tests import it by name.
"""
import numpy as np

LD = np.longdouble

# the project's Perlin tolerance: fp64 against a wider evaluation, absolute, per octave summed
TOL_OCTAVE = 1e-12


def grad_literal(h, x, y, z):
    """grad() of perlin.h:26-31, restated literally."""
    h = h & 15
    u = x if h < 8 else y
    v = y if h < 4 else (x if h in (12, 14) else z)
    return (u if (h & 1) == 0 else -u) + (v if (h & 2) == 0 else -v)


# the corner vector of each of the 16 hashes: grad() at the unit vectors
GVEC = np.array([[grad_literal(h, 1.0, 0.0, 0.0), grad_literal(h, 0.0, 1.0, 0.0), grad_literal(h, 0.0, 0.0, 1.0)]
                 for h in range(16)])


def fade(t):
    return t * t * t * (t * (t * 6 - 15) + 10)


def dfade(t):
    return 30 * t * t * (t - 1) * (t - 1)


def corner_hashes(perm, cell):
    """Hashes of the eight corners of every cell: [N, 2 (cz), 2 (cy), 2 (cx)], perlin.h:55-61."""
    perm = np.asarray(perm, np.int64)
    X, Y, Z = (cell[:, a] & 255 for a in range(3))
    out = np.empty((len(X), 2, 2, 2), np.int64)
    for cx in range(2):
        a = perm[X + cx] + Y
        for cy in range(2):
            b = perm[a + cy] + Z
            for cz in range(2):
                out[:, cz, cy, cx] = perm[b + cz]
    return out


def noise_grad(perm, pts, dtype=LD):
    """noise and its gradient at every row of pts: (value [N], gradient [N, 3]) in `dtype`."""
    p = np.asarray(pts, dtype).reshape(-1, 3)
    fl = np.floor(p)
    f = p - fl
    h = corner_hashes(perm, fl.astype(np.int64)) & 15
    G = GVEC.astype(dtype)[h]                                   # [N, 2, 2, 2, 3]
    u, du = fade(f), dfade(f)
    w = np.stack([1 - u, u], axis=-1)                           # [N, axis, corner]
    dw = np.stack([-du, du], axis=-1)
    corner = np.array([0, 1], dtype)
    d = f[:, :, None] - corner[None, None, :]                   # f - c per axis and corner: [N, axis, 2]
    # a_c = G_c . (f - c)
    a = (G[..., 0] * d[:, 0][:, None, None, :] + G[..., 1] * d[:, 1][:, None, :, None]
         + G[..., 2] * d[:, 2][:, :, None, None])               # [N, cz, cy, cx]
    wx, wy, wz = w[:, 0][:, None, None, :], w[:, 1][:, None, :, None], w[:, 2][:, :, None, None]
    dwx, dwy, dwz = dw[:, 0][:, None, None, :], dw[:, 1][:, None, :, None], dw[:, 2][:, :, None, None]
    W = wx * wy * wz
    value = (W * a).sum(axis=(1, 2, 3))
    grad = np.stack([(W * G[..., 0] + dwx * wy * wz * a).sum(axis=(1, 2, 3)),
                     (W * G[..., 1] + wx * dwy * wz * a).sum(axis=(1, 2, 3)),
                     (W * G[..., 2] + wx * wy * dwz * a).sum(axis=(1, 2, 3))], axis=-1)
    return value, grad


def turb_grad(perm, pts, depth, dtype=LD):
    """turb(p, depth) = |sum_i 2^-i noise(2^i p)| and its gradient sigma * sum_i (2^-i 2^i) grad noise(2^i p):
    (value [N], gradient [N, 3], the signed sum [N]).  For float32 points 2^i p is the float doubling the product does."""
    p = np.asarray(pts, dtype).reshape(-1, 3)
    total = np.zeros(len(p), dtype)
    g = np.zeros((len(p), 3), dtype)
    for i in range(depth):
        scale = dtype(2.0) ** i
        v, gn = noise_grad(perm, p * scale, dtype)
        total += v / scale
        g += gn * ((1 / scale) * scale)
    sigma = np.where(total < 0, dtype(-1), dtype(1))
    return np.abs(total), g * sigma[:, None], total


def fractal_grad(perm, pts, dtype=LD):
    """fractal_noise (perlin.h:75-90) and its gradient sum_i (a_i f_i) grad noise(p f_i) / max_value."""
    p = np.asarray(pts, dtype).reshape(-1, 3)
    total = np.zeros(len(p), dtype)
    g = np.zeros((len(p), 3), dtype)
    amplitude, frequency, max_value = dtype(1), dtype(1), dtype(0)
    for _ in range(6):
        v, gn = noise_grad(perm, p * frequency, dtype)
        total += v * amplitude
        g += gn * (amplitude * frequency)
        max_value += amplitude
        amplitude = amplitude / 2
        frequency = frequency * 2
    return total / max_value, g / max_value


def records(value, grad):
    """(N, 4) float64 records {value, d/dx, d/dy, d/dz}."""
    return np.concatenate([np.asarray(value, LD)[:, None], np.asarray(grad, LD)], axis=1).astype(np.float64)


def eval_records(perm, kind, pts, depth=0):
    """Records of `kind` ("noise", "turb", "fractal") and, for turb, the signed sum (else None)."""
    if kind == "noise":
        v, g = noise_grad(perm, pts)
        return records(v, g), None
    if kind == "turb":
        v, g, s = turb_grad(perm, pts, depth)
        return records(v, g), s.astype(np.float64)
    v, g = fractal_grad(perm, pts)
    return records(v, g), None


def bound(kind, depth=0):
    """TOL_OCTAVE per octave summed."""
    return TOL_OCTAVE * (1 if kind == "noise" else (6 if kind == "fractal" else max(depth, 1)))


def face_points(rng, count, lim=40):
    """float64 points on and next to cell faces, negative coordinates included: every point has at least one coordinate
    at an integer or one or a few ulps / a small step beside it."""
    p = rng.uniform(-lim, lim, (count, 3))
    rows = np.arange(count)
    ax = rng.integers(0, 3, count)
    n = np.rint(p[rows, ax])
    off = rng.choice([0.0, 2.0 ** -30, -2.0 ** -30, 2.0 ** -20, -2.0 ** -20, 2.0 ** -45, -2.0 ** -45], count)
    p[rows, ax] = n + off
    both = rng.random(count) < 0.3            # a second coordinate on a face: edges and lattice points
    ax2 = (ax + 1) % 3
    p[rows[both], ax2[both]] = np.rint(p[rows[both], ax2[both]])
    return p
