"""A float64 reference for the wavelet-noise operations, evaluated independently of any HIP code: evaluate3D on dense
lattices (oracle/wn_oracle.c wno_evaluate3d) and its WMultibandNoise composition (wno_multiband3d), evaluate2D on
points and lattices (wno_evaluate2d), evaluate3DProjected on points (wno_evaluate3d_projected) and its WMultibandNoise
composition (wno_multiband3d_projected), and the filter half of tile generation (wno_filter_tile2d/3d).

What stays float32 is what decides WHICH coefficients a sample reads: the lattice coordinate, computed as
lattice_coord does it (((float)i / den) * range, then * octave_scale, then * post_scale), pm = p - 0.5f and the
B-spline mid, ceilf(pm).  The spline weights, the tap sums, the band sum and the 1/sqrt(variance * var_per_band)
normalisation are float64.  A lattice is axis-aligned, so the 27-tap sum is contracted one axis at a time
(z, then y, then x): a few million samples take about a second.

evaluate3DProjected takes its coordinates and normal as float32 inputs; everything after that (support box, dot
product, t, weights, the 1e-6 weight test) is float64.  The oracle forms dot and t in float32 from p, so the two part by
about one float32 ulp of |p| (see projected_bound).  Tile generation is the product of two float64 matrices per axis.

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
    """Mids and float64 weights of the three taps of each coordinate.  pm = p - 0.5f and mid = ceilf(pm) are float32,
    as in bspline / bspline_axis: just above -2^k, p - 0.5f leaves p's binade and rounds, and t is taken from that pm."""
    p = np.asarray(p, np.float32)
    pm = p - f32(0.5)
    mid = np.ceil(pm).astype(np.int64)
    t = mid.astype(np.float64) - pm.astype(np.float64)
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


def evaluate3d_points(coef, pts):
    """evaluate3D at every point of an (N, 3) float32 list, in float64 (27 taps, indices wrapped modulo n)."""
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    if coef is None or np.asarray(coef).size == 0:
        return np.zeros(pts.shape[0])
    coef = np.asarray(coef, np.float32)
    n = int(round(coef.size ** (1.0 / 3.0)))
    assert n ** 3 == coef.size, coef.size
    c = coef.reshape(n, n, n).astype(np.float64)
    taps = np.arange(-1, 2)
    (mx, wx), (my, wy), (mz, wz) = (spline_axis(pts[:, a]) for a in range(3))
    ix, iy, iz = (mx[:, None] + taps) % n, (my[:, None] + taps) % n, (mz[:, None] + taps) % n
    g = c[iz[:, :, None, None], iy[:, None, :, None], ix[:, None, None, :]]   # [N, 3 (z), 3 (y), 3 (x)]
    return np.einsum("nk,nj,ni,nkji->n", wz, wy, wx, g)


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


# ---- evaluate2D --------------------------------------------------------------------------------------------------------
def _tile2d(coef):
    coef = np.asarray(coef, np.float32)
    n = int(round(coef.size ** 0.5))
    assert n * n == coef.size, coef.size
    return n, coef.reshape(n, n).astype(np.float64)         # [y][x]


def evaluate2d_points(coef, pts):
    """evaluate2D at every (x, y) of an (N, 2) float32 list, in float64 (3 x 3 taps, indices wrapped modulo n)."""
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    if coef is None or np.asarray(coef).size == 0:
        return np.zeros(pts.shape[0])
    n, c = _tile2d(coef)
    (mx, wx), (my, wy) = spline_axis(pts[:, 0]), spline_axis(pts[:, 1])
    taps = np.arange(-1, 2)
    ix, iy = (mx[:, None] + taps) % n, (my[:, None] + taps) % n
    g = c[iy[:, :, None], ix[:, None, :]]                    # [N, 3 (y), 3 (x)]
    return np.einsum("nj,ni,nji->n", wy, wx, g)


def evaluate2d_lattice(coef, px, py):
    """evaluate2D at every (px[x], py[y]) in float64: array [len(py), len(px)] (y contracted first, then x)."""
    if coef is None or np.asarray(coef).size == 0:
        return np.zeros((np.size(py), np.size(px)))
    n, c = _tile2d(coef)
    taps = np.arange(-1, 2)
    (mx, wx), (my, wy) = spline_axis(px), spline_axis(py)
    ix, iy = (mx[:, None] + taps) % n, (my[:, None] + taps) % n
    a = np.einsum("yj,yjx->yx", wy, c[iy])                   # collapse y: [ny, n]
    return np.einsum("xi,yxi->yx", wx, a[:, ix])             # ... x: [ny, nx]


# ---- evaluate3DProjected -------------------------------------------------------------------------------------------------
def _bspline_t(t):
    """The quadratic B-spline of WaveletNoise.cpp:243-255 at t in (0, 3), float64."""
    return np.where(t < 1.0, t * t / 2.0,
                    np.where(t < 2.0, 1.0 - ((t - 1.0) ** 2 + (2.0 - t) ** 2) / 2.0, (3.0 - t) ** 2 / 2.0))


def projected_points(coef, pts, normals, chunk=2048):
    """evaluate3DProjected at every point of an (N, 3) float32 list, in float64.  `normals`: one float32 normal per
    point, or one for the whole list.  Every cell of the support box (3|n_a| + 3 sqrt((1 - n_a^2) / 2) around p_a, in
    float64, one cell of margin on each side) with 0 < t_a < 3 on all three axes and weight > 1e-6 contributes; indices
    wrap modulo n."""
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    nr = np.broadcast_to(np.asarray(normals, np.float32).reshape(-1, 3), pts.shape)
    if coef is None or np.asarray(coef).size == 0:
        return np.zeros(pts.shape[0])
    coef = np.asarray(coef, np.float32)
    n = int(round(coef.size ** (1.0 / 3.0)))
    assert n ** 3 == coef.size, coef.size
    flat = coef.astype(np.float64)
    out = np.empty(pts.shape[0])
    for b in range(0, pts.shape[0], chunk):
        p = pts[b:b + chunk].astype(np.float64)              # [m, 3]
        nv = nr[b:b + chunk].astype(np.float64)
        support = 3.0 * np.abs(nv) + 3.0 * np.sqrt((1.0 - nv * nv) / 2.0)
        lo = np.ceil(p - support).astype(np.int64) - 1
        hi = np.floor(p + support).astype(np.int64) + 1
        k = [np.arange(int((hi[:, a] - lo[:, a]).max()) + 1) for a in range(3)]
        # cells [m, kz, ky, kx] per axis, broadcast
        cx = lo[:, 0, None, None, None] + k[0][None, None, None, :]
        cy = lo[:, 1, None, None, None] + k[1][None, None, :, None]
        cz = lo[:, 2, None, None, None] + k[2][None, :, None, None]
        inside = (cx <= hi[:, 0, None, None, None]) & (cy <= hi[:, 1, None, None, None]) & \
                 (cz <= hi[:, 2, None, None, None])
        cells = (cx, cy, cz)
        dot = sum(nv[:, a, None, None, None] * (p[:, a, None, None, None] - cells[a]) for a in range(3))
        weight = np.ones(dot.shape)
        for a in range(3):
            t = (cells[a] + nv[:, a, None, None, None] * dot / 2.0) - (p[:, a, None, None, None] - 1.5)
            inside &= (t > 0.0) & (t < 3.0)
            weight = weight * _bspline_t(np.clip(t, 0.0, 3.0))
        keep = inside & (weight > 1e-6)
        idx = (cx % n) + (cy % n) * n + (cz % n) * (n * n)
        out[b:b + chunk] = np.where(keep, weight * flat[idx], 0.0).reshape(p.shape[0], -1).sum(1)
    return out


def ulp32(x):
    """The float32 spacing at |x| (elementwise)."""
    return np.spacing(np.abs(np.asarray(x, np.float32))).astype(np.float64)


# Measured |oracle - float64| of evaluate3DProjected over the coordinates and normals of tests/test_ref64.py, per
# point: at most 8.4e-7 where |p| <= 4, and at most 1.1e-6 + 3.9 * ulp32(max_a |p_a|) everywhere (the largest
# multiples at coordinates just past -2^k, where p - 1.5f rounds to the next binade's ulp; random points up to |p| = 2^20
# stay under 1.8 ulp).  PROJ_A and PROJ_B are those values rounded up.
PROJ_A, PROJ_B = 1.5e-6, 5.0


def projected_bound(pts):
    """Per-point bound on |evaluate3DProjected(float32) - projected_points| (unscaled: multiply by |out_scale|)."""
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    return PROJ_A + PROJ_B * ulp32(np.abs(pts).max(1))


def multiband_projected_points(coef, pts, normals, s, first_band, nbands, w, var_per_band):
    """WMultibandNoise, normal != NULL branch (oracle wno_multiband3d_projected): bands b run while
    s + first_band + b < 0, band b is evaluate3DProjected(2 * p * 2^(first_band + b), normal), the variance sums all
    nbands weights.  Returns (value, per-point bound) in float64."""
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    w = np.asarray(w, np.float32)[:nbands].astype(np.float64)
    out = np.zeros(pts.shape[0])
    bound = np.zeros(pts.shape[0])
    for b in range(nbands):
        if not float(f32(s) + f32(first_band) + f32(b)) < 0.0:
            break
        bs = f32(2.0 ** (first_band + b))                    # powers of two: the float32 products are exact
        q = (f32(2) * pts) * bs
        out += w[b] * projected_points(coef, q, normals)
        bound += abs(w[b]) * projected_bound(q)
    variance = float(np.sum(w * w))
    if variance != 0.0:
        d = np.sqrt(variance * float(f32(var_per_band)))
        out /= d
        bound /= d
    return out, bound


# ---- tile generation -----------------------------------------------------------------------------------------------------
ANALYSIS = np.array([
    0.000334, -0.001528, 0.000410, 0.003545, -0.000938, -0.008233, 0.002172, 0.019120,
    -0.005040, -0.044412, 0.011655, 0.103311, -0.025936, -0.243780, 0.033979, 0.655340,
    0.655340, 0.033979, -0.243780, -0.025936, 0.103311, 0.011655, -0.044412, -0.005040,
    0.019120, 0.002172, -0.008233, -0.000938, 0.003546, 0.000410, -0.001528, 0.000334], np.float32)  # Appendix 1
SYNTHESIS = np.array([0.25, 0.75, 0.75, 0.25], np.float32)


def lowpass_matrix(n):
    """U @ D in float64: D (n/2 x n) is the 32-tap analysis filter, to[i] = sum_{k=-16}^{15} a[k] from[(2i + k) mod n];
    U (n x n/2) the 4-tap synthesis filter, to[i] = sum_{k = i/2, i/2 + 1; -2 <= i - 2k <= 1} s[i - 2k] from[k mod n/2].
    Taps that wrap onto the same sample add up."""
    half = n // 2
    D = np.zeros((half, n))
    for i in range(half):
        for k in range(-16, 16):
            D[i, (2 * i + k) % n] += float(ANALYSIS[16 + k])
    U = np.zeros((n, half))
    for i in range(n):
        for k in (i // 2, i // 2 + 1):
            tap = i - 2 * k
            if -2 <= tap <= 1:
                U[i, k % half] += float(SYNTHESIS[2 + tap])
    return U @ D


def tile(field, n, dims, planes=None):
    """The filter half of generateNoiseTile2D/3D in float64: field - lowpass(field), the lowpass applied along x, then
    y (then z), as the reference's passes run.  n^dims values, x fastest.  With `planes` (indices along the slowest
    axis: z, or y in 2-D) only those planes are formed, the slowest axis's rows of U @ D applied first (the passes are
    linear and commute; only float64 rounding differs): array [len(planes), ...] flattened."""
    f = np.asarray(field, np.float32).astype(np.float64).reshape((n,) * dims)   # [(z,) y, x]
    M = lowpass_matrix(n)
    if planes is not None:
        planes = np.asarray(planes)
        low = np.tensordot(M[planes], f, axes=([1], [0]))
        for axis in range(dims - 1, 0, -1):
            low = np.moveaxis(np.tensordot(M, low, axes=([1], [axis])), 0, axis)
        return (f[planes] - low).ravel()
    low = f
    for axis in range(dims - 1, -1, -1):                     # x is the last array axis
        low = np.moveaxis(np.tensordot(M, low, axes=([1], [axis])), 0, axis)
    return (f - low).ravel()


def tile_fields(n, dims, seed):
    """Fields for the filter: Gaussian, an impulse in the last corner and one inside, a constant, and mixed
    magnitudes (x1e4 and x1e-4 interleaved)."""
    rng = np.random.default_rng(seed)
    size = n ** dims
    gauss = rng.normal(size=size).astype(np.float32)
    corner = np.zeros(size, np.float32)
    corner[-1] = 1.0
    inside = np.zeros(size, np.float32)
    inside[(size // 2 + n // 3) % size] = -2.5
    const = np.full(size, 0.75, np.float32)
    mixed = gauss * np.where(np.arange(size) % 2 == 0, np.float32(1e4), np.float32(1e-4)).astype(np.float32)
    return {"gauss": gauss, "corner": corner, "inside": inside, "const": const, "mixed": mixed}


# ---- inputs at the edges, shared by tests/test_ref64.py and the GPU tests --------------------------------------------------
def edge_coords():
    """float32 coordinates where the float32 arithmetic is most delicate: exact half-integers (mid = ceilf(p - 0.5f)
    flips there), p just above -2^k for k <= 20 (p - 0.5f leaves p's binade and rounds), +-0.0, tiny magnitudes, and
    magnitudes up to 2^20."""
    v = [0.0, -0.0, 1e-30, -1e-30, 0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 63.5, 127.5, -127.5, 129.5, 1000.5, -4095.5,
         2.0 ** 20, -(2.0 ** 20), 2.0 ** 20 - 0.5, -(2.0 ** 20) + 0.5, 2.0 ** 19 + 0.25, -(2.0 ** 19) - 0.25]
    for k in range(21):
        base = f32(-(2.0 ** k))
        v.append(np.nextafter(base, f32(0)))
        v += [base + f32(u) for u in (0.001, 0.1, 0.25, 0.375, 0.4999)]
    return np.array(v, np.float32)


def edge_points(dims, count, seed):
    """`count` points whose coordinates are drawn from edge_coords(), every coordinate on its own."""
    return np.random.default_rng(seed).choice(edge_coords(), (count, dims)).astype(np.float32)


def normal_set(n_random=8, seed=5):
    """Unit normals (float32): the six axis normals, (1, 1, 1)/sqrt(3) and a sign variant, near-axis normals, normals
    with a -0.0 component, and `n_random` random unit normals."""
    s3, s2 = 1.0 / np.sqrt(3.0), 1.0 / np.sqrt(2.0)
    fixed = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (s3, s3, s3), (-s3, s3, -s3),
             (s2, s2, 0), (0.0, -0.0, 1.0), (-0.0, 1.0, -0.0)]
    near = np.array([(1.0, 1e-4, 0.0), (1e-3, -1e-3, 1.0), (-1e-4, 1.0, 1e-4)])
    r = np.random.default_rng(seed).normal(size=(n_random, 3))
    out = np.concatenate([np.array(fixed, np.float64), near / np.linalg.norm(near, axis=1, keepdims=True),
                          r / np.linalg.norm(r, axis=1, keepdims=True)])
    return out.astype(np.float32)
