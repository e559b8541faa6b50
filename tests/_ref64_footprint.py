"""A float64 reference for WMultibandNoise with a footprint per sample (include/wnoise_footprint.h), built on the per-band
references of tests/_ref64_grad.py (evaluate3D and its gradient) and tests/_ref64_grad_surface.py (evaluate3DProjected and
its gradient), and the inputs the CPU and GPU tests of that feature share.

What stays float32 is what decides WHICH bands a sample evaluates and with which fade: t_b = (s + first_band) + b and
f_b = min(1, -t_b) are formed in float32, in the evaluator's association (f_b is exact: a negation and a comparison).  The
product w_b * f_b, the band sums and the division are float64.

A plain helper module (not a conftest): the tests import it by name.
"""
import ctypes as C

import numpy as np

import _ref64
import _ref64_grad
import _ref64_grad_surface

f32 = np.float32
FP = C.POINTER(C.c_float)

W8 = [1.0, 0.5, 2.0, 1.0, 0.25, 1.5, 0.75, 1.0]   # unequal weights
NBANDS = (0, 1, 5, 8)
FIRST_BANDS = (-2, 0, 3)
CASES = [(nb, first, fade) for nb in NBANDS for first in FIRST_BANDS for fade in (0, 1)]
CASE_IDS = [f"nb{nb}_first{first}_{'fade' if fade else 'hard'}" for nb, first, fade in CASES]


def weights(nb, first):
    return [W8[(b + nb + first) % 8] for b in range(nb)]


# ---- the bands of a sample -----------------------------------------------------------------------------------------------
def band_t(s, first_band, nbands):
    """t_b = (s + first_band) + b in float32: (N, nbands)."""
    s = np.asarray(s, np.float32).reshape(-1)
    with np.errstate(invalid="ignore"):
        base = s + f32(first_band)
        return base[:, None] + np.arange(nbands, dtype=np.float32)[None, :]


def band_factors(s, first_band, nbands, fade):
    """(active, f): (N, nbands) booleans -- band b runs iff t_b < 0 and every earlier band runs -- and the float64 factors
    f_b (1 without fade, min(1, -t_b) with it; 0 where the band does not run)."""
    t = band_t(s, first_band, nbands)
    with np.errstate(invalid="ignore"):
        active = np.logical_and.accumulate(t < 0, axis=1) if nbands else np.zeros(t.shape, bool)
        f = np.minimum(f32(1), -t) if fade else np.ones_like(t)
    return active, np.where(active, f, 0).astype(np.float64)


def active_count(s, first_band, nbands):
    return band_factors(s, first_band, nbands, 0)[0].sum(1)


def multiband_footprint_points(coef, pts, normals, s, first_band, nbands, w, var_per_band, fade):
    """WMultibandNoise with footprint s[i] at point i, and its gradient with respect to p: ((N, 4) float64, bound).
    normals None: bands are evaluate3D and bound is None (the tests use tolerance()); else evaluate3DProjected with one
    normal per point or one for all, and bound is the (N, 4) per-point bound that
    _ref64_grad_surface.multiband_projected_grad_points forms, with the faded weights, plus F32_TINY."""
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    wv = np.asarray(w, np.float32)[:nbands].astype(np.float64)
    active, f = band_factors(s, first_band, nbands, fade)
    out = np.zeros((pts.shape[0], 4))
    bound = None if normals is None else np.zeros((pts.shape[0], 4))
    if normals is not None:
        normals = np.broadcast_to(np.asarray(normals, np.float32).reshape(-1, 3), pts.shape)
    for b in range(nbands):
        m = active[:, b]
        if not m.any():
            break
        bs = f32(2.0 ** (first_band + b))                    # powers of two: the float32 products are exact
        q = (f32(2) * pts[m]) * bs
        wb = wv[b] * f[m, b]
        if normals is None:
            e = _ref64_grad.evaluate3d_grad_points(coef, q)
        else:
            e = _ref64_grad_surface.projected_grad_points(coef, q, normals[m])
            bound[m, 0] += np.abs(wb) * _ref64.projected_bound(q)
            bound[m, 1:] += (np.abs(wb) * 2.0 * float(bs) * _ref64_grad_surface.projected_grad_bound(q))[:, None]
        out[m, 0] += wb * e[:, 0]
        out[m, 1:] += (wb * 2.0 * float(bs))[:, None] * e[:, 1:]
    d = _ref64_grad.out_div(w, nbands, var_per_band)
    return out / d, (None if bound is None else bound / d + F32_TINY)


# The projected bound scales with the faded weight w_b f_b, and f_b reaches the subnormals (s one float32 step under a
# threshold: f_b = 2^-149).  A float32 product in the subnormal range is rounded to a multiple of 2^-149 whatever its size, so
# below the smallest normal float32 has no relative precision to scale: the bound gets that number as an absolute floor.
F32_TINY = 2.0 ** -126


def tolerance(s, first_band, nbands, w, var_per_band):
    """_ref64_grad.tolerance(1.0, (s_i, first_band, nbands, w, var_per_band)) per point (it depends on s_i through the
    number of bands that run; the weights enter unfaded: f_b <= 1)."""
    s = np.asarray(s, np.float32).reshape(-1)
    count = active_count(s, first_band, nbands)
    by_count = {}
    for c in np.unique(count):
        rep = s[np.flatnonzero(count == c)[0]]
        assert _ref64_grad.active_bands(rep, first_band, nbands) == c
        by_count[int(c)] = _ref64_grad.tolerance(1.0, (rep, first_band, nbands, w, var_per_band))
    return np.array([by_count[int(c)] for c in count])


def texture_grey(n):
    """wavelet_texture's grey level of the float32 noise values n, as wn::wavelet_texture_grey forms it (float64 n / 4,
    clamp, 0.5 * (1 + c), rounded to float32): exact arithmetic on every step but the last cast."""
    q = np.asarray(n, np.float32).astype(np.float64) / 4.0
    return (0.5 * (1.0 + np.clip(q, -1.0, 1.0))).astype(np.float32)


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def footprints(first_band, nbands, count, seed):
    """`count` float32 footprints: -inf, +inf, NaN; the exact thresholds -(first_band + b) of every band and their float32
    neighbours on both sides; fractional values; values that leave 0, 1, ..., nbands bands; integer values; and uniform
    ones over the whole range -- each kind many times, shuffled."""
    rng = np.random.default_rng(seed)
    special = [-np.inf, np.inf, np.nan, 0.0, -0.0, 1e-30, -1e-30, -100.0, 100.0]
    for b in range(max(nbands, 1)):
        thr = f32(-(first_band + b))
        special += [thr, np.nextafter(thr, f32(-np.inf)), np.nextafter(thr, f32(np.inf)),
                    thr - f32(0.5), thr - f32(0.25), thr - f32(0.999), thr - f32(1e-3), thr + f32(0.25)]
    for c in range(nbands + 1):                              # c bands run: -c <= s + first_band < -(c - 1)
        special.append(f32(-first_band - c + 0.5))
    special = np.array(special, np.float32)
    lo, hi = -first_band - nbands - 1.5, -first_band + 1.5
    uniform = rng.uniform(lo, hi, count).astype(np.float32)
    integers = rng.integers(int(np.floor(lo)), int(np.ceil(hi)) + 1, count).astype(np.float32)
    pick = rng.integers(0, 3, count)
    s = np.where(pick == 0, rng.choice(special, count), np.where(pick == 1, uniform, integers)).astype(np.float32)
    s[:special.size] = special[:count]                       # every special value at least once
    return s[rng.permutation(count)]


def points(first_band, nbands, count, seed):
    """Half edge points (_ref64.edge_points), half uniform ones in [-300, 300]^3 and [-4, 4]^3.  The finest band
    evaluates at 2 * p * 2^(first_band + nbands - 1), and the evaluators form (int)ceilf(q - 0.5f) and mid +- 1: a
    coordinate past 2^31 has no defined result in C++ (as for wn_multiband3d_points), so edge points whose finest-band
    coordinate would pass 2^30 are replaced by others of the same set that stay inside."""
    rng = np.random.default_rng(seed)
    half = count // 2
    edges = _ref64.edge_points(3, 4 * half, seed + 1)
    limit = 2.0 ** 30 / 2.0 ** (first_band + max(nbands, 1))
    edges = edges[np.abs(edges).max(1) <= limit][:half]
    assert edges.shape[0] == half, edges.shape
    rest = count - half
    uniform = np.concatenate([rng.uniform(-300.0, 300.0, (rest - rest // 4, 3)), rng.uniform(-4.0, 4.0, (rest // 4, 3))])
    return np.concatenate([edges, uniform.astype(np.float32)])[rng.permutation(count)].astype(np.float32)


def normals(count, seed):
    ns = _ref64.normal_set()
    return np.ascontiguousarray(ns[np.random.default_rng(seed).integers(0, len(ns), count)])


# ---- the host evaluator (libwnoise_host.so) --------------------------------------------------------------------------------
def bind_host(lib):
    lib.wnhost_multiband3d_footprint.restype = C.c_float
    lib.wnhost_multiband3d_footprint.argtypes = [FP, C.c_int, FP, FP, C.c_float, C.c_int, C.c_int, C.c_int, FP, C.c_float, FP]
    lib.wnhost_wavelet_multiband_texture_value.restype = C.c_float
    lib.wnhost_wavelet_multiband_texture_value.argtypes = [FP, C.c_int, C.c_double, C.c_int, C.c_int, FP, C.c_float, C.c_int,
                                                           FP, C.c_float]
    return lib


def _tile_args(coef):
    if coef is None or np.asarray(coef).size == 0:
        return None, 0, None
    c = np.ascontiguousarray(coef, np.float32)
    return c.ctypes.data_as(FP), int(round(c.size ** (1.0 / 3.0))), c


def host_footprint(lib, coef, pts, nrs, s, first_band, nbands, w, var_per_band, fade):
    """wnhost_multiband3d_footprint at every point: ((N, 4) float32 of the gradient form, (N,) float32 of the value form).
    nrs: None, or one normal per point."""
    cp, n, _keep = _tile_args(coef)
    pts = np.ascontiguousarray(pts, np.float32)
    s = np.asarray(s, np.float32)
    wa = (C.c_float * max(1, nbands))(*[float(x) for x in w[:nbands]])
    out = np.empty((len(pts), 4), np.float32)
    val = np.empty(len(pts), np.float32)
    g = np.empty(3, np.float32)
    gp = g.ctypes.data_as(FP)
    if nrs is not None:
        nrs = np.ascontiguousarray(np.broadcast_to(np.asarray(nrs, np.float32).reshape(-1, 3), pts.shape))
    for i in range(len(pts)):
        p = pts[i].ctypes.data_as(FP)
        q = nrs[i].ctypes.data_as(FP) if nrs is not None else None
        out[i, 0] = lib.wnhost_multiband3d_footprint(cp, n, p, q, s[i], fade, first_band, nbands, wa, var_per_band, gp)
        out[i, 1:] = g
        val[i] = lib.wnhost_multiband3d_footprint(cp, n, p, q, s[i], fade, first_band, nbands, wa, var_per_band, None)
    return out, val


def host_texture(lib, coef, scale, pts, s, first_band, nbands, w, var_per_band, fade):
    cp, n, _keep = _tile_args(coef)
    pts = np.ascontiguousarray(pts, np.float32)
    s = np.asarray(s, np.float32)
    wa = (C.c_float * max(1, nbands))(*[float(x) for x in w[:nbands]])
    return np.array([lib.wnhost_wavelet_multiband_texture_value(cp, n, scale, first_band, nbands, wa, var_per_band, fade,
                                                                pts[i].ctypes.data_as(FP), s[i])
                     for i in range(len(pts))], np.float32)
