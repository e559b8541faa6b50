"""A float64 reference for curl noise on a 2-D tile (include/wnoise_curl2d.h), built on tests/_ref64_multiband2d.py: the
velocity v = (d psi/dy, -d psi/dx) of the stream function psi = WMultibandNoise2D at one footprint s with the hard cut, its
error bound, and the host's wnhost_multiband2d_curl through ctypes.

The bound: the curl channels ARE the gradient channels of that module's evaluator (one of them negated, which is exact), so
tolerance() is that module's gradient bound, K_g C u (41 + 4 nbands), unchanged.

A plain helper module (not a conftest): the tests import it by name.
"""
import ctypes as C

import numpy as np

import _ref64_multiband2d as M

f32 = np.float32
FP = M.FP


def stream_function(coef, pts, s, first_band, nbands, w, var_per_band):
    """psi at every point: (N,) float64."""
    return M.multiband2d_footprint_points(coef, pts, f32(s), first_band, nbands, w, var_per_band, 0)[:, 0]


def curl_points(coef, pts, s, first_band, nbands, w, var_per_band):
    """(N, 2) float64 of {d psi/dy, -d psi/dx}."""
    g = M.multiband2d_footprint_points(coef, pts, f32(s), first_band, nbands, w, var_per_band, 0)
    return np.stack([g[:, 2], -g[:, 1]], axis=1)


def tolerance(coef, s, first_band, nbands, w, var_per_band, count):
    """The (N, 2) per-point bound on |float32 evaluator - curl_points|: the gradient channels' own."""
    return M.tolerance(coef, f32(s), first_band, nbands, w, var_per_band, 0, count)[:, 1:]


def bind_host(lib):
    M.bind_host(lib)
    lib.wnhost_multiband2d_curl.restype = None   # AttributeError: the library has no 2-D curl
    lib.wnhost_multiband2d_curl.argtypes = [FP, C.c_int, FP, C.c_float, C.c_int, C.c_int, FP, C.c_float, FP]
    return lib


def tile_args(coef):
    """(pointer, n, the array that keeps the pointer alive) of an n x n tile; None or an empty array: the empty tile."""
    if coef is None or np.asarray(coef).size == 0:
        return None, 0, None
    keep = np.ascontiguousarray(coef, f32).reshape(-1)
    n = int(round(keep.size ** 0.5))
    assert n * n == keep.size
    return keep.ctypes.data_as(FP), n, keep


def host_curl(lib, coef, pts, s, first_band, nbands, w, var_per_band):
    """wnhost_multiband2d_curl at every point: (N, 2) float32."""
    cp, n, _keep = tile_args(coef)
    pts = np.ascontiguousarray(pts, f32).reshape(-1, 2)
    wa = (C.c_float * max(1, nbands))(*[float(x) for x in w[:nbands]])
    out = np.empty((len(pts), 2), f32)
    fn = lib.wnhost_multiband2d_curl
    for i in range(len(pts)):
        fn(cp, n, pts[i].ctypes.data_as(FP), float(s), first_band, nbands, wa, var_per_band, out[i].ctypes.data_as(FP))
    return out
