"""Python mirror of the reference's noise interface over the C ABI (include/wnoise.h).

Class and method names follow the reference (WaveletNoise.h:20-41, perlin.h:14-91,
experient/PerlinNoise.hpp:9-61, texture.h:14-115, experient/main.cpp:11-129) so the parity
tests read like calls into the reference.  Every evaluation runs on the GPU through
libwnoise_hip.so: scalar calls are batches of one.  torch is used for device memory and
streams only.
"""
import ctypes as C
import math
import sys
from dataclasses import dataclass

import numpy as np
import torch

from . import _capi
from ._capi import check, wn_grid, WN_GRID_DEFAULT, WN_GRID_EXACT, WN_Z_CONST, WN_Z_LATTICE

_lib = _capi.load()


# ---- plumbing -------------------------------------------------------------------------------
def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(x, dtype):
    """array-like / tensor -> contiguous CUDA tensor of `dtype` (no copy when already so)."""
    if isinstance(x, torch.Tensor):
        t = x
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=_NP[dtype])))
    return t.to(device="cuda", dtype=dtype).contiguous()


_NP = {torch.float32: np.float32, torch.float64: np.float64, torch.uint8: np.uint8}


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _is_scalar_point(p, width):
    if isinstance(p, torch.Tensor):
        return p.dim() == 1 and p.numel() == width
    a = np.asarray(p)
    return a.ndim == 1 and a.size == width


def _per_point(s):
    """True for an array of footprints (one per point), False for a scalar."""
    return s.dim() != 0 if isinstance(s, torch.Tensor) else np.ndim(s) != 0


def device_info():
    name = C.create_string_buffer(256)
    cus, hbm = C.c_int(0), C.c_size_t(0)
    check(_lib.wn_device_info(name, 256, C.byref(cus), C.byref(hbm)))
    return {"name": name.value.decode(), "compute_units": cus.value, "hbm_bytes": hbm.value}


class HipTimer:
    """HIP events recorded on the stream the kernels run on (torch's current stream)."""

    def __init__(self):
        self._h = C.c_void_p()
        check(_lib.wn_timer_create(C.byref(self._h)))

    def start(self):
        check(_lib.wn_timer_start(self._h, _stream()))

    def stop(self):
        check(_lib.wn_timer_stop(self._h, _stream()))

    def elapsed_ms(self):
        ms = C.c_float(0)
        check(_lib.wn_timer_elapsed_ms(self._h, C.byref(ms)))
        return ms.value

    def __del__(self):
        if getattr(self, "_h", None):
            _lib.wn_timer_destroy(self._h)
            self._h = None


# ---- WaveletNoise (WaveletNoise.h:20-59) ----------------------------------------------------
class WaveletNoise:
    def __init__(self, tileSize, seed=0):
        self.tileSizeN = _lib.wn_tile_even_size(int(tileSize))
        if self.tileSizeN != tileSize:  # WaveletNoise.cpp:22-25
            print(f"Warning: Tile size adjusted to {self.tileSizeN} (must be even)", file=sys.stderr)
        self.randomSeed = int(seed) & 0xFFFFFFFF
        self._drawn = 0      # Gaussian values consumed so far: the rng is a member (WaveletNoise.h:47)
        self._tile = None    # no coefficients yet: evaluate* return 0 (WaveletNoise.cpp:112,186,219)

    # -- tile management
    def _set_tile(self, handle):
        self._free()
        self._tile = handle

    def _free(self):
        if getattr(self, "_tile", None):
            _lib.wn_tile_destroy(self._tile)
        self._tile = None

    def __del__(self):
        self._free()

    def _handle(self, dims):
        """Tile handle for evaluation; an un-generated object evaluates an empty tile."""
        if self._tile is None:
            h = C.c_void_p()
            check(_lib.wn_tile_create(0, dims, None, C.byref(h)))
            self._tile = h
        return self._tile

    def _generate(self, dims):
        n = self.tileSizeN
        count = n ** dims
        # continue the member rng's stream: draw `_drawn + count` values, keep the tail
        field = np.empty(self._drawn + count, np.float32)
        check(_lib.wn_gaussian_fill(self.randomSeed, field.size, field.ctypes.data_as(C.c_void_p)))
        tail = np.ascontiguousarray(field[self._drawn:])
        self._drawn += count
        h = C.c_void_p()
        check(_lib.wn_tile_generate_from_field(n, dims, tail.ctypes.data_as(C.c_void_p), C.byref(h)))
        self._set_tile(h)

    def generateNoiseTile2D(self):
        self._generate(2)

    def generateNoiseTile3D(self):
        self._generate(3)

    @classmethod
    def from_coefficients(cls, coeffs, dims):
        """Adopt ready-made coefficients (n^dims floats, x fastest)."""
        c = np.ascontiguousarray(np.asarray(coeffs, np.float32).ravel())
        n = int(round(c.size ** (1.0 / dims))) if c.size else 0
        if n ** dims != c.size:
            raise ValueError("coefficient count is not n^dims")
        self = cls(n, 0)
        h = C.c_void_p()
        check(_lib.wn_tile_create(n, dims, c.ctypes.data_as(C.c_void_p) if c.size else None, C.byref(h)))
        self._set_tile(h)
        return self

    def getNoiseCoefficients(self):
        if self._tile is None:
            return np.empty(0, np.float32)
        out = np.empty(_lib.wn_tile_count(self._tile), np.float32)
        check(_lib.wn_tile_download(self._tile, out.ctypes.data_as(C.c_void_p)))
        return out

    def getTileSize(self):
        return self.tileSizeN

    # -- evaluation: a single point returns a float, an (N,k) batch returns a CUDA tensor
    def _scalar(self, fn, dims, p, width, normal=None):
        """One value through the resident scalar kernel (wn_scalar_*: no launch per call)."""
        a = (C.c_float * width)(*[float(v) for v in (p.tolist() if hasattr(p, "tolist") else p)])
        out = C.c_float(0)
        if normal is None:
            check(fn(self._handle(dims), a, C.byref(out)))
        else:
            nr = (C.c_float * 3)(*[float(v) for v in (normal.tolist() if hasattr(normal, "tolist") else normal)])
            check(fn(self._handle(dims), a, nr, C.byref(out)))
        return out.value

    def _points(self, fn, dims, p, width, extra=None):
        single = _is_scalar_point(p, width)
        pts = _dev(p, torch.float32).reshape(-1, width)
        out = torch.empty(pts.shape[0], dtype=torch.float32, device="cuda")
        if extra is None:
            check(fn(self._handle(dims), _ptr(pts), pts.shape[0], _ptr(out), _stream()))
        else:
            check(fn(self._handle(dims), _ptr(pts), _ptr(extra), pts.shape[0], _ptr(out), _stream()))
        return float(out.item()) if single else out

    def evaluate2D(self, p):
        if _is_scalar_point(p, 2):
            return self._scalar(_lib.wn_scalar_eval2d, 2, p, 2)
        return self._points(_lib.wn_eval2d_points, 2, p, 2)

    def evaluate3D(self, p):
        if _is_scalar_point(p, 3):
            return self._scalar(_lib.wn_scalar_eval3d, 3, p, 3)
        return self._points(_lib.wn_eval3d_points, 3, p, 3)

    def evaluate3DProjected(self, p, normal):
        if _is_scalar_point(p, 3) and _is_scalar_point(normal, 3):
            return self._scalar(_lib.wn_scalar_eval3d_projected, 3, p, 3, normal)
        pts = _dev(p, torch.float32).reshape(-1, 3)
        nr = _dev(normal, torch.float32).reshape(-1, 3)
        if nr.shape[0] == 1 and pts.shape[0] != 1:
            nr = nr.expand(pts.shape[0], 3).contiguous()
        return self._points(_lib.wn_eval3d_projected_points, 3, p, 3, extra=nr)

    def _footprint(self, p, s, firstBand, nbands, w, variance, normal, fade, grad):
        """WMultibandNoise / its gradient with one footprint per point (include/wnoise_footprint.h)."""
        pts = _dev(p, torch.float32).reshape(-1, 3)
        sd = _dev(s, torch.float32).reshape(-1)
        if sd.shape[0] != pts.shape[0]:
            raise ValueError("s: a scalar, or one footprint per point")
        out = torch.empty((pts.shape[0], 4) if grad else pts.shape[0], dtype=torch.float32, device="cuda")
        wa = (C.c_float * max(1, nbands))(*[float(x) for x in list(w)[:nbands]])
        if normal is not None:
            nr = _dev(normal, torch.float32).reshape(-1, 3)
            one = nr.shape[0] == 1
            if not one and nr.shape[0] != pts.shape[0]:
                raise ValueError("normal: one vector, or one per point")
            fn = _lib.wn_multiband3d_projected_footprint_grad_points if grad else _lib.wn_multiband3d_projected_footprint_points
            check(fn(self._handle(3), _ptr(pts), _ptr(nr), int(one), _ptr(sd), pts.shape[0], int(firstBand), int(nbands), wa,
                     float(0.296 if variance is None else variance), int(bool(fade)), _ptr(out), _stream()))
            return out
        fn = _lib.wn_multiband3d_footprint_grad_points if grad else _lib.wn_multiband3d_footprint_points
        check(fn(self._handle(3), _ptr(pts), _ptr(sd), pts.shape[0], int(firstBand), int(nbands), wa,
                 float(0.18402 if variance is None else variance), int(bool(fade)), _ptr(out), _stream()))
        return out

    def WMultibandNoise(self, p, s, firstBand, nbands, w, variance=None, normal=None, fade=False):
        """Cook & DeRose Appendix 2; absent from the reference.  normal=None: bands are WNoise = evaluate3D
        (variance defaults to the reference's empirical 0.18402); with a normal (one for all points, or one per
        point) bands are WProjectedNoise = evaluate3DProjected (variance defaults to 0.296).
        `s`: a scalar -- one footprint for the whole call (wn_multiband3d_points; `fade` is not read) -- or an array
        with one footprint per point (include/wnoise_footprint.h): band b of a point runs while (s + firstBand) + b < 0,
        and with fade=True the finest surviving band fades in over one octave of footprint."""
        if _per_point(s):
            return self._footprint(p, s, firstBand, nbands, w, variance, normal, fade, False)
        single = _is_scalar_point(p, 3)
        pts = _dev(p, torch.float32).reshape(-1, 3)
        out = torch.empty(pts.shape[0], dtype=torch.float32, device="cuda")
        wa = (C.c_float * max(1, nbands))(*[float(x) for x in list(w)[:nbands]])
        if normal is not None:
            nr = _dev(normal, torch.float32).reshape(-1, 3)
            one = nr.shape[0] == 1
            if not one and nr.shape[0] != pts.shape[0]:
                raise ValueError("normal: one vector, or one per point")
            check(_lib.wn_multiband3d_projected_points(self._handle(3), _ptr(pts), _ptr(nr), int(one), pts.shape[0],
                                                       float(s), int(firstBand), int(nbands), wa,
                                                       float(0.296 if variance is None else variance), _ptr(out),
                                                       _stream()))
            return float(out.item()) if single else out
        variance = 0.18402 if variance is None else variance
        check(_lib.wn_multiband3d_points(self._handle(3), _ptr(pts), pts.shape[0], float(s),
                                         int(firstBand), int(nbands), wa, float(variance),
                                         _ptr(out), _stream()))
        return float(out.item()) if single else out

    # -- analytic gradients (absent from the reference): (N, 4) CUDA tensors of {value, d/dx, d/dy, d/dz}
    def evaluate3DGradient(self, p):
        """evaluate3D and its gradient at one point or an (N, 3) batch (wn_eval3d_grad_points): the value column has the
        bits of evaluate3D."""
        pts = _dev(p, torch.float32).reshape(-1, 3)
        out = torch.empty((pts.shape[0], 4), dtype=torch.float32, device="cuda")
        check(_lib.wn_eval3d_grad_points(self._handle(3), _ptr(pts), pts.shape[0], _ptr(out), _stream()))
        return out

    def WMultibandNoiseGradient(self, p, s, firstBand, nbands, w, variance=None, normal=None, fade=False):
        """WMultibandNoise and its gradient with respect to p.  normal=None: bands are evaluate3D
        (wn_multiband3d_grad_points; variance defaults to 0.18402); with a normal (one for all points, or one per point)
        bands are evaluate3DProjected (wn_multiband3d_projected_grad_points; variance defaults to 0.296).
        `s` and `fade` as in WMultibandNoise: an array s gives every point its own band limit."""
        if _per_point(s):
            return self._footprint(p, s, firstBand, nbands, w, variance, normal, fade, True)
        pts = _dev(p, torch.float32).reshape(-1, 3)
        out = torch.empty((pts.shape[0], 4), dtype=torch.float32, device="cuda")
        wa = (C.c_float * max(1, nbands))(*[float(x) for x in list(w)[:nbands]])
        if normal is not None:
            nr = _dev(normal, torch.float32).reshape(-1, 3)
            one = nr.shape[0] == 1
            if not one and nr.shape[0] != pts.shape[0]:
                raise ValueError("normal: one vector, or one per point")
            check(_lib.wn_multiband3d_projected_grad_points(self._handle(3), _ptr(pts), _ptr(nr), int(one), pts.shape[0],
                                                            float(s), int(firstBand), int(nbands), wa,
                                                            float(0.296 if variance is None else variance), _ptr(out),
                                                            _stream()))
            return out
        variance = 0.18402 if variance is None else variance
        check(_lib.wn_multiband3d_grad_points(self._handle(3), _ptr(pts), pts.shape[0], float(s), int(firstBand),
                                              int(nbands), wa, float(variance), _ptr(out), _stream()))
        return out

    # -- divergence-free curl noise (absent from the reference): (N, 3) CUDA tensors of {vx, vy, vz}
    def _curl_offsets(self, offsets):
        """Nine int32: the (x, y, z) whole-cell tile offsets of the potentials psi0, psi1, psi2.  None: (0, 0, 0),
        (n//3,)*3, (2*n//3,)*3 of the tile size n -- a default only, not a measured decorrelation."""
        if offsets is None:
            n = self.tileSizeN
            offsets = ((0, 0, 0), (n // 3,) * 3, (2 * n // 3,) * 3)
        flat = [int(v) for v in np.asarray(offsets, dtype=np.int64).reshape(-1)]
        if len(flat) != 9:
            raise ValueError("offsets: three (x, y, z) triples")
        return (C.c_int32 * 9)(*flat)

    def evaluate3DCurl(self, p, offsets=None):
        """The curl of the vector potential whose components are evaluate3D of this tile shifted by the whole-cell
        `offsets` (wn_eval3d_curl_points), at one point or an (N, 3) batch: v = (d psi2/dy - d psi1/dz, d psi0/dz -
        d psi2/dx, d psi1/dx - d psi0/dy), divergence-free.  Every component has the bits of the subtraction of two
        evaluate3DGradient channels on from_coefficients(np.roll(c3, (-oz, -oy, -ox), (0, 1, 2))) tiles."""
        pts = _dev(p, torch.float32).reshape(-1, 3)
        out = torch.empty((pts.shape[0], 3), dtype=torch.float32, device="cuda")
        check(_lib.wn_eval3d_curl_points(self._handle(3), _ptr(pts), pts.shape[0], self._curl_offsets(offsets), _ptr(out),
                                         _stream()))
        return out

    def WMultibandNoiseCurl(self, p, s, firstBand, nbands, w, variance=None, offsets=None):
        """evaluate3DCurl with WMultibandNoise (normal=None) potentials, derivatives with respect to p
        (wn_multiband3d_curl_points); the offsets are the same in every band."""
        pts = _dev(p, torch.float32).reshape(-1, 3)
        out = torch.empty((pts.shape[0], 3), dtype=torch.float32, device="cuda")
        wa = (C.c_float * max(1, nbands))(*[float(x) for x in list(w)[:nbands]])
        check(_lib.wn_multiband3d_curl_points(self._handle(3), _ptr(pts), pts.shape[0], self._curl_offsets(offsets),
                                              float(s), int(firstBand), int(nbands), wa,
                                              float(0.18402 if variance is None else variance), _ptr(out), _stream()))
        return out

    # -- particles moved through that curl field (include/wnoise_advect.h; absent from the reference)
    _ADVECT_METHODS = {"euler": _capi.WN_ADVECT_EULER, "midpoint": _capi.WN_ADVECT_MIDPOINT, "rk4": _capi.WN_ADVECT_RK4}

    def _advect(self, call, pts, h, steps, method, gain, drift, trajectory_every):
        if method not in self._ADVECT_METHODS:
            raise ValueError(f"method: one of {sorted(self._ADVECT_METHODS)}")
        pts = _dev(pts, torch.float32).reshape(-1, 3)
        n, steps, every = pts.shape[0], int(steps), int(trajectory_every)
        a = _capi.wn_advect(self._ADVECT_METHODS[method], steps, float(h), float(gain),
                            (C.c_float * 3)(*([0.0] * 3 if drift is None else [float(x) for x in drift])), every)
        out = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        traj = torch.empty((steps // every + 1, n, 3), dtype=torch.float32, device="cuda") if every >= 1 and steps >= 0 else None
        check(call(_ptr(pts), n, C.byref(a), _ptr(out), _ptr(traj)))
        return out if traj is None else (out, traj)

    def advectCurl(self, pts, h, steps, method="rk4", offsets=None, gain=1.0, drift=None, trajectory_every=0):
        """An (N, 3) batch of particles moved `steps` time steps of size h (negative: backwards) through the velocity
        gain * evaluate3DCurl(., offsets) + drift, all steps inside the kernel (wn_eval3d_curl_advect_points).  method:
        "euler", "midpoint" or "rk4".  Returns the final (N, 3) positions; with trajectory_every = e >= 1 also the
        (steps // e + 1, N, 3) positions after steps 0, e, 2e, ...  Float32 with every operation rounded on its own: the
        bits of stepping with evaluate3DCurl and separately rounded float32 tensor operations."""
        off = self._curl_offsets(offsets)
        return self._advect(lambda p, n, a, out, traj: _lib.wn_eval3d_curl_advect_points(
            self._handle(3), p, n, off, a, out, traj, _stream()), pts, h, steps, method, gain, drift, trajectory_every)

    def WMultibandNoiseAdvectCurl(self, pts, h, steps, s, firstBand, nbands, w, variance=None, method="rk4", offsets=None,
                                  gain=1.0, drift=None, trajectory_every=0):
        """advectCurl through gain * WMultibandNoiseCurl(., s, firstBand, nbands, w, variance, offsets) + drift
        (wn_multiband3d_curl_advect_points)."""
        off = self._curl_offsets(offsets)
        wa = (C.c_float * max(1, nbands))(*[float(x) for x in list(w)[:nbands]])
        var = float(0.18402 if variance is None else variance)
        return self._advect(lambda p, n, a, out, traj: _lib.wn_multiband3d_curl_advect_points(
            self._handle(3), p, n, off, float(s), int(firstBand), int(nbands), wa, var, a, out, traj, _stream()),
            pts, h, steps, method, gain, drift, trajectory_every)

    # -- that curl field with solid boundaries (include/wnoise_bounded.h; absent from the reference)
    _OBSTACLE_KINDS = {"sphere": _capi.WN_OBSTACLE_SPHERE, "container": _capi.WN_OBSTACLE_CONTAINER,
                       "halfspace": _capi.WN_OBSTACLE_HALFSPACE}

    @classmethod
    def _obstacles(cls, obstacles):
        """The wn_obstacle array of a list of ("sphere", c, r, d0), ("container", c, r, d0) and ("halfspace", n, o, d0)
        entries, and its length; the library checks the values."""
        obstacles = list(obstacles)
        arr = (_capi.wn_obstacle * max(1, len(obstacles)))()
        for dst, entry in zip(arr, obstacles):
            kind, c, r, d0 = entry
            if kind not in cls._OBSTACLE_KINDS:
                raise ValueError(f"obstacle kind: one of {sorted(cls._OBSTACLE_KINDS)}")
            c = [float(x) for x in c]
            if len(c) != 3:
                raise ValueError("an obstacle's centre or normal has three components")
            dst.kind, dst.c, dst.r, dst.d0 = cls._OBSTACLE_KINDS[kind], (C.c_float * 3)(*c), float(r), float(d0)
        return arr, len(obstacles)

    def evaluate3DCurlBounded(self, p, obstacles, offsets=None):
        """evaluate3DCurl with its potential faded to zero towards every solid of `obstacles`
        (wn_eval3d_curl_bounded_points): v = A curl Psi + grad A x Psi, still divergence-free, with no normal component on
        a solid's surface.  `obstacles`: a list of at most 16 ("sphere", c, r, d0), ("container", c, r, d0) or
        ("halfspace", n, o, d0), in the coordinates of p; d0 is the width of the ramp.  A point inside a solid gets 0, a
        point at distance >= d0 from all of them (and obstacles=[]) the bits of evaluate3DCurl."""
        pts = _dev(p, torch.float32).reshape(-1, 3)
        out = torch.empty((pts.shape[0], 3), dtype=torch.float32, device="cuda")
        obs, nobs = self._obstacles(obstacles)
        check(_lib.wn_eval3d_curl_bounded_points(self._handle(3), _ptr(pts), pts.shape[0], self._curl_offsets(offsets), obs,
                                                 nobs, _ptr(out), _stream()))
        return out

    def WMultibandNoiseCurlBounded(self, p, obstacles, s, firstBand, nbands, w, variance=None, offsets=None):
        """evaluate3DCurlBounded with WMultibandNoise (normal=None) potentials (wn_multiband3d_curl_bounded_points); the
        obstacles live in the coordinates of p."""
        pts = _dev(p, torch.float32).reshape(-1, 3)
        out = torch.empty((pts.shape[0], 3), dtype=torch.float32, device="cuda")
        wa = (C.c_float * max(1, nbands))(*[float(x) for x in list(w)[:nbands]])
        obs, nobs = self._obstacles(obstacles)
        check(_lib.wn_multiband3d_curl_bounded_points(self._handle(3), _ptr(pts), pts.shape[0], self._curl_offsets(offsets),
                                                      float(s), int(firstBand), int(nbands), wa,
                                                      float(0.18402 if variance is None else variance), obs, nobs,
                                                      _ptr(out), _stream()))
        return out

    def advectCurlBounded(self, pts, h, steps, obstacles, method="rk4", offsets=None, gain=1.0, drift=None,
                          trajectory_every=0):
        """advectCurl through gain * evaluate3DCurlBounded(., obstacles, offsets) + drift, all steps inside the kernel
        (wn_eval3d_curl_bounded_advect_points): particles flow around the solids.  A particle inside one moves by drift
        alone."""
        off = self._curl_offsets(offsets)
        obs, nobs = self._obstacles(obstacles)
        return self._advect(lambda p, n, a, out, traj: _lib.wn_eval3d_curl_bounded_advect_points(
            self._handle(3), p, n, off, obs, nobs, a, out, traj, _stream()), pts, h, steps, method, gain, drift,
            trajectory_every)

    def WMultibandNoiseAdvectCurlBounded(self, pts, h, steps, obstacles, s, firstBand, nbands, w, variance=None, method="rk4",
                                         offsets=None, gain=1.0, drift=None, trajectory_every=0):
        """advectCurlBounded through gain * WMultibandNoiseCurlBounded(., obstacles, s, firstBand, nbands, w, variance,
        offsets) + drift (wn_multiband3d_curl_bounded_advect_points)."""
        off = self._curl_offsets(offsets)
        obs, nobs = self._obstacles(obstacles)
        wa = (C.c_float * max(1, nbands))(*[float(x) for x in list(w)[:nbands]])
        var = float(0.18402 if variance is None else variance)
        return self._advect(lambda p, n, a, out, traj: _lib.wn_multiband3d_curl_bounded_advect_points(
            self._handle(3), p, n, off, float(s), int(firstBand), int(nbands), wa, var, obs, nobs, a, out, traj, _stream()),
            pts, h, steps, method, gain, drift, trajectory_every)

    def evaluate2DGradient(self, p):
        """evaluate2D and its gradient at one point or an (N, 2) batch (wn_eval2d_grad_points): an (N, 3) CUDA tensor of
        {value, d/dx, d/dy}; the value column has the bits of evaluate2D."""
        pts = _dev(p, torch.float32).reshape(-1, 2)
        out = torch.empty((pts.shape[0], 3), dtype=torch.float32, device="cuda")
        check(_lib.wn_eval2d_grad_points(self._handle(2), _ptr(pts), pts.shape[0], _ptr(out), _stream()))
        return out

    # -- WMultibandNoise on the 2-D tile (include/wnoise_multiband2d.h; absent from the reference)
    def _multiband2d(self, p, s, firstBand, nbands, w, variance, fade, grad):
        single = _is_scalar_point(p, 2) and not grad
        pts = _dev(p, torch.float32).reshape(-1, 2)
        n = pts.shape[0]
        out = torch.empty((n, 3) if grad else n, dtype=torch.float32, device="cuda")
        wa = (C.c_float * max(1, nbands))(*[float(x) for x in list(w)[:nbands]])
        if _per_point(s):
            sd = _dev(s, torch.float32).reshape(-1)
            if sd.shape[0] != n:
                raise ValueError("s: a scalar, or one footprint per point")
            fn = _lib.wn_multiband2d_footprint_grad_points if grad else _lib.wn_multiband2d_footprint_points
            check(fn(self._handle(2), _ptr(pts), _ptr(sd), n, int(firstBand), int(nbands), wa, float(variance),
                     int(bool(fade)), _ptr(out), _stream()))
            return out
        fn = _lib.wn_multiband2d_grad_points if grad else _lib.wn_multiband2d_points
        check(fn(self._handle(2), _ptr(pts), n, float(s), int(firstBand), int(nbands), wa, float(variance), _ptr(out),
                 _stream()))
        return float(out.item()) if single else out

    def WMultibandNoise2D(self, p, s, firstBand, nbands, w, variance=0.19686, fade=False):
        """WMultibandNoise with evaluate2D bands on the 2-D tile, at one point or an (N, 2) batch: sum_b w[b] *
        evaluate2D(2 * p * 2^(firstBand+b)) over the bands with (s + firstBand) + b < 0, divided by
        sqrt(sum w^2 * variance) (variance defaults to the reference's 2-D constant 0.19686).  `s`: a scalar -- one
        footprint for the whole call (wn_multiband2d_points; `fade` is not read) -- or one footprint per point
        (wn_multiband2d_footprint_points): with fade=True the finest surviving band of a point fades in over one octave."""
        return self._multiband2d(p, s, firstBand, nbands, w, variance, fade, False)

    def WMultibandNoise2DGradient(self, p, s, firstBand, nbands, w, variance=0.19686, fade=False):
        """WMultibandNoise2D and its gradient with respect to p: an (N, 3) CUDA tensor of {value, d/dx, d/dy}
        (wn_multiband2d_grad_points / wn_multiband2d_footprint_grad_points); the value column has the bits of
        WMultibandNoise2D."""
        return self._multiband2d(p, s, firstBand, nbands, w, variance, fade, True)

    # -- curl noise on the 2-D tile and particles moved through it (include/wnoise_curl2d.h; absent from the reference)
    def WMultibandNoise2DCurl(self, p, s, firstBand, nbands, w, variance=0.19686):
        """The divergence-free velocity (d psi/dy, -d psi/dx) of the stream function psi = WMultibandNoise2D at the scalar
        footprint s, at one point or an (N, 2) batch (wn_multiband2d_curl_points): an (N, 2) CUDA tensor of {vx, vy}.  vx has
        the bits of WMultibandNoise2DGradient's d/dy column, vy those of its d/dx column with the sign flipped.
        firstBand=-1, nbands=1, w=[1], variance=1 is the curl of evaluate2D."""
        pts = _dev(p, torch.float32).reshape(-1, 2)
        out = torch.empty((pts.shape[0], 2), dtype=torch.float32, device="cuda")
        wa = (C.c_float * max(1, nbands))(*[float(x) for x in list(w)[:nbands]])
        check(_lib.wn_multiband2d_curl_points(self._handle(2), _ptr(pts), pts.shape[0], float(s), int(firstBand), int(nbands),
                                              wa, float(variance), _ptr(out), _stream()))
        return out

    def WMultibandNoise2DAdvectCurl(self, pts, h, steps, s, firstBand, nbands, w, variance=0.19686, method="rk4", gain=1.0,
                                    drift=None, trajectory_every=0):
        """An (N, 2) batch of particles moved `steps` time steps of size h (negative: backwards) through the velocity
        gain * WMultibandNoise2DCurl(., s, firstBand, nbands, w, variance) + drift, all steps inside the kernel
        (wn_multiband2d_curl_advect_points).  method: "euler", "midpoint" or "rk4".  Returns the final (N, 2) positions; with
        trajectory_every = e >= 1 also the (steps // e + 1, N, 2) positions after steps 0, e, 2e, ...  Float32 with every
        operation rounded on its own: the bits of stepping with WMultibandNoise2DCurl and separately rounded float32 tensor
        operations."""
        if method not in self._ADVECT_METHODS:
            raise ValueError(f"method: one of {sorted(self._ADVECT_METHODS)}")
        pts = _dev(pts, torch.float32).reshape(-1, 2)
        n, steps, every = pts.shape[0], int(steps), int(trajectory_every)
        a = _capi.wn_advect2d(self._ADVECT_METHODS[method], steps, float(h), float(gain),
                              (C.c_float * 2)(*([0.0] * 2 if drift is None else [float(x) for x in drift])), every)
        wa = (C.c_float * max(1, nbands))(*[float(x) for x in list(w)[:nbands]])
        out = torch.empty((n, 2), dtype=torch.float32, device="cuda")
        traj = torch.empty((steps // every + 1, n, 2), dtype=torch.float32, device="cuda") if every >= 1 and steps >= 0 else None
        check(_lib.wn_multiband2d_curl_advect_points(self._handle(2), _ptr(pts), n, float(s), int(firstBand), int(nbands), wa,
                                                     float(variance), C.byref(a), _ptr(out), _ptr(traj), _stream()))
        return out if traj is None else (out, traj)

    # -- that field with solid boundaries and a background stream (include/wnoise_bounded2d.h; absent from the reference)
    _OBSTACLE2D_KINDS = {"disc": _capi.WN_OBSTACLE_SPHERE, "container": _capi.WN_OBSTACLE_CONTAINER,
                         "halfplane": _capi.WN_OBSTACLE_HALFSPACE}

    @classmethod
    def _bounds2d(cls, obstacles, flow):
        """The wn_obstacle2d array of a list of ("disc", c, r, d0), ("container", c, r, d0) and ("halfplane", n, o, d0)
        entries, its length, and the float pair of flow=(ux, uy) or None; the library checks the values."""
        obstacles = list(obstacles)
        arr = (_capi.wn_obstacle2d * max(1, len(obstacles)))()
        for dst, entry in zip(arr, obstacles):
            kind, c, r, d0 = entry
            if kind not in cls._OBSTACLE2D_KINDS:
                raise ValueError(f"obstacle kind: one of {sorted(cls._OBSTACLE2D_KINDS)}")
            c = [float(x) for x in c]
            if len(c) != 2:
                raise ValueError("an obstacle's centre or normal has two components")
            dst.kind, dst.c, dst.r, dst.d0 = cls._OBSTACLE2D_KINDS[kind], (C.c_float * 2)(*c), float(r), float(d0)
        if flow is not None:
            flow = [float(x) for x in flow]
            if len(flow) != 2:
                raise ValueError("flow: None or (ux, uy)")
            flow = (C.c_float * 2)(*flow)
        return arr, len(obstacles), flow

    def WMultibandNoise2DCurlBounded(self, p, obstacles, s, firstBand, nbands, w, variance=0.19686, flow=None):
        """WMultibandNoise2DCurl with its stream function faded to zero towards every solid of `obstacles`
        (wn_multiband2d_curl_bounded_points): still divergence-free, with no normal component on a solid's surface.
        `obstacles`: a list of at most 16 ("disc", c, r, d0), ("container", c, r, d0) or ("halfplane", n, o, d0), in the
        coordinates of p; d0 is the width of the ramp.  flow=(ux, uy) adds the uniform stream ux * y - uy * x to the stream
        function, so that it is bent around the solids with the noise (a drift is not).  A point inside a solid gets 0; with
        flow=None a point at distance >= d0 from every solid (and obstacles=[]) has the bits of WMultibandNoise2DCurl."""
        pts = _dev(p, torch.float32).reshape(-1, 2)
        out = torch.empty((pts.shape[0], 2), dtype=torch.float32, device="cuda")
        wa = (C.c_float * max(1, nbands))(*[float(x) for x in list(w)[:nbands]])
        obs, nobs, fl = self._bounds2d(obstacles, flow)
        check(_lib.wn_multiband2d_curl_bounded_points(self._handle(2), _ptr(pts), pts.shape[0], float(s), int(firstBand),
                                                      int(nbands), wa, float(variance), obs, nobs, fl, _ptr(out), _stream()))
        return out

    def WMultibandNoise2DAdvectCurlBounded(self, pts, h, steps, obstacles, s, firstBand, nbands, w, variance=0.19686,
                                           method="rk4", gain=1.0, drift=None, trajectory_every=0, flow=None):
        """WMultibandNoise2DAdvectCurl through gain * WMultibandNoise2DCurlBounded(., obstacles, s, firstBand, nbands, w,
        variance, flow) + drift, all steps inside the kernel (wn_multiband2d_curl_bounded_advect_points): particles flow
        around the solids.  A particle inside one moves by drift alone."""
        if method not in self._ADVECT_METHODS:
            raise ValueError(f"method: one of {sorted(self._ADVECT_METHODS)}")
        pts = _dev(pts, torch.float32).reshape(-1, 2)
        n, steps, every = pts.shape[0], int(steps), int(trajectory_every)
        a = _capi.wn_advect2d(self._ADVECT_METHODS[method], steps, float(h), float(gain),
                              (C.c_float * 2)(*([0.0] * 2 if drift is None else [float(x) for x in drift])), every)
        wa = (C.c_float * max(1, nbands))(*[float(x) for x in list(w)[:nbands]])
        obs, nobs, fl = self._bounds2d(obstacles, flow)
        out = torch.empty((n, 2), dtype=torch.float32, device="cuda")
        traj = torch.empty((steps // every + 1, n, 2), dtype=torch.float32, device="cuda") if every >= 1 and steps >= 0 else None
        check(_lib.wn_multiband2d_curl_bounded_advect_points(self._handle(2), _ptr(pts), n, float(s), int(firstBand),
                                                             int(nbands), wa, float(variance), obs, nobs, fl, C.byref(a),
                                                             _ptr(out), _ptr(traj), _stream()))
        return out if traj is None else (out, traj)

    def evaluate3DProjectedGradient(self, p, normal):
        """evaluate3DProjected and its gradient with respect to p, the normal held fixed (wn_eval3d_projected_grad_points):
        (N, 4).  `normal`: one for all points, or one per point.  The value column has the bits of evaluate3DProjected;
        the gradient is that of the sum without the value's 1e-6 weight cut (include/wnoise.h)."""
        pts = _dev(p, torch.float32).reshape(-1, 3)
        nr = _dev(normal, torch.float32).reshape(-1, 3)
        if nr.shape[0] == 1 and pts.shape[0] != 1:
            nr = nr.expand(pts.shape[0], 3).contiguous()
        if nr.shape[0] != pts.shape[0]:
            raise ValueError("normal: one vector, or one per point")
        out = torch.empty((pts.shape[0], 4), dtype=torch.float32, device="cuda")
        check(_lib.wn_eval3d_projected_grad_points(self._handle(3), _ptr(pts), _ptr(nr), pts.shape[0], _ptr(out),
                                                   _stream()))
        return out


# ---- perlin / PerlinNoise (perlin.h:14-91, experient/PerlinNoise.hpp:9-61) -------------------
class perlin:
    def __init__(self, seed=5489):  # std::mt19937::default_seed
        self._h = C.c_void_p()
        check(_lib.wn_perm_create_seeded(int(seed) & 0xFFFFFFFF, C.byref(self._h)))

    @classmethod
    def from_table(cls, table512):
        self = cls.__new__(cls)
        t = np.ascontiguousarray(np.asarray(table512, np.int32))
        self._h = C.c_void_p()
        check(_lib.wn_perm_create(t.ctypes.data_as(C.c_void_p), C.byref(self._h)))
        return self

    def __del__(self):
        if getattr(self, "_h", None):
            _lib.wn_perm_destroy(self._h)
            self._h = None

    @property
    def p(self):
        out = np.empty(512, np.int32)
        check(_lib.wn_perm_download(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def _run(self, fn, pts, *mid):
        out = torch.empty(pts.shape[0], dtype=torch.float64, device="cuda")
        check(fn(self._h, _ptr(pts), pts.shape[0], *mid, _ptr(out), _stream()))
        return out

    def noise(self, x, y=None, z=None):
        """noise(x,y,z) / noise(x,y) on doubles (perlin.h:42,65); noise(p) on a float vec3 or an
        (N,3) batch: float32 input follows noise(const point3&) (perlin.h:70), float64 input
        follows noise(double,double,double)."""
        if y is not None:
            out = C.c_double(0)
            check(_lib.wn_scalar_perlin(self._h, float(x), float(y), 0.0 if z is None else float(z), C.byref(out)))
            return out.value
        single = _is_scalar_point(x, 3)
        is64 = (x.dtype == torch.float64) if isinstance(x, torch.Tensor) else \
            (np.asarray(x).dtype == np.float64 and not single)
        if single and not is64:
            return self._scalar_vec3(x, 0)  # noise(const point3&), perlin.h:70
        if is64:
            out = self._run(_lib.wn_perlin_points, _dev(x, torch.float64).reshape(-1, 3))
        else:
            out = self._run(_lib.wn_perlin_points_vec3, _dev(x, torch.float32).reshape(-1, 3))
        return float(out.item()) if single else out

    def _scalar_vec3(self, p, kind, depth=0):
        a = (C.c_float * 3)(*[float(v) for v in (p.tolist() if hasattr(p, "tolist") else p)])
        out = C.c_double(0)
        check(_lib.wn_scalar_perlin_vec3(self._h, a, kind, depth, C.byref(out)))
        return out.value

    def fractal_noise(self, p):
        single = _is_scalar_point(p, 3)
        if single:
            return self._scalar_vec3(p, 2)
        out = self._run(_lib.wn_perlin_fractal_points, _dev(p, torch.float32).reshape(-1, 3))
        return float(out.item()) if single else out

    def turb(self, p, depth=7):
        """RTOW turb(p, depth); absent from the reference."""
        single = _is_scalar_point(p, 3)
        if single:
            return self._scalar_vec3(p, 1, int(depth))
        out = self._run(_lib.wn_perlin_turb_points, _dev(p, torch.float32).reshape(-1, 3), int(depth))
        return float(out.item()) if single else out

    # -- analytic gradients (absent from the reference): (N, 4) float64 CUDA tensors of {value, d/dx, d/dy, d/dz}
    def _grad(self, fn, pts, *mid):
        out = torch.empty((pts.shape[0], 4), dtype=torch.float64, device="cuda")
        check(fn(self._h, _ptr(pts), pts.shape[0], *mid, _ptr(out), _stream()))
        return out

    def noise_gradient(self, p):
        """noise and its gradient at one point or an (N, 3) batch: float64 input follows noise(double, double, double)
        (wn_perlin_grad_points), anything else noise(const point3&) on floats (wn_perlin_grad_points_vec3).  The value
        column has the bits of noise()."""
        is64 = (p.dtype == torch.float64) if isinstance(p, torch.Tensor) else (np.asarray(p).dtype == np.float64)
        if is64:
            return self._grad(_lib.wn_perlin_grad_points, _dev(p, torch.float64).reshape(-1, 3))
        return self._grad(_lib.wn_perlin_grad_points_vec3, _dev(p, torch.float32).reshape(-1, 3))

    def turb_gradient(self, p, depth=7):
        """turb(p, depth) and its gradient (wn_perlin_turb_grad_points): the sign of the octave sum times the sum of the
        octaves' noise gradients; not differentiable where the sum is 0."""
        return self._grad(_lib.wn_perlin_turb_grad_points, _dev(p, torch.float32).reshape(-1, 3), int(depth))

    def fractal_noise_gradient(self, p):
        """fractal_noise(p) and its gradient (wn_perlin_fractal_grad_points)."""
        return self._grad(_lib.wn_perlin_fractal_grad_points, _dev(p, torch.float32).reshape(-1, 3))


    # -- divergence-free curl noise (absent from the reference; include/wnoise_perlin_curl.h): (N, 3) float64 CUDA
    # tensors of {vx, vy, vz}
    @staticmethod
    def _curl_offsets(offsets):
        """Nine int32: the (x, y, z) whole-cell offsets of the potentials psi0, psi1, psi2 (any integers, reduced
        & 255).  None: (0, 0, 0), (85, 85, 85), (170, 170, 170) -- a default only, not a measured decorrelation."""
        if offsets is None:
            offsets = ((0, 0, 0), (85, 85, 85), (170, 170, 170))
        flat = [int(v) for v in np.asarray(offsets, dtype=np.int64).reshape(-1)]
        if len(flat) != 9:
            raise ValueError("offsets: three (x, y, z) triples")
        return (C.c_int32 * 9)(*flat)

    def _curl(self, pts, kind, depth, offsets):
        out = torch.empty((pts.shape[0], 3), dtype=torch.float64, device="cuda")
        check(_lib.wn_perlin_curl_points_vec3(self._h, _ptr(pts), pts.shape[0], kind, int(depth), self._curl_offsets(offsets),
                                              _ptr(out), _stream()))
        return out

    def noise_curl(self, p, offsets=None):
        """The curl of the vector potential whose components are noise() on cells shifted by the whole-cell `offsets`,
        at one point or an (N, 3) batch: v = (d psi2/dy - d psi1/dz, d psi0/dz - d psi2/dx, d psi1/dx - d psi0/dy),
        divergence-free.  float64 input follows noise(double, double, double) (wn_perlin_curl_points), anything else
        noise(const point3&) on floats (wn_perlin_curl_points_vec3).  Every component has the bits of the subtraction
        of two noise_gradient channels at p + o_k wherever that addition is exact."""
        is64 = (p.dtype == torch.float64) if isinstance(p, torch.Tensor) else (np.asarray(p).dtype == np.float64)
        if not is64:
            return self._curl(_dev(p, torch.float32).reshape(-1, 3), _capi.WN_PERLIN_CURL_NOISE, 0, offsets)
        pts = _dev(p, torch.float64).reshape(-1, 3)
        out = torch.empty((pts.shape[0], 3), dtype=torch.float64, device="cuda")
        check(_lib.wn_perlin_curl_points(self._h, _ptr(pts), pts.shape[0], self._curl_offsets(offsets), _ptr(out), _stream()))
        return out

    def turb_curl(self, p, depth=7, offsets=None):
        """noise_curl with the potentials sum_{i<depth} 2^-i noise_k(2^i p): turb's sum before its fabs (the curl of
        |sum| is not divergence-free where the sum is 0).  The offsets are the same in every octave."""
        return self._curl(_dev(p, torch.float32).reshape(-1, 3), _capi.WN_PERLIN_CURL_TURB, depth, offsets)

    def fractal_noise_curl(self, p, offsets=None):
        """noise_curl with fractal_noise potentials (six octaves)."""
        return self._curl(_dev(p, torch.float32).reshape(-1, 3), _capi.WN_PERLIN_CURL_FRACTAL, 0, offsets)

    # -- particles moved through that curl field (include/wnoise_perlin_advect.h; absent from the reference)
    _CURL_KINDS = {"noise": _capi.WN_PERLIN_CURL_NOISE, "turb": _capi.WN_PERLIN_CURL_TURB,
                   "fractal": _capi.WN_PERLIN_CURL_FRACTAL}

    def advect_curl(self, pts, h, steps, kind="noise", depth=7, method="rk4", offsets=None, gain=1.0, drift=None,
                    trajectory_every=0):
        """An (N, 3) batch of particles moved `steps` time steps of size h (negative: backwards) through the velocity
        gain * v + drift, all steps inside the kernel (wn_perlin_curl_advect_points).  kind: "noise" (v = noise_curl at the
        float64 stage point), "turb" (turb_curl with `depth` octaves) or "fractal" (fractal_noise_curl), the last two at the
        stage point rounded to float32.  method: "euler", "midpoint" or "rk4".  Returns the final (N, 3) float64 positions;
        with trajectory_every = e >= 1 also the (steps // e + 1, N, 3) positions after steps 0, e, 2e, ...  Float64 with
        every operation rounded on its own: the bits of stepping with the curl members and separately rounded float64
        tensor operations."""
        methods = WaveletNoise._ADVECT_METHODS
        if method not in methods:
            raise ValueError(f"method: one of {sorted(methods)}")
        if kind not in self._CURL_KINDS:
            raise ValueError(f"kind: one of {sorted(self._CURL_KINDS)}")
        pts = _dev(pts, torch.float64).reshape(-1, 3)
        n, steps, every = pts.shape[0], int(steps), int(trajectory_every)
        a = _capi.wn_advect(methods[method], steps, float(h), float(gain),
                            (C.c_float * 3)(*([0.0] * 3 if drift is None else [float(x) for x in drift])), every)
        out = torch.empty((n, 3), dtype=torch.float64, device="cuda")
        traj = torch.empty((steps // every + 1, n, 3), dtype=torch.float64, device="cuda") if every >= 1 and steps >= 0 else None
        check(_lib.wn_perlin_curl_advect_points(self._h, _ptr(pts), n, self._CURL_KINDS[kind], int(depth),
                                                self._curl_offsets(offsets), C.byref(a), _ptr(out), _ptr(traj), _stream()))
        return out if traj is None else (out, traj)

    # -- that curl field with solid boundaries (include/wnoise_perlin_bounded.h; absent from the reference): the potential
    # values Psi, the bounded velocity, and particles moved through it.  (N, 3) float64 CUDA tensors.
    def _potential(self, pts, kind, depth, offsets):
        out = torch.empty((pts.shape[0], 3), dtype=torch.float64, device="cuda")
        check(_lib.wn_perlin_curl_potential_points_f32(self._h, _ptr(pts), pts.shape[0], kind, int(depth),
                                                        self._curl_offsets(offsets), _ptr(out), _stream()))
        return out

    def noise_potential(self, p, offsets=None):
        """The vector potential Psi = (psi0, psi1, psi2) that noise_curl differentiates: noise() on cells shifted by the
        whole-cell `offsets`.  float64 input follows noise(double, double, double) (wn_perlin_curl_potential_points_f64),
        anything else noise(const point3&) on floats (wn_perlin_curl_potential_points_f32)."""
        is64 = (p.dtype == torch.float64) if isinstance(p, torch.Tensor) else (np.asarray(p).dtype == np.float64)
        if not is64:
            return self._potential(_dev(p, torch.float32).reshape(-1, 3), _capi.WN_PERLIN_CURL_NOISE, 0, offsets)
        pts = _dev(p, torch.float64).reshape(-1, 3)
        out = torch.empty((pts.shape[0], 3), dtype=torch.float64, device="cuda")
        check(_lib.wn_perlin_curl_potential_points_f64(self._h, _ptr(pts), pts.shape[0], self._curl_offsets(offsets), _ptr(out),
                                                   _stream()))
        return out

    def turb_potential(self, p, depth=7, offsets=None):
        """The potential of turb_curl: turb's octave sum before its fabs, per shifted potential."""
        return self._potential(_dev(p, torch.float32).reshape(-1, 3), _capi.WN_PERLIN_CURL_TURB, depth, offsets)

    def fractal_noise_potential(self, p, offsets=None):
        """The potential of fractal_noise_curl: fractal_noise per shifted potential."""
        return self._potential(_dev(p, torch.float32).reshape(-1, 3), _capi.WN_PERLIN_CURL_FRACTAL, 0, offsets)

    def _curl_bounded(self, pts, kind, depth, obstacles, offsets):
        out = torch.empty((pts.shape[0], 3), dtype=torch.float64, device="cuda")
        obs, nobs = WaveletNoise._obstacles(obstacles)
        check(_lib.wn_perlin_curl_bounded_points_f32(self._h, _ptr(pts), pts.shape[0], kind, int(depth),
                                                      self._curl_offsets(offsets), obs, nobs, _ptr(out), _stream()))
        return out

    def noise_curl_bounded(self, p, obstacles, offsets=None):
        """noise_curl with its potential faded to zero towards every solid of `obstacles` (wn_perlin_curl_bounded_points_f64 /
        _points_vec3): v = A curl Psi + grad A x Psi in float64, still divergence-free, with no normal component on a
        solid's surface.  `obstacles`: the list WaveletNoise.evaluate3DCurlBounded takes, in the coordinates of p.  A point
        inside a solid gets 0, a point at distance >= d0 from all of them (and obstacles=[]) the bits of noise_curl."""
        is64 = (p.dtype == torch.float64) if isinstance(p, torch.Tensor) else (np.asarray(p).dtype == np.float64)
        if not is64:
            return self._curl_bounded(_dev(p, torch.float32).reshape(-1, 3), _capi.WN_PERLIN_CURL_NOISE, 0, obstacles, offsets)
        pts = _dev(p, torch.float64).reshape(-1, 3)
        out = torch.empty((pts.shape[0], 3), dtype=torch.float64, device="cuda")
        obs, nobs = WaveletNoise._obstacles(obstacles)
        check(_lib.wn_perlin_curl_bounded_points_f64(self._h, _ptr(pts), pts.shape[0], self._curl_offsets(offsets), obs, nobs,
                                                 _ptr(out), _stream()))
        return out

    def turb_curl_bounded(self, p, obstacles, depth=7, offsets=None):
        """noise_curl_bounded around turb_curl and turb_potential."""
        return self._curl_bounded(_dev(p, torch.float32).reshape(-1, 3), _capi.WN_PERLIN_CURL_TURB, depth, obstacles, offsets)

    def fractal_noise_curl_bounded(self, p, obstacles, offsets=None):
        """noise_curl_bounded around fractal_noise_curl and fractal_noise_potential."""
        return self._curl_bounded(_dev(p, torch.float32).reshape(-1, 3), _capi.WN_PERLIN_CURL_FRACTAL, 0, obstacles, offsets)

    def advect_curl_bounded(self, pts, h, steps, obstacles, kind="noise", depth=7, method="rk4", offsets=None, gain=1.0,
                            drift=None, trajectory_every=0):
        """advect_curl through gain * v + drift with the bounded v of noise_curl_bounded / turb_curl_bounded /
        fractal_noise_curl_bounded, all steps inside the kernel (wn_perlin_curl_bounded_advect_points_f64): particles flow
        around the solids.  A particle inside one moves by drift alone."""
        methods = WaveletNoise._ADVECT_METHODS
        if method not in methods:
            raise ValueError(f"method: one of {sorted(methods)}")
        if kind not in self._CURL_KINDS:
            raise ValueError(f"kind: one of {sorted(self._CURL_KINDS)}")
        obs, nobs = WaveletNoise._obstacles(obstacles)
        pts = _dev(pts, torch.float64).reshape(-1, 3)
        n, steps, every = pts.shape[0], int(steps), int(trajectory_every)
        a = _capi.wn_advect(methods[method], steps, float(h), float(gain),
                            (C.c_float * 3)(*([0.0] * 3 if drift is None else [float(x) for x in drift])), every)
        out = torch.empty((n, 3), dtype=torch.float64, device="cuda")
        traj = torch.empty((steps // every + 1, n, 3), dtype=torch.float64, device="cuda") if every >= 1 and steps >= 0 else None
        check(_lib.wn_perlin_curl_bounded_advect_points_f64(self._h, _ptr(pts), n, self._CURL_KINDS[kind], int(depth),
                                                        self._curl_offsets(offsets), obs, nobs, C.byref(a), _ptr(out),
                                                        _ptr(traj), _stream()))
        return out if traj is None else (out, traj)

    # -- octave limiting by a footprint per sample (absent from the reference; include/wnoise_perlin_footprint.h)
    def _footprint(self, fn, p, s, octaves, bias, fade, channels):
        pts = _dev(p, torch.float32).reshape(-1, 3)
        sd = _dev(s, torch.float32).reshape(-1)
        if sd.shape[0] != pts.shape[0]:
            raise ValueError("s: one footprint per point")
        out = torch.empty((pts.shape[0], channels) if channels > 1 else pts.shape[0], dtype=torch.float64, device="cuda")
        check(fn(self._h, _ptr(pts), _ptr(sd), pts.shape[0], int(octaves), float(bias), int(bool(fade)), _ptr(out), _stream()))
        return out

    def turb_footprint(self, p, s, depth=7, bias=0.0, fade=False):
        """turb(p, depth) with the octaves each sample's footprint can carry (wn_perlin_turb_footprint_points): `s`, one
        per point, is the log2 of the footprint in the noise space of p; octave i runs while (s + bias) + i < 0, and with
        `fade` the finest surviving octave enters with min(1, -t_i).  (N,) float64."""
        return self._footprint(_lib.wn_perlin_turb_footprint_points, p, s, depth, bias, fade, 1)

    def fractal_noise_footprint(self, p, s, octaves=6, bias=0.0, fade=False):
        """fractal_noise over `octaves` octaves, limited per sample as turb_footprint; the normalisation sums all
        `octaves` amplitudes, however many run (wn_perlin_fractal_footprint_points)."""
        return self._footprint(_lib.wn_perlin_fractal_footprint_points, p, s, octaves, bias, fade, 1)

    def turb_footprint_gradient(self, p, s, depth=7, bias=0.0, fade=False):
        """turb_footprint and its gradient: (N, 4) float64 of {value, d/dx, d/dy, d/dz}."""
        return self._footprint(_lib.wn_perlin_turb_footprint_grad_points, p, s, depth, bias, fade, 4)

    def fractal_noise_footprint_gradient(self, p, s, octaves=6, bias=0.0, fade=False):
        """fractal_noise_footprint and its gradient: (N, 4) float64 of {value, d/dx, d/dy, d/dz}."""
        return self._footprint(_lib.wn_perlin_fractal_footprint_grad_points, p, s, octaves, bias, fade, 4)


PerlinNoise = perlin  # experient/PerlinNoise.hpp is the same algorithm with an explicit seed


# ---- textures (texture.h) --------------------------------------------------------------------
class noise_texture:
    def __init__(self, scale, octave=4):
        self.noise = perlin()  # default-seeded member (texture.h:46)
        self.scale, self.octave_level = float(scale), int(octave)

    def grey(self, p, active=None, out=None):
        pts = _dev(p, torch.float32).reshape(-1, 3)
        if out is None:
            out = torch.zeros(pts.shape[0], dtype=torch.float32, device="cuda")
        act = _dev(active, torch.uint8) if active is not None else None
        check(_lib.wn_noise_texture_points(self.noise._h, self.scale, self.octave_level, _ptr(pts),
                                           _ptr(act), pts.shape[0], _ptr(out), _stream()))
        return out

    def value(self, u, v, p):
        if _is_scalar_point(p, 3):  # the reference's call shape: one request to the resident scalar kernel
            a = (C.c_float * 3)(*[float(x) for x in (p.tolist() if hasattr(p, "tolist") else p)])
            out = C.c_float(0)
            check(_lib.wn_scalar_noise_texture(self.noise._h, self.scale, self.octave_level, a, C.byref(out)))
            return (out.value,) * 3
        g = self.grey(p)
        return g[:, None].expand(-1, 3)


class wavelet_texture:
    def __init__(self, scale=1.0, octave=4, use_3d=True):
        self.scale, self.octave_level, self.use_3d_noise = float(scale), int(octave), bool(use_3d)
        TILE_SIZE, SEED = 128, 12345  # texture.h:55-56
        self.noise_2d = WaveletNoise(TILE_SIZE, SEED)
        self.noise_2d.generateNoiseTile2D()
        self.noise_3d = None
        if self.use_3d_noise:
            self.noise_3d = WaveletNoise(TILE_SIZE, SEED)
            self.noise_3d.generateNoiseTile3D()

    def grey(self, p, active=None, out=None):
        pts = _dev(p, torch.float32).reshape(-1, 3)
        if out is None:
            out = torch.zeros(pts.shape[0], dtype=torch.float32, device="cuda")
        act = _dev(active, torch.uint8) if active is not None else None
        use3d = self.use_3d_noise and self.noise_3d is not None
        src = self.noise_3d if use3d else self.noise_2d
        check(_lib.wn_wavelet_texture_points(src._handle(3 if use3d else 2), int(use3d), self.scale,
                                             self.octave_level, _ptr(pts), _ptr(act), pts.shape[0],
                                             _ptr(out), _stream()))
        return out

    def value(self, u, v, p):
        if _is_scalar_point(p, 3):
            use3d = self.use_3d_noise and self.noise_3d is not None
            src = self.noise_3d if use3d else self.noise_2d
            a = (C.c_float * 3)(*[float(x) for x in (p.tolist() if hasattr(p, "tolist") else p)])
            out = C.c_float(0)
            check(_lib.wn_scalar_wavelet_texture(src._handle(3 if use3d else 2), int(use3d), self.scale,
                                                 self.octave_level, a, C.byref(out)))
            return (out.value,) * 3
        g = self.grey(p)
        return g[:, None].expand(-1, 3)


class wavelet_multiband_texture:
    """WMultibandNoise as a texture, band-limited by each hit's footprint (absent from the reference;
    wn_wavelet_multiband_texture_points): pos = (float)(p * scale), n = WMultibandNoise(pos, s, firstBand, nbands, w),
    grey = 0.5 * (1 + clamp(n / 4, -1, 1)).  `s`: log2 of the hit's footprint in noise space (after scale)."""

    def __init__(self, scale, firstBand, nbands, w, variance=0.18402, fade=True):
        self.scale, self.firstBand, self.nbands = float(scale), int(firstBand), int(nbands)
        self.w = [float(x) for x in list(w)[:self.nbands]]
        self.variance, self.fade = float(variance), bool(fade)
        self.default_footprint = -math.inf  # value(): all bands
        self.noise_3d = WaveletNoise(128, 12345)  # wavelet_texture's tile (texture.h:55-56)
        self.noise_3d.generateNoiseTile3D()

    def grey(self, p, s, active=None, out=None):
        pts = _dev(p, torch.float32).reshape(-1, 3)
        sd = _dev(s, torch.float32).reshape(-1)
        if sd.shape[0] != pts.shape[0]:
            raise ValueError("s: one footprint per point")
        if out is None:
            out = torch.zeros(pts.shape[0], dtype=torch.float32, device="cuda")
        act = _dev(active, torch.uint8) if active is not None else None
        wa = (C.c_float * max(1, self.nbands))(*self.w)
        check(_lib.wn_wavelet_multiband_texture_points(self.noise_3d._handle(3), self.scale, self.firstBand, self.nbands, wa,
                                                       self.variance, int(self.fade), _ptr(pts), _ptr(sd), _ptr(act),
                                                       pts.shape[0], _ptr(out), _stream()))
        return out

    def value(self, u, v, p):
        """One point: a 3-tuple at the default footprint; an (N, 3) batch: (N, 3), every point at the default footprint."""
        pts = _dev(p, torch.float32).reshape(-1, 3)
        g = self.grey(pts, torch.full((pts.shape[0],), self.default_footprint, dtype=torch.float32, device="cuda"))
        if _is_scalar_point(p, 3):
            return (float(g.item()),) * 3
        return g[:, None].expand(-1, 3)


class noise_multiband_texture:
    """fractal_noise as a texture, octave-limited by each hit's footprint (absent from the reference;
    wn_noise_multiband_texture_points): pos = (float)scale * p, n = fractal_noise over `octaves` octaves of which octave i
    runs while (s + bias) + i < 0, grey = 0.5 * (1 + n).  `s`: log2 of the hit's footprint in noise space (after scale)."""

    def __init__(self, scale, octaves=6, bias=0.0, fade=True):
        self.noise = perlin()  # default-seeded member, as noise_texture
        self.scale, self.octaves, self.bias, self.fade = float(scale), int(octaves), float(bias), bool(fade)
        self.default_footprint = -math.inf  # value(): all octaves

    def grey(self, p, s, active=None, out=None):
        pts = _dev(p, torch.float32).reshape(-1, 3)
        sd = _dev(s, torch.float32).reshape(-1)
        if sd.shape[0] != pts.shape[0]:
            raise ValueError("s: one footprint per point")
        if out is None:
            out = torch.zeros(pts.shape[0], dtype=torch.float32, device="cuda")
        act = _dev(active, torch.uint8) if active is not None else None
        check(_lib.wn_noise_multiband_texture_points(self.noise._h, self.scale, self.octaves, self.bias, int(self.fade),
                                                     _ptr(pts), _ptr(sd), _ptr(act), pts.shape[0], _ptr(out), _stream()))
        return out

    def value(self, u, v, p):
        """One point: a 3-tuple at the default footprint; an (N, 3) batch: (N, 3), every point at the default footprint."""
        pts = _dev(p, torch.float32).reshape(-1, 3)
        g = self.grey(pts, torch.full((pts.shape[0],), self.default_footprint, dtype=torch.float32, device="cuda"))
        if _is_scalar_point(p, 3):
            return (float(g.item()),) * 3
        return g[:, None].expand(-1, 3)


# ---- dense grids (experient/main.cpp) -----------------------------------------------------------
@dataclass
class GridSpec:
    den: int
    nx: int
    ny: int
    z0: int = 0
    z1: int = 1
    base_range: float = 4.0          # experient/main.cpp:13
    octave_scale: float = 1.0
    post_scale: float = 1.0
    z_mode: int = WN_Z_LATTICE
    z_const: float = 0.0
    out_scale: float = 1.0
    flags: int = WN_GRID_DEFAULT

    def c(self):
        return wn_grid(self.den, self.nx, self.ny, self.z0, self.z1, self.base_range,
                       self.octave_scale, self.post_scale, self.z_mode, self.z_const,
                       self.out_scale, self.flags)

    @property
    def nz(self):
        return 1 if self.z_mode == WN_Z_CONST else self.z1 - self.z0

    def empty(self, out=None):
        n = self.nz * self.ny * self.nx
        if out is None:
            return torch.empty(n, dtype=torch.float32, device="cuda")
        assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= n
        return out


def _f32(x):
    return float(np.float32(x))


def _inv_stddev(var):
    return _f32(np.float32(1.0) / np.sqrt(np.float32(var)))  # 1.0f / std::sqrt(0.18402f)


def _octave_scale(octave):
    return _f32(math.pow(2.0, octave))  # std::pow(2.0f, octave) -> float


def _write(t, outputFile):
    if outputFile:
        t.cpu().numpy().astype("<f4").tofile(outputFile)  # raw float32, experient/main.cpp:32-34


def generate2DOctaveBandNoise(imageSize, octave, outputFile, noise, flags=WN_GRID_EXACT):
    g = GridSpec(imageSize, imageSize, imageSize, octave_scale=_octave_scale(octave), post_scale=2.0,
                 out_scale=_inv_stddev(0.19686), flags=flags)
    out = g.empty()
    gc = g.c()
    check(_lib.wn_eval2d_grid(noise._handle(2), C.byref(gc), _ptr(out), _stream()))
    out = out.view(imageSize, imageSize)
    _write(out, outputFile)
    return out


def _multiband2d_image(fn, planes, noise, image_size, s, firstBand, nbands, w, variance, den, out):
    """[planes, ny, nx] from one launch of a wn_multiband2d_*grid entry point; image_size: an int or (nx, ny)."""
    nx, ny = (int(image_size),) * 2 if np.ndim(image_size) == 0 else (int(image_size[0]), int(image_size[1]))
    w = [1.0] * nbands if w is None else list(w)
    g = GridSpec(nx if den is None else int(den), nx, ny)
    n = planes * ny * nx
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device="cuda")
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= n
    gc = g.c()
    wa = (C.c_float * max(1, nbands))(*[float(x) for x in w[:nbands]])
    check(fn(noise._handle(2), C.byref(gc), float(s), int(firstBand), int(nbands), wa, float(variance), _ptr(out), _stream()))
    return out[:n].view(planes, ny, nx)


def generate2DMultibandNoise(noise, image_size, s=-16.0, firstBand=0, nbands=5, w=None, variance=0.19686, den=None,
                             outputFile=None, out=None):
    """A fractal 2-D image in one launch (wn_multiband2d_grid): WMultibandNoise with evaluate2D bands at p = (i/den)*4 on
    both axes (generate2DOctaveBandNoise's lattice before its octave scaling), [ny, nx].  image_size: an int (a square
    image) or (nx, ny); den defaults to nx; w to unit weights; outputFile: the raw float32 format of the other generators."""
    img = _multiband2d_image(_lib.wn_multiband2d_grid, 1, noise, image_size, s, firstBand, nbands, w, variance, den, out)[0]
    _write(img, outputFile)
    return img


def generate2DMultibandNoiseGradient(noise, image_size, s=-16.0, firstBand=0, nbands=5, w=None, variance=0.19686,
                                     den=None, out=None):
    """generate2DMultibandNoise with the gradient with respect to p (wn_multiband2d_grad_grid): [3, ny, nx] -- value, d/dx,
    d/dy; the value plane has the bits of generate2DMultibandNoise."""
    return _multiband2d_image(_lib.wn_multiband2d_grad_grid, 3, noise, image_size, s, firstBand, nbands, w, variance, den,
                              out)


def generate2DMultibandNoiseCurl(noise, image_size, s=-16.0, firstBand=0, nbands=5, w=None, variance=0.19686, den=None,
                                 out=None):
    """The curl of generate2DMultibandNoise's stream function on its lattice (wn_multiband2d_curl_grid): [2, ny, nx] -- vx =
    d/dy and vy = -d/dx of generate2DMultibandNoiseGradient, the same bits but for vy's sign."""
    return _multiband2d_image(_lib.wn_multiband2d_curl_grid, 2, noise, image_size, s, firstBand, nbands, w, variance, den,
                              out)


def generate2DMultibandNoiseCurlBounded(noise, image_size, obstacles, s=-16.0, firstBand=0, nbands=5, w=None, variance=0.19686,
                                        den=None, out=None, flow=None):
    """generate2DMultibandNoiseCurl with solid boundaries and a background stream (wn_multiband2d_curl_bounded_grid):
    [2, ny, nx].  `obstacles` and `flow` as WaveletNoise.WMultibandNoise2DCurlBounded, in the lattice's coordinate
    p = (i/den)*4."""
    obs, nobs, fl = WaveletNoise._bounds2d(obstacles, flow)
    return _multiband2d_image(lambda tile, g, s_, first, nb, wa, var, o, st: _lib.wn_multiband2d_curl_bounded_grid(
        tile, g, s_, first, nb, wa, var, obs, nobs, fl, o, st), 2, noise, image_size, s, firstBand, nbands, w, variance, den, out)


def generate3DSlicedOctaveBandNoise(imageSize, octave, outputFile, noise, flags=WN_GRID_EXACT, out=None):
    """Byte-identical to the reference's file by default (WN_GRID_EXACT); flags=WN_GRID_DEFAULT opts in
    to the separable brick kernel (within 1e-5).  `out`: a flat float32 CUDA tensor to write into, as the volume helpers."""
    g = GridSpec(imageSize, imageSize, imageSize, octave_scale=_octave_scale(octave), post_scale=2.0,
                 z_mode=WN_Z_CONST, z_const=2.0, out_scale=_inv_stddev(0.18402), flags=flags)
    out = g.empty(out)
    gc = g.c()
    check(_lib.wn_eval3d_grid(noise._handle(3), C.byref(gc), _ptr(out), _stream()))
    out = out[: imageSize * imageSize].view(imageSize, imageSize)
    _write(out, outputFile)
    return out


def generate3DProjectedOctaveBandNoise(imageSize, octave, outputFile, noise, normal=(0.0, 0.0, 1.0)):
    g = GridSpec(imageSize, imageSize, imageSize, octave_scale=_octave_scale(octave), post_scale=2.0,
                 z_mode=WN_Z_CONST, z_const=2.0, out_scale=_inv_stddev(0.296))
    out = g.empty()
    gc = g.c()
    nr = (C.c_float * 3)(*[float(v) for v in normal])
    check(_lib.wn_eval3d_projected_grid(noise._handle(3), C.byref(gc), nr, _ptr(out), _stream()))
    out = out.view(imageSize, imageSize)
    _write(out, outputFile)
    return out


def generatePerlinNoise2D(imageSize, octave, outputFile, perlin_obj):
    g = GridSpec(imageSize, imageSize, imageSize, octave_scale=_octave_scale(octave),
                 z_mode=WN_Z_CONST, z_const=0.0)
    out = g.empty()
    gc = g.c()
    check(_lib.wn_perlin_grid(perlin_obj._h, C.byref(gc), _ptr(out), _stream()))
    out = out.view(imageSize, imageSize)
    _write(out, outputFile)
    return out


def generatePerlinNoise3DSliced(imageSize, octave, outputFile, perlin_obj):
    os_ = _octave_scale(octave)
    g = GridSpec(imageSize, imageSize, imageSize, octave_scale=os_, z_mode=WN_Z_CONST,
                 z_const=_f32(np.float32(1.0) * np.float32(os_)))
    out = g.empty()
    gc = g.c()
    check(_lib.wn_perlin_grid(perlin_obj._h, C.byref(gc), _ptr(out), _stream()))
    out = out.view(imageSize, imageSize)
    _write(out, outputFile)
    return out


# ---- volumes ---------------------------------------------------------
def wavelet_volume(noise, den, nx, ny, z0, z1, octave, exact=False, out=None):
    """Config 2/5: q = ((i/den)*4)*2^octave*2 on all three axes, evaluate3D(q)/sqrt(0.18402)."""
    g = GridSpec(den, nx, ny, z0, z1, octave_scale=_octave_scale(octave), post_scale=2.0,
                 out_scale=_inv_stddev(0.18402), flags=WN_GRID_EXACT if exact else WN_GRID_DEFAULT)
    out = g.empty(out)
    gc = g.c()
    check(_lib.wn_eval3d_grid(noise._handle(3), C.byref(gc), _ptr(out), _stream()))
    return out[: g.nz * ny * nx].view(g.nz, ny, nx)


def wavelet_volume_launcher(noise, den, nx, ny, z0, z1, octave, out, exact=False):
    """The same call as wavelet_volume with its arguments marshalled once: returns launch(), one kernel launch into
    `out` on the stream that is current NOW (for long back-to-back runs, where a few tens of microseconds of
    argument handling per call would sit beside a 100 us kernel)."""
    g = GridSpec(den, nx, ny, z0, z1, octave_scale=_octave_scale(octave), post_scale=2.0,
                 out_scale=_inv_stddev(0.18402), flags=WN_GRID_EXACT if exact else WN_GRID_DEFAULT)
    out = g.empty(out)
    gc, h, p, st, fn = g.c(), noise._handle(3), _ptr(out), _stream(), _lib.wn_eval3d_grid
    ref = C.byref(gc)

    def launch():
        rc = fn(h, ref, p, st)
        if rc:
            check(rc)
    launch.keep = (gc, noise, out)
    return launch


def multiband_volume(noise, den, nx, ny, z0, z1, s=-16.0, firstBand=0, nbands=5, w=None,
                     variance=0.18402, exact=False, out=None):
    """Config 3(A): WMultibandNoise(p=(i/den)*4, s, NULL, firstBand, nbands, w)."""
    w = [1.0] * nbands if w is None else list(w)
    g = GridSpec(den, nx, ny, z0, z1, flags=WN_GRID_EXACT if exact else WN_GRID_DEFAULT)
    out = g.empty(out)
    gc = g.c()
    wa = (C.c_float * max(1, nbands))(*[float(x) for x in w[:nbands]])
    check(_lib.wn_multiband3d_grid(noise._handle(3), C.byref(gc), float(s), int(firstBand),
                                   int(nbands), wa, float(variance), _ptr(out), _stream()))
    return out[: g.nz * ny * nx].view(g.nz, ny, nx)


# ---- sparse brick lists (include/wnoise_bricks.h) ---------------------------------------------------
def _bricks_args(den, bricks, bounds, out, ch=1):
    """The (n, 3) int32 device list, (nx, ny, z0, z1) -- `den` on each axis by default, as the generators do -- and the
    (n, 8, 8, 8) output, indexed [brick][z][y][x]; `ch` such arrays one after the other for the derivative fields."""
    if not (isinstance(bricks, torch.Tensor) and bricks.is_cuda and bricks.dtype == torch.int32 and bricks.dim() == 2
            and bricks.shape[1] == 3 and bricks.is_contiguous()):
        raise ValueError("bricks must be a contiguous (n, 3) int32 CUDA tensor of (bx, by, bz)")
    nx, ny, z0, z1 = (den, den, 0, den) if bounds is None else (int(v) for v in bounds)
    n = bricks.shape[0]
    edge = _capi.WN_BRICK
    if out is None:
        out = torch.empty((ch * n, edge, edge, edge), dtype=torch.float32, device="cuda")
    elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == ch * n * edge ** 3):
        raise ValueError("out must be a contiguous float32 CUDA tensor of %sn * 512 elements" % ("" if ch == 1 else f"{ch} * "))
    return n, (nx, ny, z0, z1), out


def wavelet_bricks(noise, den, bricks, octave, bounds=None, exact=False, out=None):
    """wavelet_volume on the listed 8^3 bricks of the lattice only: brick (bx, by, bz) holds the samples
    [8bz, 8bz+8) x [8by, 8by+8) x [8bx, 8bx+8) of wavelet_volume(noise, den, ...), as out[i][z][y][x].  Bricks outside
    `bounds` are left untouched (with out=None their contents are undefined)."""
    n, (nx, ny, z0, z1), out = _bricks_args(den, bricks, bounds, out)
    g = GridSpec(den, nx, ny, z0, z1, octave_scale=_octave_scale(octave), post_scale=2.0,
                 out_scale=_inv_stddev(0.18402), flags=WN_GRID_EXACT if exact else WN_GRID_DEFAULT)
    gc = g.c()
    check(_lib.wn_eval3d_bricks(noise._handle(3), C.byref(gc), _ptr(bricks), n, _ptr(out), _stream()))
    return out.view(n, _capi.WN_BRICK, _capi.WN_BRICK, _capi.WN_BRICK)


def multiband_bricks(noise, den, bricks, s=-16.0, firstBand=0, nbands=5, w=None, variance=0.18402, bounds=None,
                     exact=False, out=None):
    """multiband_volume on the listed 8^3 bricks of the lattice only, laid out as wavelet_bricks."""
    w = [1.0] * nbands if w is None else list(w)
    n, (nx, ny, z0, z1), out = _bricks_args(den, bricks, bounds, out)
    g = GridSpec(den, nx, ny, z0, z1, flags=WN_GRID_EXACT if exact else WN_GRID_DEFAULT)
    gc = g.c()
    wa = (C.c_float * max(1, nbands))(*[float(x) for x in w[:nbands]])
    check(_lib.wn_multiband3d_bricks(noise._handle(3), C.byref(gc), _ptr(bricks), n, float(s), int(firstBand),
                                     int(nbands), wa, float(variance), _ptr(out), _stream()))
    return out.view(n, _capi.WN_BRICK, _capi.WN_BRICK, _capi.WN_BRICK)


# ---- gradient and curl brick lists (include/wnoise_brick_fields.h) ------------------------------------
def _brick_fields_view(out, ch, n):
    return out.view(ch, n, _capi.WN_BRICK, _capi.WN_BRICK, _capi.WN_BRICK)


def wavelet_gradient_bricks(noise, den, bricks, octave, bounds=None, exact=False, out=None):
    """wavelet_gradient_volume on the listed 8^3 bricks only (wn_eval3d_grad_bricks): (4, n, 8, 8, 8) -- value, d/dx,
    d/dy, d/dz as out[channel][i][z][y][x]; list, bounds and untouched bricks as wavelet_bricks."""
    n, (nx, ny, z0, z1), out = _bricks_args(den, bricks, bounds, out, 4)
    g = GridSpec(den, nx, ny, z0, z1, octave_scale=_octave_scale(octave), post_scale=2.0,
                 out_scale=_inv_stddev(0.18402), flags=WN_GRID_EXACT if exact else WN_GRID_DEFAULT)
    gc = g.c()
    check(_lib.wn_eval3d_grad_bricks(noise._handle(3), C.byref(gc), _ptr(bricks), n, _ptr(out), _stream()))
    return _brick_fields_view(out, 4, n)


def multiband_gradient_bricks(noise, den, bricks, s=-16.0, firstBand=0, nbands=5, w=None, variance=0.18402, bounds=None,
                              exact=False, out=None):
    """multiband_gradient_volume on the listed 8^3 bricks only (wn_multiband3d_grad_bricks): (4, n, 8, 8, 8)."""
    w = [1.0] * nbands if w is None else list(w)
    n, (nx, ny, z0, z1), out = _bricks_args(den, bricks, bounds, out, 4)
    g = GridSpec(den, nx, ny, z0, z1, flags=WN_GRID_EXACT if exact else WN_GRID_DEFAULT)
    gc = g.c()
    wa = (C.c_float * max(1, nbands))(*[float(x) for x in w[:nbands]])
    check(_lib.wn_multiband3d_grad_bricks(noise._handle(3), C.byref(gc), _ptr(bricks), n, float(s), int(firstBand),
                                          int(nbands), wa, float(variance), _ptr(out), _stream()))
    return _brick_fields_view(out, 4, n)


def curl_bricks(noise, den, bricks, octave, offsets=None, bounds=None, exact=False, out=None):
    """curl_volume on the listed 8^3 bricks only (wn_eval3d_curl_bricks; `offsets` as WaveletNoise.evaluate3DCurl):
    (3, n, 8, 8, 8) -- vx, vy, vz as out[component][i][z][y][x]."""
    n, (nx, ny, z0, z1), out = _bricks_args(den, bricks, bounds, out, 3)
    g = GridSpec(den, nx, ny, z0, z1, octave_scale=_octave_scale(octave), post_scale=2.0,
                 out_scale=_inv_stddev(0.18402), flags=WN_GRID_EXACT if exact else WN_GRID_DEFAULT)
    gc = g.c()
    check(_lib.wn_eval3d_curl_bricks(noise._handle(3), C.byref(gc), _ptr(bricks), n, noise._curl_offsets(offsets), _ptr(out),
                                     _stream()))
    return _brick_fields_view(out, 3, n)


def multiband_curl_bricks(noise, den, bricks, s=-16.0, firstBand=0, nbands=5, w=None, variance=0.18402, offsets=None,
                          bounds=None, exact=False, out=None):
    """multiband_curl_volume on the listed 8^3 bricks only (wn_multiband3d_curl_bricks): (3, n, 8, 8, 8)."""
    w = [1.0] * nbands if w is None else list(w)
    n, (nx, ny, z0, z1), out = _bricks_args(den, bricks, bounds, out, 3)
    g = GridSpec(den, nx, ny, z0, z1, flags=WN_GRID_EXACT if exact else WN_GRID_DEFAULT)
    gc = g.c()
    wa = (C.c_float * max(1, nbands))(*[float(x) for x in w[:nbands]])
    check(_lib.wn_multiband3d_curl_bricks(noise._handle(3), C.byref(gc), _ptr(bricks), n, noise._curl_offsets(offsets),
                                          float(s), int(firstBand), int(nbands), wa, float(variance), _ptr(out), _stream()))
    return _brick_fields_view(out, 3, n)


# ---- curl brick lists with solid boundaries (include/wnoise_bounded_bricks.h) --------------------------
def curl_bounded_bricks(noise, den, bricks, octave, obstacles, offsets=None, bounds=None, exact=False, out=None):
    """curl_bricks with its potential faded to zero towards every solid of `obstacles` (wn_eval3d_curl_bounded_bricks):
    (3, n, 8, 8, 8).  `obstacles` as WaveletNoise.evaluate3DCurlBounded takes them, in the samples' noise-space coordinates
    ((i / den) * 4 * 2^octave * 2); a sample inside a solid gets 0, one at distance >= d0 from all of them (and
    obstacles=[]) the bits of curl_bricks."""
    n, (nx, ny, z0, z1), out = _bricks_args(den, bricks, bounds, out, 3)
    g = GridSpec(den, nx, ny, z0, z1, octave_scale=_octave_scale(octave), post_scale=2.0,
                 out_scale=_inv_stddev(0.18402), flags=WN_GRID_EXACT if exact else WN_GRID_DEFAULT)
    gc = g.c()
    obs, nobs = noise._obstacles(obstacles)
    check(_lib.wn_eval3d_curl_bounded_bricks(noise._handle(3), C.byref(gc), _ptr(bricks), n, noise._curl_offsets(offsets),
                                             obs, nobs, _ptr(out), _stream()))
    return _brick_fields_view(out, 3, n)


def multiband_curl_bounded_bricks(noise, den, bricks, obstacles, s=-16.0, firstBand=0, nbands=5, w=None, variance=0.18402,
                                  offsets=None, bounds=None, exact=False, out=None):
    """multiband_curl_bricks with the solids of `obstacles` (wn_multiband3d_curl_bounded_bricks): (3, n, 8, 8, 8); the
    obstacles live in the lattice coordinate p = (i / den) * 4."""
    w = [1.0] * nbands if w is None else list(w)
    n, (nx, ny, z0, z1), out = _bricks_args(den, bricks, bounds, out, 3)
    g = GridSpec(den, nx, ny, z0, z1, flags=WN_GRID_EXACT if exact else WN_GRID_DEFAULT)
    gc = g.c()
    wa = (C.c_float * max(1, nbands))(*[float(x) for x in w[:nbands]])
    obs, nobs = noise._obstacles(obstacles)
    check(_lib.wn_multiband3d_curl_bounded_bricks(noise._handle(3), C.byref(gc), _ptr(bricks), n, noise._curl_offsets(offsets),
                                                  float(s), int(firstBand), int(nbands), wa, float(variance), obs, nobs,
                                                  _ptr(out), _stream()))
    return _brick_fields_view(out, 3, n)


def _grad_out(g, out):
    n = 4 * g.nz * g.ny * g.nx
    if out is None:
        return torch.empty(n, dtype=torch.float32, device="cuda")
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= n
    return out


def wavelet_gradient_volume(noise, den, nx, ny, z0, z1, octave, exact=False, out=None):
    """wavelet_volume's lattice with the gradient (wn_eval3d_grad_grid): [4, nz, ny, nx] -- value, d/dx, d/dy, d/dz
    with respect to the coordinate passed to evaluate3D, all four times 1/sqrt(0.18402)."""
    g = GridSpec(den, nx, ny, z0, z1, octave_scale=_octave_scale(octave), post_scale=2.0,
                 out_scale=_inv_stddev(0.18402), flags=WN_GRID_EXACT if exact else WN_GRID_DEFAULT)
    out = _grad_out(g, out)
    gc = g.c()
    check(_lib.wn_eval3d_grad_grid(noise._handle(3), C.byref(gc), _ptr(out), _stream()))
    return out[: 4 * g.nz * ny * nx].view(4, g.nz, ny, nx)


def multiband_gradient_volume(noise, den, nx, ny, z0, z1, s=-16.0, firstBand=0, nbands=5, w=None,
                              variance=0.18402, exact=False, out=None):
    """multiband_volume's lattice with the gradient with respect to p = (i/den)*4 (wn_multiband3d_grad_grid):
    [4, nz, ny, nx]."""
    w = [1.0] * nbands if w is None else list(w)
    g = GridSpec(den, nx, ny, z0, z1, flags=WN_GRID_EXACT if exact else WN_GRID_DEFAULT)
    out = _grad_out(g, out)
    gc = g.c()
    wa = (C.c_float * max(1, nbands))(*[float(x) for x in w[:nbands]])
    check(_lib.wn_multiband3d_grad_grid(noise._handle(3), C.byref(gc), float(s), int(firstBand),
                                        int(nbands), wa, float(variance), _ptr(out), _stream()))
    return out[: 4 * g.nz * ny * nx].view(4, g.nz, ny, nx)


def _curl_out(g, out):
    n = 3 * g.nz * g.ny * g.nx
    if out is None:
        return torch.empty(n, dtype=torch.float32, device="cuda")
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= n
    return out


def curl_volume(noise, den, nx, ny, z0, z1, octave, offsets=None, exact=False, out=None):
    """wavelet_gradient_volume's lattice with the curl of the three shifted potentials (wn_eval3d_curl_grid; `offsets` as
    WaveletNoise.evaluate3DCurl): [3, nz, ny, nx] -- vx, vy, vz, derivatives with respect to the coordinate passed to
    evaluate3D, all three times 1/sqrt(0.18402)."""
    g = GridSpec(den, nx, ny, z0, z1, octave_scale=_octave_scale(octave), post_scale=2.0,
                 out_scale=_inv_stddev(0.18402), flags=WN_GRID_EXACT if exact else WN_GRID_DEFAULT)
    out = _curl_out(g, out)
    gc = g.c()
    check(_lib.wn_eval3d_curl_grid(noise._handle(3), C.byref(gc), noise._curl_offsets(offsets), _ptr(out), _stream()))
    return out[: 3 * g.nz * ny * nx].view(3, g.nz, ny, nx)


def multiband_curl_volume(noise, den, nx, ny, z0, z1, s=-16.0, firstBand=0, nbands=5, w=None, variance=0.18402,
                          offsets=None, exact=False, out=None):
    """multiband_gradient_volume's lattice with the curl of three shifted WMultibandNoise potentials, derivatives with
    respect to p = (i/den)*4 (wn_multiband3d_curl_grid): [3, nz, ny, nx]."""
    w = [1.0] * nbands if w is None else list(w)
    g = GridSpec(den, nx, ny, z0, z1, flags=WN_GRID_EXACT if exact else WN_GRID_DEFAULT)
    out = _curl_out(g, out)
    gc = g.c()
    wa = (C.c_float * max(1, nbands))(*[float(x) for x in w[:nbands]])
    check(_lib.wn_multiband3d_curl_grid(noise._handle(3), C.byref(gc), noise._curl_offsets(offsets), float(s),
                                        int(firstBand), int(nbands), wa, float(variance), _ptr(out), _stream()))
    return out[: 3 * g.nz * ny * nx].view(3, g.nz, ny, nx)


def wavelet2d_gradient_image(noise, den, nx, ny, octave, out=None):
    """generate2DOctaveBandNoise's lattice with the gradient (wn_eval2d_grad_grid): [3, ny, nx] -- value, d/dx, d/dy
    with respect to the coordinate passed to evaluate2D, all three times 1/sqrt(0.19686)."""
    g = GridSpec(den, nx, ny, octave_scale=_octave_scale(octave), post_scale=2.0, out_scale=_inv_stddev(0.19686))
    n = 3 * ny * nx
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device="cuda")
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= n
    gc = g.c()
    check(_lib.wn_eval2d_grad_grid(noise._handle(2), C.byref(gc), _ptr(out), _stream()))
    return out[:n].view(3, ny, nx)


def projected_gradient_volume(noise, den, nx, ny, z0, z1, octave, normal=(0.0, 0.0, 1.0), out=None):
    """wavelet_volume's lattice through evaluate3DProjected with one normal, and the gradient with respect to the
    coordinate passed to it (wn_eval3d_projected_grad_grid): [4, nz, ny, nx], all four times 1/sqrt(0.296)."""
    g = GridSpec(den, nx, ny, z0, z1, octave_scale=_octave_scale(octave), post_scale=2.0, out_scale=_inv_stddev(0.296))
    out = _grad_out(g, out)
    gc = g.c()
    nr = (C.c_float * 3)(*[float(v) for v in normal])
    check(_lib.wn_eval3d_projected_grad_grid(noise._handle(3), C.byref(gc), nr, _ptr(out), _stream()))
    return out[: 4 * g.nz * ny * nx].view(4, g.nz, ny, nx)


def perlin_volume(perlin_obj, den, nx, ny, z0, z1, octave, out=None):
    g = GridSpec(den, nx, ny, z0, z1, octave_scale=_octave_scale(octave))
    out = g.empty(out)
    gc = g.c()
    check(_lib.wn_perlin_grid(perlin_obj._h, C.byref(gc), _ptr(out), _stream()))
    return out[: g.nz * ny * nx].view(g.nz, ny, nx)


def turb_volume(perlin_obj, den, nx, ny, z0, z1, depth=7, out=None):
    """Config 3(B): turb(p=(i/den)*4, depth)."""
    g = GridSpec(den, nx, ny, z0, z1)
    out = g.empty(out)
    gc = g.c()
    check(_lib.wn_perlin_turb_grid(perlin_obj._h, C.byref(gc), int(depth), _ptr(out), _stream()))
    return out[: g.nz * ny * nx].view(g.nz, ny, nx)


def perlin_gradient_volume(perlin_obj, den, nx, ny, z0, z1, octave, out=None):
    """perlin_volume's lattice with the gradient (wn_perlin_grad_grid): [4, nz, ny, nx] -- value, d/dx, d/dy, d/dz with
    respect to the coordinate passed to noise()."""
    g = GridSpec(den, nx, ny, z0, z1, octave_scale=_octave_scale(octave))
    out = _grad_out(g, out)
    gc = g.c()
    check(_lib.wn_perlin_grad_grid(perlin_obj._h, C.byref(gc), _ptr(out), _stream()))
    return out[: 4 * g.nz * ny * nx].view(4, g.nz, ny, nx)


def turb_gradient_volume(perlin_obj, den, nx, ny, z0, z1, depth=7, out=None):
    """turb_volume's lattice with the gradient with respect to p = (i/den)*4 (wn_perlin_turb_grad_grid):
    [4, nz, ny, nx]."""
    g = GridSpec(den, nx, ny, z0, z1)
    out = _grad_out(g, out)
    gc = g.c()
    check(_lib.wn_perlin_turb_grad_grid(perlin_obj._h, C.byref(gc), int(depth), _ptr(out), _stream()))
    return out[: 4 * g.nz * ny * nx].view(4, g.nz, ny, nx)


_PERLIN_CURL_KINDS = {"noise": _capi.WN_PERLIN_CURL_NOISE, "turb": _capi.WN_PERLIN_CURL_TURB,
                      "fractal": _capi.WN_PERLIN_CURL_FRACTAL}


def perlin_curl_volume(perlin_obj, den, nx, ny, z0, z1, octave, kind="noise", depth=7, offsets=None, out=None):
    """perlin_volume's lattice p = (i/den)*4 * 2^octave (octave 0: turb_volume's) with the curl of three shifted Perlin
    potentials (wn_perlin_curl_grid; `kind`: "noise", "turb" with `depth`, "fractal"; `offsets` as perlin.noise_curl):
    [3, nz, ny, nx] -- vx, vy, vz, derivatives with respect to p."""
    g = GridSpec(den, nx, ny, z0, z1, octave_scale=_octave_scale(octave))
    out = _curl_out(g, out)
    gc = g.c()
    check(_lib.wn_perlin_curl_grid(perlin_obj._h, C.byref(gc), _PERLIN_CURL_KINDS[kind], int(depth),
                                   perlin._curl_offsets(offsets), _ptr(out), _stream()))
    return out[: 3 * g.nz * ny * nx].view(3, g.nz, ny, nx)


# ---- sparse brick lists of Perlin noise (include/wnoise_perlin_bricks.h) ---------------------------------
def _perlin_bricks(fn, perlin_obj, den, bricks, octave, bounds, out, ch, *mid):
    """One wn_perlin_*_bricks call on perlin_volume's lattice p = (i/den)*4 * 2^octave (octave 0: turb_volume's); `mid`:
    the arguments between the grid and the list."""
    n, (nx, ny, z0, z1), out = _bricks_args(den, bricks, bounds, out, ch)
    gc = GridSpec(den, nx, ny, z0, z1, octave_scale=_octave_scale(octave)).c()
    check(fn(perlin_obj._h, C.byref(gc), *mid, _ptr(bricks), n, _ptr(out), _stream()))
    edge = _capi.WN_BRICK
    return out.view(n, edge, edge, edge) if ch == 1 else _brick_fields_view(out, ch, n)


def perlin_bricks(perlin_obj, den, bricks, octave, bounds=None, out=None):
    """perlin_volume on the listed 8^3 bricks of the lattice only (wn_perlin_bricks): brick (bx, by, bz) holds the samples
    [8bz, 8bz+8) x [8by, 8by+8) x [8bx, 8bx+8) of perlin_volume(perlin_obj, den, ...), as out[i][z][y][x], bit for bit.
    Bricks outside `bounds` (nx, ny, z0, z1; `den` on each axis by default) are left untouched."""
    return _perlin_bricks(_lib.wn_perlin_bricks, perlin_obj, den, bricks, octave, bounds, out, 1)


def turb_bricks(perlin_obj, den, bricks, depth=7, octave=0, bounds=None, out=None):
    """turb_volume on the listed bricks only (wn_perlin_turb_bricks): turb(p = (i/den)*4 * 2^octave, depth)."""
    return _perlin_bricks(_lib.wn_perlin_turb_bricks, perlin_obj, den, bricks, octave, bounds, out, 1, int(depth))


def fractal_bricks(perlin_obj, den, bricks, octave=0, bounds=None, out=None):
    """fractal_noise(p = (i/den)*4 * 2^octave) on the listed bricks only (wn_perlin_fractal_bricks)."""
    return _perlin_bricks(_lib.wn_perlin_fractal_bricks, perlin_obj, den, bricks, octave, bounds, out, 1)


def perlin_gradient_bricks(perlin_obj, den, bricks, octave, bounds=None, out=None):
    """perlin_gradient_volume on the listed bricks only (wn_perlin_grad_bricks): (4, n, 8, 8, 8) -- value, d/dx, d/dy,
    d/dz as out[channel][i][z][y][x]."""
    return _perlin_bricks(_lib.wn_perlin_grad_bricks, perlin_obj, den, bricks, octave, bounds, out, 4)


def turb_gradient_bricks(perlin_obj, den, bricks, depth=7, octave=0, bounds=None, out=None):
    """turb_gradient_volume on the listed bricks only (wn_perlin_turb_grad_bricks): (4, n, 8, 8, 8)."""
    return _perlin_bricks(_lib.wn_perlin_turb_grad_bricks, perlin_obj, den, bricks, octave, bounds, out, 4, int(depth))


def fractal_gradient_bricks(perlin_obj, den, bricks, octave=0, bounds=None, out=None):
    """fractal_noise with its gradient on the listed bricks only (wn_perlin_fractal_grad_bricks): (4, n, 8, 8, 8)."""
    return _perlin_bricks(_lib.wn_perlin_fractal_grad_bricks, perlin_obj, den, bricks, octave, bounds, out, 4)


def perlin_curl_bricks(perlin_obj, den, bricks, octave, kind="noise", depth=7, offsets=None, bounds=None, out=None):
    """perlin_curl_volume on the listed bricks only (wn_perlin_curl_bricks; `kind`, `depth` and `offsets` as there):
    (3, n, 8, 8, 8) -- vx, vy, vz as out[component][i][z][y][x]."""
    return _perlin_bricks(_lib.wn_perlin_curl_bricks, perlin_obj, den, bricks, octave, bounds, out, 3,
                          _PERLIN_CURL_KINDS[kind], int(depth), perlin._curl_offsets(offsets))


# ---- Perlin curl brick lists with solid boundaries (include/wnoise_perlin_bounded_bricks.h) ---------------
def perlin_curl_bounded_bricks(perlin_obj, den, bricks, octave, obstacles, kind="noise", depth=7, offsets=None, bounds=None,
                               out=None):
    """perlin_curl_bricks with its potential faded to zero towards every solid of `obstacles`
    (wn_perlin_curl_bounded_bricks): (3, n, 8, 8, 8).  `obstacles` as perlin.noise_curl_bounded takes them, in the samples'
    coordinates p = (i / den) * 4 * 2^octave; a sample inside a solid gets 0, one at distance >= d0 from all of them (and
    obstacles=[]) the bits of perlin_curl_bricks, every other sample (float) of perlin.noise_curl_bounded /
    turb_curl_bounded / fractal_noise_curl_bounded at its float coordinates."""
    obs, nobs = WaveletNoise._obstacles(obstacles)
    return _perlin_bricks(_lib.wn_perlin_curl_bounded_bricks, perlin_obj, den, bricks, octave, bounds, out, 3,
                          _PERLIN_CURL_KINDS[kind], int(depth), perlin._curl_offsets(offsets), obs, nobs)
