"""What the Perlin advection tests share (tests/test_perlin_advect_host.py, tests/test_gpu_perlin_advect.py): the time steps
of include/wnoise_perlin_advect.h written out in numpy float64, one separately rounded operation per statement, around any
velocity function; the cases (tests/_advect.py's); the float64 point set; and the host's wnhost_perlin_curl /
wnhost_perlin_turb_curl / wnhost_perlin_fractal_curl / wnhost_perlin_curl_advect through ctypes."""
import ctypes as C
import os

import numpy as np

import _advect as A

ROOT, PKG = A.ROOT, A.PKG
FP, DP, IP = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int)
f64 = np.float64

NOISE, TURB, FRACTAL = 0, 1, 2
EULER, MIDPOINT, RK4 = A.EULER, A.MIDPOINT, A.RK4
METHOD_NAMES, DRIFT, ZERO = A.METHOD_NAMES, A.DRIFT, A.ZERO
CASES, CASE_IDS = A.CASES, A.CASE_IDS
wn_advect, advect_struct = A.wn_advect, A.advect_struct
# (kind, depth): noise, turb without an octave, with one and with seven, fractal_noise
KINDS = [(NOISE, 0), (TURB, 0), (TURB, 1), (TURB, 7), (FRACTAL, 0)]
KIND_IDS = ["noise", "turb0", "turb1", "turb7", "fractal"]
KIND_NAMES = {NOISE: "noise", TURB: "turb", FRACTAL: "fractal"}
# the library's default, and offsets that are negative and >= 256
DEFAULT_OFFSETS = ((0, 0, 0), (85, 85, 85), (170, 170, 170))
OFFSET_SETS = {"default": DEFAULT_OFFSETS, "wide": ((-3, 260, 7), (511, -129, 1000), (2, -300, 255))}


def points(seed=43):
    """350 float64 points: 300 uniform in (-300, 300); 25 on integers, where the fractional part is 0; 25 at
    nextafter(k, -inf) for integers k: those doubles lie in cell k - 1 and their float rounding is k, in cell k, so they
    tell an evaluation at q from one at (float)q."""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-300.0, 300.0, (350, 3))
    pts[300:325] = rng.integers(-300, 301, (25, 3)).astype(f64)
    k = rng.integers(-300, 301, (25, 3)).astype(f64)
    pts[325:] = np.nextafter(k, -np.inf)
    assert pts.dtype == f64
    assert (np.floor(pts[325:]) == k - 1).all() and (pts[325:].astype(np.float32).astype(f64) == k).all()
    return pts


def step_f64(method, p, h, gain, drift, velocity):
    """One step of (N, 3) float64 positions; velocity(q) -> (N, 3) float64 receives the float64 stage points (for turb and
    fractal_noise it rounds them with .astype(np.float32) itself).  h, gain and drift are floats widened to float64, as
    wn_advect carries them.  Every statement is one float64 operation."""
    h, gain, drift = f64(np.float32(h)), f64(np.float32(gain)), np.asarray(drift, np.float32).astype(f64)
    h2 = f64(0.5) * h
    h6 = h / f64(6.0)
    assert p.dtype == f64 and h2.dtype == f64 and h6.dtype == f64 and drift.dtype == f64

    def k(q):
        assert q.dtype == f64
        v = velocity(q)
        assert v.dtype == f64
        t = gain * v
        return t + drift

    def from_p(f, kk):
        t = f * kk
        return p + t

    k1 = k(p)
    if method == EULER:
        out = from_p(h, k1)
    elif method == MIDPOINT:
        out = from_p(h, k(from_p(h2, k1)))
    else:
        k2 = k(from_p(h2, k1))
        k3 = k(from_p(h2, k2))
        k4 = k(from_p(h, k3))
        t2 = f64(2.0) * k2
        s = k1 + t2
        t3 = f64(2.0) * k3
        s = s + t3
        s = s + k4
        out = from_p(h6, s)
    assert out.dtype == f64
    return out


def trace_f64(method, steps, p, h, gain, drift, velocity):
    """The positions after steps 0, 1, ..., steps: a list of (N, 3) float64 arrays."""
    path = [np.ascontiguousarray(p, f64)]
    for _ in range(steps):
        path.append(step_f64(method, path[-1], h, gain, drift, velocity))
    return path


def load_host():
    path = os.path.join(PKG, "libwnoise_host.so")
    if not os.path.exists(path):
        import __graft_entry__
        __graft_entry__.build()
    lib = C.CDLL(path)
    for name, args in (("wnhost_perlin_curl", [IP, C.c_double, C.c_double, C.c_double, IP, DP]),
                       ("wnhost_perlin_turb_curl", [IP, FP, C.c_int, IP, DP]),
                       ("wnhost_perlin_fractal_curl", [IP, FP, IP, DP])):
        getattr(lib, name).restype = None
        getattr(lib, name).argtypes = args
    lib.wnhost_perlin_curl_advect.restype = C.c_int   # AttributeError: the library has no Perlin advection
    lib.wnhost_perlin_curl_advect.argtypes = [IP, C.c_int, C.c_int, DP, IP, C.POINTER(wn_advect), DP, DP]
    return lib


def perm_table(seed):
    """The 512-entry table of perlin(seed) (wn_perlin_permutation is a host helper: no device needed)."""
    hip = C.CDLL(os.path.join(PKG, "libwnoise_hip.so"))
    p = np.zeros(512, np.int32)
    assert hip.wn_perlin_permutation(C.c_uint32(seed), p.ctypes.data_as(C.c_void_p)) == 0
    return p


def _offsets(offsets):
    return np.ascontiguousarray(np.asarray(offsets, np.int32).reshape(9))


def host_velocity(host, perm, kind, depth, offsets):
    """velocity(q) for trace_f64 from the host's point evaluators: noise at the float64 point, turb and fractal_noise at
    q.astype(np.float32)."""
    pp, off = perm.ctypes.data_as(IP), _offsets(offsets)
    op = off.ctypes.data_as(IP)

    def velocity(q):
        assert q.dtype == f64
        out = np.empty((len(q), 3), f64)
        v = np.zeros(3, f64)
        vp = v.ctypes.data_as(DP)
        if kind == NOISE:
            for i, (x, y, z) in enumerate(q.tolist()):
                host.wnhost_perlin_curl(pp, x, y, z, op, vp)
                out[i] = v
            return out
        q32 = np.ascontiguousarray(q.astype(np.float32))
        for i in range(len(q32)):
            if kind == TURB:
                host.wnhost_perlin_turb_curl(pp, q32[i].ctypes.data_as(FP), depth, op, vp)
            else:
                host.wnhost_perlin_fractal_curl(pp, q32[i].ctypes.data_as(FP), op, vp)
            out[i] = v
        return out
    return velocity


def host_advect(host, perm, kind, depth, pts, offsets, adv):
    """wnhost_perlin_curl_advect on every point: the final (N, 3) positions and the (S, N, 3) trajectory (None when
    adv.traj_every == 0)."""
    pp, off = perm.ctypes.data_as(IP), _offsets(offsets)
    pts = np.ascontiguousarray(pts, f64)
    out = np.empty((len(pts), 3), f64)
    snaps = adv.steps // adv.traj_every + 1 if adv.traj_every else 0
    traj = np.empty((len(pts), max(snaps, 1), 3), f64)
    for i in range(len(pts)):
        rc = host.wnhost_perlin_curl_advect(pp, kind, depth, pts[i].ctypes.data_as(DP), off.ctypes.data_as(IP), C.byref(adv),
                                            out[i].ctypes.data_as(DP), traj[i].ctypes.data_as(DP) if snaps else None)
        assert rc == 0, rc
    return out, (np.ascontiguousarray(traj.transpose(1, 0, 2)) if snaps else None)
