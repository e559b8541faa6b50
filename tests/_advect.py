"""What the advection tests share (tests/test_advect_host.py, tests/test_gpu_advect.py): the time steps of
include/wnoise_advect.h written out in numpy float32, one separately rounded operation per statement, around any velocity
function; the cases; and the host's wnhost_eval3d_curl / wnhost_eval3d_curl_advect through ctypes."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "wavelet-noise-in-ray-tracing_amd")
FP = C.POINTER(C.c_float)
IP = C.POINTER(C.c_int32)
f32 = np.float32

EULER, MIDPOINT, RK4 = 0, 1, 2
METHOD_NAMES = {EULER: "euler", MIDPOINT: "midpoint", RK4: "rk4"}
DRIFT = (0.1, -0.2, 0.05)
ZERO = (0.0, 0.0, 0.0)
# (method, steps, h, gain, drift): every method with steps 0, 1 and 3, both signs of h, both gains, with and without drift
CASES = [
    (EULER, 0, 0.37, 1.0, ZERO),
    (EULER, 1, 0.37, 1.0, ZERO),
    (EULER, 3, -0.37, 0.75, DRIFT),
    (EULER, 3, 0.37, 1.0, DRIFT),
    (MIDPOINT, 0, -0.37, 1.0, DRIFT),
    (MIDPOINT, 1, 0.37, 0.75, ZERO),
    (MIDPOINT, 3, 0.37, 1.0, DRIFT),
    (MIDPOINT, 3, -0.37, 0.75, ZERO),
    (RK4, 0, 0.37, 0.75, DRIFT),
    (RK4, 1, 0.37, 1.0, ZERO),
    (RK4, 1, -0.37, 0.75, DRIFT),
    (RK4, 3, 0.37, 1.0, DRIFT),
    (RK4, 3, -0.37, 0.75, ZERO),
    (RK4, 3, 0.37, 0.75, DRIFT),
]
CASE_IDS = [f"{METHOD_NAMES[m]}_{n}_h{h}_g{g}_{'drift' if d != ZERO else 'still'}" for m, n, h, g, d in CASES]


class wn_advect(C.Structure):
    """include/wnoise_advect.h"""
    _fields_ = [("method", C.c_int32), ("steps", C.c_int32), ("h", C.c_float), ("gain", C.c_float),
                ("drift", C.c_float * 3), ("traj_every", C.c_int32)]


def advect_struct(method, steps, h, gain, drift, every=0):
    return wn_advect(method, steps, h, gain, (C.c_float * 3)(*drift), every)


def points(seed=41):
    """300 points uniform in (-300, 300) and 50 more on half-integer knots, where a spline's mid flips."""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-300.0, 300.0, (350, 3)).astype(f32)
    pts[300:] = np.floor(pts[300:]) + f32(0.5)
    return pts


def step_f32(method, p, h, gain, drift, velocity):
    """One step of (N, 3) float32 positions; velocity(q) -> (N, 3) float32.  Every statement is one float32 operation."""
    h, gain, drift = f32(h), f32(gain), np.asarray(drift, f32)
    h2 = f32(0.5) * h
    h6 = h / f32(6.0)
    assert p.dtype == f32 and h2.dtype == f32 and h6.dtype == f32

    def k(q):
        v = velocity(q)
        assert v.dtype == f32
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
        t2 = f32(2.0) * k2
        s = k1 + t2
        t3 = f32(2.0) * k3
        s = s + t3
        s = s + k4
        out = from_p(h6, s)
    assert out.dtype == f32
    return out


def trace_f32(method, steps, p, h, gain, drift, velocity):
    """The positions after steps 0, 1, ..., steps: a list of (N, 3) float32 arrays."""
    path = [np.ascontiguousarray(p, f32)]
    for _ in range(steps):
        path.append(step_f32(method, path[-1], h, gain, drift, velocity))
    return path


def load_host():
    path = os.path.join(PKG, "libwnoise_host.so")
    if not os.path.exists(path):
        import __graft_entry__
        __graft_entry__.build()
    lib = C.CDLL(path)
    lib.wnhost_eval3d_curl.restype = None
    lib.wnhost_eval3d_curl.argtypes = [FP, C.c_int, FP, IP, FP]
    lib.wnhost_eval3d_curl_advect.restype = C.c_int   # AttributeError: the library has no advection
    lib.wnhost_eval3d_curl_advect.argtypes = [FP, C.c_int, FP, IP, C.POINTER(wn_advect), FP, FP]
    return lib


def _tile(coef):
    coef = np.ascontiguousarray(coef, f32).reshape(-1)
    n = int(round(coef.size ** (1.0 / 3.0))) if coef.size else 0
    assert n ** 3 == coef.size
    return coef, n, (coef.ctypes.data_as(FP) if coef.size else None)


def host_curl(host, coef, pts, offsets):
    coef, n, cp = _tile(coef)
    off = np.ascontiguousarray(np.asarray(offsets, np.int32).reshape(9))
    pts = np.ascontiguousarray(pts, f32)
    out = np.empty((len(pts), 3), f32)
    for i in range(len(pts)):
        host.wnhost_eval3d_curl(cp, n, pts[i].ctypes.data_as(FP), off.ctypes.data_as(IP), out[i].ctypes.data_as(FP))
    return out


def host_advect(host, coef, pts, offsets, adv):
    """wnhost_eval3d_curl_advect on every point: the final (N, 3) positions and the (S, N, 3) trajectory (None when
    adv.traj_every == 0)."""
    coef, n, cp = _tile(coef)
    off = np.ascontiguousarray(np.asarray(offsets, np.int32).reshape(9))
    pts = np.ascontiguousarray(pts, f32)
    out = np.empty((len(pts), 3), f32)
    snaps = adv.steps // adv.traj_every + 1 if adv.traj_every else 0
    traj = np.empty((len(pts), max(snaps, 1), 3), f32)
    for i in range(len(pts)):
        rc = host.wnhost_eval3d_curl_advect(cp, n, pts[i].ctypes.data_as(FP), off.ctypes.data_as(IP), C.byref(adv),
                                            out[i].ctypes.data_as(FP), traj[i].ctypes.data_as(FP) if snaps else None)
        assert rc == 0, rc
    return out, (np.ascontiguousarray(traj.transpose(1, 0, 2)) if snaps else None)
