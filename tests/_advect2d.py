"""What the 2-D advection tests share (tests/test_curl2d_host.py, tests/test_gpu_curl2d.py): the time steps of
include/wnoise_curl2d.h written out in numpy float32, one separately rounded operation per statement, around any velocity
function -- tests/_advect.py's step, whose statements are whole-array operations and so hold for (N, 2) positions as they
stand; the cases; and the host's wnhost_multiband2d_curl_advect through ctypes."""
import ctypes as C
import os

import numpy as np

import _advect as A3
import _ref64_curl2d as R

PKG = A3.PKG
FP = A3.FP
f32 = np.float32

EULER, MIDPOINT, RK4 = A3.EULER, A3.MIDPOINT, A3.RK4
METHOD_NAMES = A3.METHOD_NAMES
DRIFT = (0.1, -0.2)
ZERO = (0.0, 0.0)
# (method, steps, h, gain, drift): every method with steps 0, 1 and 3, both signs of h, both gains, with and without drift
CASES = [(m, n, h, g, DRIFT if d != A3.ZERO else ZERO) for m, n, h, g, d in A3.CASES]
CASE_IDS = A3.CASE_IDS


class wn_advect2d(C.Structure):
    """include/wnoise_curl2d.h"""
    _fields_ = [("method", C.c_int32), ("steps", C.c_int32), ("h", C.c_float), ("gain", C.c_float),
                ("drift", C.c_float * 2), ("traj_every", C.c_int32)]


def advect_struct(method, steps, h, gain, drift, every=0):
    return wn_advect2d(method, steps, h, gain, (C.c_float * 2)(*drift), every)


def points(seed=41):
    """300 points uniform in (-300, 300)^2 and 50 more on half-integer knots, where a spline's mid flips."""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-300.0, 300.0, (350, 2)).astype(f32)
    pts[300:] = np.floor(pts[300:]) + f32(0.5)
    return pts


def step_f32(method, p, h, gain, drift, velocity):
    """One step of (N, 2) float32 positions; velocity(q) -> (N, 2) float32.  Every statement is one float32 operation."""
    assert p.ndim == 2 and p.shape[1] == 2 and len(drift) == 2
    return A3.step_f32(method, p, h, gain, drift, velocity)


def trace_f32(method, steps, p, h, gain, drift, velocity):
    """The positions after steps 0, 1, ..., steps: a list of (N, 2) float32 arrays."""
    path = [np.ascontiguousarray(p, f32)]
    for _ in range(steps):
        path.append(step_f32(method, path[-1], h, gain, drift, velocity))
    return path


def load_host():
    path = os.path.join(PKG, "libwnoise_host.so")
    if not os.path.exists(path):
        import __graft_entry__
        __graft_entry__.build()
    lib = R.bind_host(C.CDLL(path))
    lib.wnhost_multiband2d_curl_advect.restype = C.c_int   # AttributeError: the library has no 2-D advection
    lib.wnhost_multiband2d_curl_advect.argtypes = [FP, C.c_int, FP, C.c_float, C.c_int, C.c_int, FP, C.c_float,
                                                   C.POINTER(wn_advect2d), FP, FP]
    return lib


def host_advect(host, coef, pts, bands, adv):
    """wnhost_multiband2d_curl_advect on every point; bands = (s, first_band, nbands, w, var_per_band).  The final (N, 2)
    positions and the (S, N, 2) trajectory (None when adv.traj_every == 0)."""
    s, first, nb, w, var = bands
    cp, n, _keep = R.tile_args(coef)
    wa = (C.c_float * max(1, nb))(*[float(x) for x in w[:nb]])
    pts = np.ascontiguousarray(pts, f32)
    out = np.empty((len(pts), 2), f32)
    snaps = adv.steps // adv.traj_every + 1 if adv.traj_every else 0
    traj = np.empty((len(pts), max(snaps, 1), 2), f32)
    for i in range(len(pts)):
        rc = host.wnhost_multiband2d_curl_advect(cp, n, pts[i].ctypes.data_as(FP), float(s), first, nb, wa, var, C.byref(adv),
                                                 out[i].ctypes.data_as(FP), traj[i].ctypes.data_as(FP) if snaps else None)
        assert rc == 0, rc
    return out, (np.ascontiguousarray(traj.transpose(1, 0, 2)) if snaps else None)
