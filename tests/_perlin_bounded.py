"""What the Perlin boundary tests share (tests/test_perlin_bounded_host.py, tests/test_gpu_perlin_bounded.py): the obstacle
ramp and the bounded velocity of include/wnoise_perlin_bounded.h written out in numpy float64, one separately rounded
operation per statement, around any curl and any potential-value function -- the float64 twin of tests/_bounded.py, whose
obstacle sets and wn_obstacle it uses; tests/_perlin_advect.py's points, kinds, offsets and trace; and the host's
wnhost_perlin_*curl_potential / wnhost_perlin_curl_bounded / wnhost_perlin_curl_bounded_advect through ctypes.

An obstacle is the tuple the Python members take: ("sphere", c, r, d0), ("container", c, r, d0) or ("halfspace", n, o, d0);
its numbers are floats in the C ABI, so they enter the arithmetic as float32 values widened to float64."""
import ctypes as C

import numpy as np

import _bounded as B
import _perlin_advect as PA

f32, f64 = np.float32, np.float64
FP, DP, IP, OP = PA.FP, PA.DP, PA.IP, B.OP
FAR, NEAR, INSIDE = B.FAR, B.NEAR, B.INSIDE
SETS, THREE, obstacle_array = B.SETS, B.THREE, B.obstacle_array
NOISE, TURB, FRACTAL = PA.NOISE, PA.TURB, PA.FRACTAL
KINDS, KIND_IDS, OFFSET_SETS = PA.KINDS, PA.KIND_IDS, PA.OFFSET_SETS
points, trace_f64 = PA.points, PA.trace_f64
ZERO_OFFSETS = ((0, 0, 0), (0, 0, 0), (0, 0, 0))


def widen(v):
    return np.asarray(v, f32).astype(f64)


# ---- the arithmetic, one float64 operation per statement -------------------------------------------------------------------
def distance_f64(obstacle, x):
    """d (N,) and nrm (N, 3) of one obstacle at the (N, 3) float64 points x."""
    kind, c, r, _ = obstacle
    c, r = widen(c), widen(r)
    if kind == "halfspace":
        t0 = c[0] * x[:, 0]
        t1 = c[1] * x[:, 1]
        t2 = c[2] * x[:, 2]
        s = t0 + t1
        s = s + t2
        d = s - r
        return d, np.broadcast_to(c, x.shape)
    dx = x - c
    q0 = dx[:, 0] * dx[:, 0]
    q1 = dx[:, 1] * dx[:, 1]
    q2 = dx[:, 2] * dx[:, 2]
    l2 = q0 + q1
    l2 = l2 + q2
    ln = np.sqrt(l2)
    assert ln.dtype == f64
    with np.errstate(divide="ignore", invalid="ignore"):
        m = dx / ln[:, None]
    m = np.where(ln[:, None] == 0, f64(0.0), m)
    if kind == "sphere":
        return ln - r, m
    return r - ln, -m


def ramp_f64(obstacles, x):
    """where (N,) in {FAR, NEAR, INSIDE}, A (N,) and G (N, 3): the running product over the near obstacles in list order."""
    x = np.ascontiguousarray(x)
    assert x.dtype == f64
    n = len(x)
    Ar, G = np.ones(n, f64), np.zeros((n, 3), f64)
    inside, near = np.zeros(n, bool), np.zeros(n, bool)
    for ob in obstacles:
        d0 = widen(ob[3])
        d, nrm = distance_f64(ob, x)
        inside |= d <= 0
        act = ~(d >= d0)
        near |= act
        r = d / d0
        r2 = r * r
        t = r2 * f64(0.375)
        t = f64(-1.25) + t
        t = r2 * t
        t = f64(1.875) + t
        alpha = r * t
        q = f64(1.0) - r2
        qq = q * q
        t = f64(1.875) * qq
        dalpha = t / d0
        ad = Ar * dalpha
        g1 = G * alpha[:, None]
        g2 = ad[:, None] * nrm
        gn = g1 + g2
        an = Ar * alpha
        assert gn.dtype == f64 and an.dtype == f64
        G = np.where(act[:, None], gn, G)
        Ar = np.where(act, an, Ar)
    where = np.where(inside, INSIDE, np.where(near, NEAR, FAR))
    return where, Ar, G


def velocity_f64(where, Ar, G, c, psi):
    """v = A c + G x Psi at the near points, c at the far ones, +0 inside."""
    out = np.array(c, f64)
    for k in range(3):
        a, b = (k + 1) % 3, (k + 2) % 3
        t1 = G[:, a] * psi[:, b]
        t2 = G[:, b] * psi[:, a]
        x = t1 - t2
        t = Ar * c[:, k]
        v = t + x
        assert v.dtype == f64
        out[:, k] = np.where(where == NEAR, v, c[:, k])
    out[where == INSIDE] = 0.0
    return out


def compose_f64(obstacles, x, curl, values):
    """The bounded velocity at the (N, 3) float64 points x -- the points the evaluator receives, a float point widened --
    from curl(x) -> (N, 3) float64, the unbounded entry point, and values(x) -> (N, 3) float64, the potential values."""
    x = np.ascontiguousarray(x)
    assert x.dtype == f64
    where, Ar, G = ramp_f64(obstacles, x)
    c, psi = curl(x), values(x)
    assert c.dtype == f64 and psi.dtype == f64
    return velocity_f64(where, Ar, G, c, psi)


def received(kind, q):
    """The point the evaluator of `kind` receives for the float64 point q, as float64: q itself (noise), (float)q widened."""
    q = np.ascontiguousarray(q, f64)
    return q if kind == NOISE else q.astype(f32).astype(f64)


# ---- the host library --------------------------------------------------------------------------------------------------------
def load_host():
    lib = PA.load_host()
    for name, args in (("wnhost_perlin_curl_potential", [IP, C.c_double, C.c_double, C.c_double, IP, DP]),   # AttributeError:
                       ("wnhost_perlin_turb_curl_potential", [IP, FP, C.c_int, IP, DP]),                     # no Perlin boundaries
                       ("wnhost_perlin_fractal_curl_potential", [IP, FP, IP, DP])):
        getattr(lib, name).restype = None
        getattr(lib, name).argtypes = args
    lib.wnhost_perlin_curl_bounded.restype = C.c_int
    lib.wnhost_perlin_curl_bounded.argtypes = [IP, C.c_int, C.c_int, DP, IP, OP, C.c_int, DP]
    lib.wnhost_perlin_curl_bounded_advect.restype = C.c_int
    lib.wnhost_perlin_curl_bounded_advect.argtypes = [IP, C.c_int, C.c_int, DP, IP, OP, C.c_int, C.POINTER(PA.wn_advect), DP, DP]
    for name, args in (("wnhost_perlin", [IP, C.c_double, C.c_double, C.c_double]), ("wnhost_perlin_fractal", [IP, FP]),
                       ("wnhost_perlin_turb", [IP, FP, C.c_int])):
        getattr(lib, name).restype = C.c_double
        getattr(lib, name).argtypes = args
    return lib


def host_potential(host, perm, kind, depth, offsets):
    """values(q) from the host's potential functions: noise at the float64 point, turb and fractal_noise at
    q.astype(np.float32)."""
    pp, off = perm.ctypes.data_as(IP), PA._offsets(offsets)
    op = off.ctypes.data_as(IP)

    def values(q):
        assert q.dtype == f64
        out = np.empty((len(q), 3), f64)
        v = np.zeros(3, f64)
        vp = v.ctypes.data_as(DP)
        q32 = np.ascontiguousarray(q.astype(f32))
        for i, (x, y, z) in enumerate(q.tolist()):
            if kind == NOISE:
                host.wnhost_perlin_curl_potential(pp, x, y, z, op, vp)
            elif kind == TURB:
                host.wnhost_perlin_turb_curl_potential(pp, q32[i].ctypes.data_as(FP), depth, op, vp)
            else:
                host.wnhost_perlin_fractal_curl_potential(pp, q32[i].ctypes.data_as(FP), op, vp)
            out[i] = v
        return out
    return values


def host_scalar(host, perm, kind, depth):
    """value(q) -> (N,) from the host's noise (at the float64 point), turb and fractal_noise (at q.astype(np.float32))."""
    pp = perm.ctypes.data_as(IP)

    def value(q):
        q32 = np.ascontiguousarray(q.astype(f32))
        if kind == NOISE:
            return np.array([host.wnhost_perlin(pp, x, y, z) for x, y, z in q.tolist()], f64)
        if kind == TURB:
            return np.array([host.wnhost_perlin_turb(pp, q32[i].ctypes.data_as(FP), depth) for i in range(len(q))], f64)
        return np.array([host.wnhost_perlin_fractal(pp, q32[i].ctypes.data_as(FP)) for i in range(len(q))], f64)
    return value


def host_bounded(host, perm, kind, depth, offsets, obstacles):
    """velocity(q) from wnhost_perlin_curl_bounded, which takes the float64 point for every kind."""
    pp, off = perm.ctypes.data_as(IP), PA._offsets(offsets)
    arr = obstacle_array(obstacles)

    def velocity(q):
        q = np.ascontiguousarray(q, f64)
        out = np.empty((len(q), 3), f64)
        for i in range(len(q)):
            rc = host.wnhost_perlin_curl_bounded(pp, kind, depth, q[i].ctypes.data_as(DP), off.ctypes.data_as(IP), arr,
                                                 len(obstacles), out[i].ctypes.data_as(DP))
            assert rc == 0, rc
        return out
    return velocity


def host_bounded_advect(host, perm, kind, depth, pts, offsets, obstacles, adv):
    """wnhost_perlin_curl_bounded_advect on every point: the final (N, 3) positions and the (S, N, 3) trajectory (None when
    adv.traj_every == 0)."""
    pp, off = perm.ctypes.data_as(IP), PA._offsets(offsets)
    arr = obstacle_array(obstacles)
    pts = np.ascontiguousarray(pts, f64)
    out = np.empty((len(pts), 3), f64)
    snaps = adv.steps // adv.traj_every + 1 if adv.traj_every else 0
    traj = np.empty((len(pts), max(snaps, 1), 3), f64)
    for i in range(len(pts)):
        rc = host.wnhost_perlin_curl_bounded_advect(pp, kind, depth, pts[i].ctypes.data_as(DP), off.ctypes.data_as(IP), arr,
                                                    len(obstacles), C.byref(adv), out[i].ctypes.data_as(DP),
                                                    traj[i].ctypes.data_as(DP) if snaps else None)
        assert rc == 0, rc
    return out, (np.ascontiguousarray(traj.transpose(1, 0, 2)) if snaps else None)
