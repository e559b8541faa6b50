"""What the boundary tests share (tests/test_bounded_host.py, tests/test_gpu_bounded.py): the obstacle ramp and the bounded
velocity of include/wnoise_bounded.h written out in numpy float32, one separately rounded operation per statement, around
any curl and any potential-value function; the obstacle sets; and the host's wnhost_eval3d_curl_bounded /
wnhost_eval3d_curl_bounded_advect through ctypes.

An obstacle is the tuple the Python members take: ("sphere", c, r, d0), ("container", c, r, d0) or ("halfspace", n, o, d0)."""
import ctypes as C

import numpy as np

import _advect as A

f32 = np.float32
FP, IP = A.FP, A.IP
KINDS = {"sphere": 0, "container": 1, "halfspace": 2}
FAR, NEAR, INSIDE = 0, 1, 2


class wn_obstacle(C.Structure):
    """include/wnoise_bounded.h"""
    _fields_ = [("kind", C.c_int32), ("c", C.c_float * 3), ("r", C.c_float), ("d0", C.c_float), ("reserved", C.c_int32 * 2)]


OP = C.POINTER(wn_obstacle)


def obstacle_array(obstacles):
    arr = (wn_obstacle * max(1, len(obstacles)))()
    for dst, (kind, c, r, d0) in zip(arr, obstacles):
        dst.kind, dst.c, dst.r, dst.d0 = KINDS[kind], (C.c_float * 3)(*c), r, d0
    return arr


# ---- the obstacle sets of the tests, at the scale of A.points(): coordinates in (-300, 300) -------------------------------
SPHERE = ("sphere", (0.0, 0.0, 0.0), 120.0, 80.0)
GROUND = ("halfspace", (0.0, 1.0, 0.0), -250.0, 100.0)        # fluid where y > -250
CONTAINER = ("container", (0.0, 0.0, 0.0), 500.0, 150.0)
THREE = [SPHERE, GROUND, CONTAINER]                             # the ramps of the ground and the container overlap


def sixteen(seed=5):
    """16 obstacles: THREE, a ground plane with a normal that is not a unit vector, and 12 small spheres."""
    rng = np.random.default_rng(seed)
    out = THREE + [("halfspace", (0.5, 0.0, 2.0), -600.0, 90.0)]
    for _ in range(12):
        c = rng.uniform(-250.0, 250.0, 3)
        out.append(("sphere", tuple(float(f32(v)) for v in c), float(f32(rng.uniform(20.0, 50.0))),
                    float(f32(rng.uniform(30.0, 70.0)))))
    return out


SETS = {"none": [], "sphere": [SPHERE], "three": THREE, "sixteen": sixteen()}


# ---- the arithmetic, one float32 operation per statement -------------------------------------------------------------------
def distance_f32(obstacle, x):
    """d (N,) and nrm (N, 3) of one obstacle at the (N, 3) float32 points x."""
    kind, c, r, _ = obstacle
    c, r = np.asarray(c, f32), f32(r)
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
    assert ln.dtype == f32
    with np.errstate(divide="ignore", invalid="ignore"):
        m = dx / ln[:, None]
    m = np.where(ln[:, None] == 0, f32(0.0), m)
    if kind == "sphere":
        return ln - r, m
    return r - ln, -m


def ramp_f32(obstacles, x):
    """where (N,) in {FAR, NEAR, INSIDE}, A (N,) and G (N, 3): the running product over the near obstacles in list order."""
    x = np.ascontiguousarray(x, f32)
    n = len(x)
    Ar, G = np.ones(n, f32), np.zeros((n, 3), f32)
    inside, near = np.zeros(n, bool), np.zeros(n, bool)
    for ob in obstacles:
        d0 = f32(ob[3])
        d, nrm = distance_f32(ob, x)
        inside |= d <= 0
        act = ~(d >= d0)
        near |= act
        r = d / d0
        r2 = r * r
        t = r2 * f32(0.375)
        t = f32(-1.25) + t
        t = r2 * t
        t = f32(1.875) + t
        alpha = r * t
        q = f32(1.0) - r2
        qq = q * q
        t = f32(1.875) * qq
        dalpha = t / d0
        ad = Ar * dalpha
        g1 = G * alpha[:, None]
        g2 = ad[:, None] * nrm
        gn = g1 + g2
        an = Ar * alpha
        assert gn.dtype == f32 and an.dtype == f32
        G = np.where(act[:, None], gn, G)
        Ar = np.where(act, an, Ar)
    where = np.where(inside, INSIDE, np.where(near, NEAR, FAR))
    return where, Ar, G


def velocity_f32(where, Ar, G, c, psi):
    """v = A c + G x Psi at the near points, c at the far ones, 0 inside."""
    out = np.array(c, f32)
    for k in range(3):
        a, b = (k + 1) % 3, (k + 2) % 3
        t1 = G[:, a] * psi[:, b]
        t2 = G[:, b] * psi[:, a]
        x = t1 - t2
        t = Ar * c[:, k]
        v = t + x
        assert v.dtype == f32
        out[:, k] = np.where(where == NEAR, v, c[:, k])
    out[where == INSIDE] = 0.0
    return out


def compose_f32(obstacles, x, curl, values):
    """The bounded velocity at x from curl(x) -> (N, 3) float32, the unbounded entry point, and values(x) -> (N, 3)
    float32, the three potential values on the rolled tiles."""
    x = np.ascontiguousarray(x, f32)
    where, Ar, G = ramp_f32(obstacles, x)
    c, psi = curl(x), values(x)
    assert c.dtype == f32 and psi.dtype == f32
    return velocity_f32(where, Ar, G, c, psi)


# ---- the host library --------------------------------------------------------------------------------------------------------
def load_host():
    lib = A.load_host()
    lib.wnhost_eval3d.restype = C.c_float
    lib.wnhost_eval3d.argtypes = [FP, C.c_int, FP]
    lib.wnhost_eval3d_curl_bounded.restype = C.c_int   # AttributeError: the library has no boundaries
    lib.wnhost_eval3d_curl_bounded.argtypes = [FP, C.c_int, FP, IP, OP, C.c_int, FP]
    lib.wnhost_eval3d_curl_bounded_advect.restype = C.c_int
    lib.wnhost_eval3d_curl_bounded_advect.argtypes = [FP, C.c_int, FP, IP, OP, C.c_int, C.POINTER(A.wn_advect), FP, FP]
    return lib


def host_values(host, coef, pts, offsets):
    """wnhost_eval3d on the three rolled tiles: (N, 3) float32."""
    import _ref64_curl
    pts = np.ascontiguousarray(pts, f32)
    out = np.empty((len(pts), 3), f32)
    for k, tile in enumerate(_ref64_curl.rolled_tiles(coef, offsets)):
        tile, n, cp = A._tile(tile)
        for i in range(len(pts)):
            out[i, k] = host.wnhost_eval3d(cp, n, pts[i].ctypes.data_as(FP))
    return out


def host_bounded(host, coef, pts, offsets, obstacles):
    coef, n, cp = A._tile(coef)
    off = np.ascontiguousarray(np.asarray(offsets, np.int32).reshape(9))
    pts = np.ascontiguousarray(pts, f32)
    arr = obstacle_array(obstacles)
    out = np.empty((len(pts), 3), f32)
    for i in range(len(pts)):
        rc = host.wnhost_eval3d_curl_bounded(cp, n, pts[i].ctypes.data_as(FP), off.ctypes.data_as(IP), arr, len(obstacles),
                                             out[i].ctypes.data_as(FP))
        assert rc == 0, rc
    return out


def host_bounded_advect(host, coef, pts, offsets, obstacles, adv):
    """wnhost_eval3d_curl_bounded_advect on every point: the final (N, 3) positions and the (S, N, 3) trajectory (None when
    adv.traj_every == 0)."""
    coef, n, cp = A._tile(coef)
    off = np.ascontiguousarray(np.asarray(offsets, np.int32).reshape(9))
    pts = np.ascontiguousarray(pts, f32)
    arr = obstacle_array(obstacles)
    out = np.empty((len(pts), 3), f32)
    snaps = adv.steps // adv.traj_every + 1 if adv.traj_every else 0
    traj = np.empty((len(pts), max(snaps, 1), 3), f32)
    for i in range(len(pts)):
        rc = host.wnhost_eval3d_curl_bounded_advect(cp, n, pts[i].ctypes.data_as(FP), off.ctypes.data_as(IP), arr,
                                                    len(obstacles), C.byref(adv), out[i].ctypes.data_as(FP),
                                                    traj[i].ctypes.data_as(FP) if snaps else None)
        assert rc == 0, rc
    return out, (np.ascontiguousarray(traj.transpose(1, 0, 2)) if snaps else None)
