"""What the 2-D boundary tests share (tests/test_bounded2d_host.py, tests/test_gpu_bounded2d.py): the obstacle ramp, the
background stream and the bounded velocity of include/wnoise_bounded2d.h written out in numpy float32, one separately rounded
operation per statement, around any function that yields {psi, d/dx, d/dy}; the obstacle sets; and the host's
wnhost_multiband2d_curl_bounded / wnhost_multiband2d_curl_bounded_advect through ctypes.

An obstacle is the tuple the Python members take: ("disc", c, r, d0), ("container", c, r, d0) or ("halfplane", n, o, d0);
a stream is None or (ux, uy); bands = (s, first_band, nbands, w, var_per_band) as in tests/_advect2d.py."""
import ctypes as C

import numpy as np

import _advect2d as A
import _ref64_curl2d as R2
import _ref64_multiband2d as M

f32 = np.float32
FP = A.FP
KINDS = {"disc": 0, "container": 1, "halfplane": 2}
FAR, NEAR, INSIDE = 0, 1, 2


class wn_obstacle2d(C.Structure):
    """include/wnoise_bounded2d.h"""
    _fields_ = [("kind", C.c_int32), ("c", C.c_float * 2), ("r", C.c_float), ("d0", C.c_float), ("reserved", C.c_int32 * 3)]


OP = C.POINTER(wn_obstacle2d)


def obstacle_array(obstacles):
    arr = (wn_obstacle2d * max(1, len(obstacles)))()
    for dst, (kind, c, r, d0) in zip(arr, obstacles):
        dst.kind, dst.c, dst.r, dst.d0 = KINDS[kind], (C.c_float * 2)(*c), r, d0
    return arr


def flow_array(flow):
    return None if flow is None else (C.c_float * 2)(*flow)


# ---- the obstacle sets of the tests, at the scale of A.points(): coordinates in (-300, 300) -------------------------------
DISC = ("disc", (0.0, 0.0), 120.0, 80.0)
GROUND = ("halfplane", (0.0, 2.0), -500.0, 200.0)           # not a unit normal: fluid where y > -250, the ramp ends at y = -150
CONTAINER = ("container", (0.0, 0.0), 500.0, 150.0)
THREE = [DISC, GROUND, CONTAINER]                             # the ramps of the ground and the container overlap
FLOW = (0.3, -0.2)
FLOWS = {"noflow": None, "zeroflow": (0.0, 0.0), "flow": FLOW}


def sixteen(seed=5):
    """16 obstacles: THREE, a second half-plane with a normal that is not a unit vector, and 12 small discs."""
    rng = np.random.default_rng(seed)
    out = THREE + [("halfplane", (0.5, 2.0), -700.0, 90.0)]
    for _ in range(12):
        c = rng.uniform(-250.0, 250.0, 2)
        out.append(("disc", tuple(float(f32(v)) for v in c), float(f32(rng.uniform(20.0, 50.0))),
                    float(f32(rng.uniform(30.0, 70.0)))))
    return out


SETS = {"none": [], "disc": [DISC], "three": THREE, "sixteen": sixteen()}


def points(oset, count=350, seed=41):
    """`count` points uniform in (-300, 300)^2, the last seventh on half-integer knots; for the lone disc drawn into
    (-210, 210)^2, where its ramp fills near half of the box.  Every obstacle set then has far, near and inside points."""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-300.0, 300.0, (count, 2)).astype(f32)
    if oset == "disc":
        pts = pts * f32(0.7)
    k = count - count // 7
    pts[k:] = np.floor(pts[k:]) + f32(0.5)
    return pts


# ---- the arithmetic, one float32 operation per statement -------------------------------------------------------------------
def distance_f32(obstacle, x):
    """d (N,) and nrm (N, 2) of one obstacle at the (N, 2) float32 points x."""
    kind, c, r, _ = obstacle
    c, r = np.asarray(c, f32), f32(r)
    if kind == "halfplane":
        t0 = c[0] * x[:, 0]
        t1 = c[1] * x[:, 1]
        s = t0 + t1
        d = s - r
        return d, np.broadcast_to(c, x.shape)
    dx = x - c
    q0 = dx[:, 0] * dx[:, 0]
    q1 = dx[:, 1] * dx[:, 1]
    l2 = q0 + q1
    ln = np.sqrt(l2)
    assert ln.dtype == f32
    with np.errstate(divide="ignore", invalid="ignore"):
        m = dx / ln[:, None]
    m = np.where(ln[:, None] == 0, f32(0.0), m)
    if kind == "disc":
        return ln - r, m
    return r - ln, -m


def ramp_f32(obstacles, x):
    """where (N,) in {FAR, NEAR, INSIDE}, A (N,) and G (N, 2): the running product over the near obstacles in list order."""
    x = np.ascontiguousarray(x, f32)
    n = len(x)
    Ar, G = np.ones(n, f32), np.zeros((n, 2), f32)
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


def velocity_f32(where, Ar, G, grad, flow, x):
    """The contract's velocity from grad = (N, 3) float32 {psi, gx, gy} at the (N, 2) float32 points x."""
    psi, gx, gy = grad[:, 0], grad[:, 1], grad[:, 2]
    if flow is not None:
        ux, uy = f32(flow[0]), f32(flow[1])
        a0 = ux * x[:, 1]
        a1 = uy * x[:, 0]
        bg = a0 - a1
        psi = psi + bg
        gx = gx - uy
        gy = gy + ux
    t0 = Ar * gy
    u0 = G[:, 1] * psi
    v0 = t0 + u0
    t1 = Ar * gx
    u1 = G[:, 0] * psi
    v1 = t1 + u1
    v1 = -v1
    near = np.stack([v0, v1], axis=1)
    far = np.stack([gy, -gx], axis=1)
    assert near.dtype == f32 and far.dtype == f32
    out = np.where((where == NEAR)[:, None], near, far)
    out[where == INSIDE] = 0.0
    return out


def compose_f32(obstacles, flow, x, grad):
    """The bounded velocity at x from grad(x) -> (N, 3) float32: the channels of wn_multiband2d_grad_points."""
    x = np.ascontiguousarray(x, f32)
    where, Ar, G = ramp_f32(obstacles, x)
    g = grad(x)
    assert g.dtype == f32
    return velocity_f32(where, Ar, G, g, flow, x)


# ---- the host library --------------------------------------------------------------------------------------------------------
def load_host():
    lib = A.load_host()
    lib.wnhost_multiband2d_curl_bounded.restype = C.c_int   # AttributeError: the library has no 2-D boundaries
    lib.wnhost_multiband2d_curl_bounded.argtypes = [FP, C.c_int, FP, C.c_float, C.c_int, C.c_int, FP, C.c_float, OP, C.c_int,
                                                    FP, FP]
    lib.wnhost_multiband2d_curl_bounded_advect.restype = C.c_int
    lib.wnhost_multiband2d_curl_bounded_advect.argtypes = [FP, C.c_int, FP, C.c_float, C.c_int, C.c_int, FP, C.c_float, OP,
                                                           C.c_int, FP, C.POINTER(A.wn_advect2d), FP, FP]
    return lib


def host_grad(host, coef, pts, bands):
    """wnhost_multiband2d_footprint's gradient form with the hard cut: (N, 3) float32 {psi, gx, gy}."""
    s, first, nb, w, var = bands
    return M.host_multiband2d(host, coef, pts, s, first, nb, w, var, 0, value_form=False)[0]


def host_bounded(host, coef, pts, bands, obstacles, flow):
    s, first, nb, w, var = bands
    cp, n, _keep = R2.tile_args(coef)
    wa = (C.c_float * max(1, nb))(*[float(x) for x in w[:nb]])
    pts = np.ascontiguousarray(pts, f32)
    arr, fl = obstacle_array(obstacles), flow_array(flow)
    out = np.empty((len(pts), 2), f32)
    for i in range(len(pts)):
        rc = host.wnhost_multiband2d_curl_bounded(cp, n, pts[i].ctypes.data_as(FP), float(s), first, nb, wa, var, arr,
                                                  len(obstacles), fl, out[i].ctypes.data_as(FP))
        assert rc == 0, rc
    return out


def host_bounded_advect(host, coef, pts, bands, obstacles, flow, adv):
    """wnhost_multiband2d_curl_bounded_advect on every point: the final (N, 2) positions and the (S, N, 2) trajectory (None
    when adv.traj_every == 0)."""
    s, first, nb, w, var = bands
    cp, n, _keep = R2.tile_args(coef)
    wa = (C.c_float * max(1, nb))(*[float(x) for x in w[:nb]])
    pts = np.ascontiguousarray(pts, f32)
    arr, fl = obstacle_array(obstacles), flow_array(flow)
    out = np.empty((len(pts), 2), f32)
    snaps = adv.steps // adv.traj_every + 1 if adv.traj_every else 0
    traj = np.empty((len(pts), max(snaps, 1), 2), f32)
    for i in range(len(pts)):
        rc = host.wnhost_multiband2d_curl_bounded_advect(cp, n, pts[i].ctypes.data_as(FP), float(s), first, nb, wa, var, arr,
                                                         len(obstacles), fl, C.byref(adv), out[i].ctypes.data_as(FP),
                                                         traj[i].ctypes.data_as(FP) if snaps else None)
        assert rc == 0, rc
    return out, (np.ascontiguousarray(traj.transpose(1, 0, 2)) if snaps else None)
