"""CPU checks of the analytic gradients of perlin::noise, turb and fractal_noise: the long-double reference
(tests/_ref64_perlin_grad.py) against central differences of its own value, and the host evaluators wnhost_perlin_grad /
wnhost_perlin_turb_grad / wnhost_perlin_fractal_grad (host/scalar_eval.h, in libwnoise_host.so) against that reference
and against wnhost_perlin / wnhost_perlin_turb / wnhost_perlin_fractal.  Nothing touches a device."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT, bits

import _ref64_perlin_grad as R

PKG = os.path.join(ROOT, "wavelet-noise-in-ray-tracing_amd")
FP, DP, IP = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int)
LD = np.longdouble
SEEDS = [12345, 5489]


@pytest.fixture(scope="module")
def libs():
    for name in ("libwnoise_host.so", "libwnoise_hip.so"):
        if not os.path.exists(os.path.join(PKG, name)):
            import __graft_entry__
            __graft_entry__.build()
    host = C.CDLL(os.path.join(PKG, "libwnoise_host.so"))
    for name, args in (("wnhost_perlin", [IP, C.c_double, C.c_double, C.c_double]),
                       ("wnhost_perlin_grad", [IP, C.c_double, C.c_double, C.c_double, DP]),
                       ("wnhost_perlin_turb", [IP, FP, C.c_int]), ("wnhost_perlin_turb_grad", [IP, FP, C.c_int, DP]),
                       ("wnhost_perlin_fractal", [IP, FP]), ("wnhost_perlin_fractal_grad", [IP, FP, DP])):
        getattr(host, name).restype = C.c_double
        getattr(host, name).argtypes = args
    hip = C.CDLL(os.path.join(PKG, "libwnoise_hip.so"))  # wn_perlin_permutation is a host helper: no device needed
    return host, hip


def perm_table(hip, seed):
    p = np.zeros(512, np.int32)
    assert hip.wn_perlin_permutation(C.c_uint32(seed), p.ctypes.data_as(C.c_void_p)) == 0
    return p


def host_records(host, perm, kind, pts, depth=0):
    """The host evaluator at every row of pts (float64 for "noise64", else float32): (N, 4) float64 records and the
    matching value function's results."""
    pp = perm.ctypes.data_as(IP)
    g = np.zeros(3)
    gp = g.ctypes.data_as(DP)
    out = np.empty((len(pts), 4))
    val = np.empty(len(pts))
    if kind == "noise64":
        pts = np.ascontiguousarray(pts, np.float64)
        for i, (x, y, z) in enumerate(pts.tolist()):
            out[i, 0] = host.wnhost_perlin_grad(pp, x, y, z, gp)
            out[i, 1:] = g
            val[i] = host.wnhost_perlin(pp, x, y, z)
        return out, val
    pts = np.ascontiguousarray(pts, np.float32)
    for i in range(len(pts)):
        q = pts[i].ctypes.data_as(FP)
        if kind == "turb":
            out[i, 0] = host.wnhost_perlin_turb_grad(pp, q, depth, gp)
            val[i] = host.wnhost_perlin_turb(pp, q, depth)
        else:
            out[i, 0] = host.wnhost_perlin_fractal_grad(pp, q, gp)
            val[i] = host.wnhost_perlin_fractal(pp, q)
        out[i, 1:] = g
    return out, val


# ---- the reference gradient is the derivative of the reference value -------------------------------------------------------
def _interior(p, finest, h):
    """Rows of p whose coordinates, at the finest octave's scale, stay at least 2h from a cell face: the +-h neighbours
    are then in the same cell in every octave (the coarser octaves' faces are a subset of the finest's)."""
    q = np.asarray(p, LD) * LD(finest)
    f = q - np.floor(q)
    return ((f > 2 * h * finest) & (f < 1 - 2 * h * finest)).all(axis=1)


def _central(fn, p, h):
    """Central differences of fn (points -> values) in long double: [N, 3]."""
    cols = []
    for ax in range(3):
        e = np.zeros(3, LD)
        e[ax] = h
        cols.append((fn(p + e) - fn(p - e)) / (2 * h))
    return np.stack(cols, axis=-1)


@pytest.mark.parametrize("seed", SEEDS)
def test_ref_noise_gradient_is_the_derivative_of_the_ref_value(libs, seed):
    """Central differences in long double at h = 2^-20 inside a cell: the quotient is off by h^2/6 times the third
    derivative (about 2e-11) plus round-off 1e-19 / h.  Bound: 1e-9 per noise evaluation."""
    perm = perm_table(libs[1], seed)
    h = LD(2.0) ** -20
    p = np.random.default_rng(seed).uniform(-300.0, 300.0, (60000, 3)).astype(LD)
    p = p[_interior(p, 1, h)]
    assert len(p) > 59000
    _, g = R.noise_grad(perm, p)
    err = np.abs(_central(lambda q: R.noise_grad(perm, q)[0], p, h) - g).max()
    print("noise: central differences vs analytic, max", float(err))
    assert err <= 1e-9


@pytest.mark.parametrize("kind,depth", [("turb", 1), ("turb", 7), ("turb", 12), ("fractal", 6)])
def test_ref_octave_sum_gradient_is_the_derivative_of_the_ref_value(libs, kind, depth):
    """turb and fractal_noise.  The step is 2^-20 at the FINEST octave's scale (h = 2^-20 / 2^(depth-1) in p): octave i
    sees the step 2^i h and contributes a truncation error of 4^i h^2/6 times noise's third derivative, so a step of
    2^-20 in p itself would leave 4^(depth-1) times noise's own error in the last octave (8e-8 at depth 7); scaled, the
    octaves' errors sum to 4/3 of noise's.  Round-off 1e-19 / h stays below 1e-9 up to depth 12.  Bound: 1e-9 per noise
    evaluation, depth of them.  turb: points within 1e-6 of the kink (|sum| < 1e-6) are left out, at most 1 %."""
    perm = perm_table(libs[1], 12345)
    finest = 2.0 ** (depth - 1)
    h = LD(2.0) ** -20 / LD(finest)
    p = np.random.default_rng(depth).uniform(-8.0, 8.0, (40000, 3)).astype(LD)
    p = p[_interior(p, finest, h)]
    assert len(p) > 39000
    if kind == "turb":
        _, g, s = R.turb_grad(perm, p, depth)
        keep = np.abs(s) >= 1e-6
        assert (~keep).mean() <= 0.01
        p, g = p[keep], g[keep]
        fd = _central(lambda q: R.turb_grad(perm, q, depth)[0], p, h)
    else:
        _, g = R.fractal_grad(perm, p)
        fd = _central(lambda q: R.fractal_grad(perm, q)[0], p, h)
    err = np.abs(fd - g).max()
    print(kind, depth, "central differences vs analytic, max", float(err))
    assert err <= 1e-9 * depth


# ---- the host evaluators against the reference ---------------------------------------------------------------------------------
def _point_sets(seed):
    rng = np.random.default_rng(seed)
    return {"random": np.concatenate([rng.uniform(-300.0, 300.0, (12000, 3)), rng.uniform(-4.0, 4.0, (3000, 3))]),
            "faces": R.face_points(rng, 6000)}


@pytest.mark.parametrize("pset", ["random", "faces"])
@pytest.mark.parametrize("seed", SEEDS)
def test_host_noise_gradient(libs, seed, pset):
    """noise(double, double, double): every channel within 1e-12 of the reference, the value channel with the bits of
    wnhost_perlin."""
    host, hip = libs
    perm = perm_table(hip, seed)
    pts = _point_sets(seed)[pset]
    got, val = host_records(host, perm, "noise64", pts)
    assert (bits(got[:, 0]) == bits(val)).all()
    want, _ = R.eval_records(perm, "noise", pts.astype(LD))
    err = np.abs(got - want).max(0)
    print("noise", seed, pset, "max |host - reference| per channel", err)
    assert (err <= R.bound("noise")).all(), err


@pytest.mark.parametrize("pset", ["random", "faces"])
@pytest.mark.parametrize("kind,depth", [("turb", 1), ("turb", 7), ("turb", 8), ("turb", 12), ("fractal", 6)])
@pytest.mark.parametrize("seed", SEEDS)
def test_host_octave_sum_gradients(libs, seed, kind, depth, pset):
    """turb / fractal_noise on float points: every channel within 1e-12 per octave summed, the value channel with the
    bits of wnhost_perlin_turb / wnhost_perlin_fractal.  turb: points where a differently ordered sum may take the other
    sign (|sum| < 1e-10) are left out, at most 1e-4 of them."""
    host, hip = libs
    perm = perm_table(hip, seed)
    pts = _point_sets(seed + depth)[pset].astype(np.float32)
    got, val = host_records(host, perm, kind, pts, depth)
    assert (bits(got[:, 0]) == bits(val)).all()
    want, s = R.eval_records(perm, kind, pts, depth)
    keep = np.ones(len(pts), bool)
    if kind == "turb":
        keep = np.abs(s) >= 1e-10
        if pset == "random":
            assert (~keep).mean() <= 1e-4
        # on faces the sum is exactly 0 where all three coordinates are lattice points of every octave: gradient sign +1
        # in both, by definition; anything else this close to the kink is left out
        exact_zero = s == 0.0
        keep |= exact_zero
    err = np.abs(got - want)[keep].max(0)
    print(kind, depth, seed, pset, "max |host - reference| per channel", err, "left out", int((~keep).sum()))
    assert (err <= R.bound(kind, depth)).all(), err


def test_gradient_at_lattice_points_is_the_corner_vector(libs):
    """At an integer lattice point the value is 0 and the gradient is that corner's G (exactly: every fade and fade' is
    0 there)."""
    host, hip = libs
    perm = perm_table(hip, 12345)
    rng = np.random.default_rng(8)
    pts = rng.integers(-300, 300, (4000, 3)).astype(np.float64)
    got, _ = host_records(host, perm, "noise64", pts)
    h = R.corner_hashes(perm, pts.astype(np.int64))[:, 0, 0, 0] & 15
    assert (got[:, 0] == 0.0).all()
    assert (got[:, 1:] == R.GVEC[h]).all()


def test_gradient_is_continuous_across_cell_faces(libs):
    """Either side of a face, 2^-30 away: the gradient jumps by the second derivative times the distance.  |second
    derivative| <= 64 (fade'' <= 5.8 times corner differences <= 4, plus 2 fade' <= 3.75 times unit vectors, with
    margin), so the jump stays below 64 * 2^-29."""
    host, hip = libs
    perm = perm_table(hip, 5489)
    rng = np.random.default_rng(9)
    base = rng.uniform(-50.0, 50.0, (3000, 3))
    ax = rng.integers(0, 3, len(base))
    rows = np.arange(len(base))
    face = np.rint(base[rows, ax])
    lo, hi = base.copy(), base.copy()
    lo[rows, ax] = face - 2.0 ** -30
    hi[rows, ax] = face + 2.0 ** -30
    a, _ = host_records(host, perm, "noise64", lo)
    b, _ = host_records(host, perm, "noise64", hi)
    jump = np.abs(a - b).max()
    print("largest jump across a face at +-2^-30:", jump)
    assert jump <= 64 * 2.0 ** -29


def test_turb_depth_zero_is_zero_in_all_channels(libs):
    host, hip = libs
    perm = perm_table(hip, 12345)
    pts = np.random.default_rng(10).uniform(-300.0, 300.0, (50, 3)).astype(np.float32)
    got, val = host_records(host, perm, "turb", pts, 0)
    assert (got == 0.0).all() and (val == 0.0).all()
