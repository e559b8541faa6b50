"""CPU checks of the curl of three Perlin potentials (include/wnoise_perlin_curl.h): the host evaluators
wnhost_perlin_curl / wnhost_perlin_turb_curl / wnhost_perlin_fractal_curl (host/scalar_eval.h, in libwnoise_host.so; the
kernels' source compiled for the host) against the long-double reference (tests/_ref64_perlin_curl.py), the composition
with wnhost_perlin_grad bit for bit, the reference field's divergence, and the new header's symbols.  Nothing touches a
device."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, bits

import _ref64_perlin_curl as RC
import _ref64_perlin_grad as R

PKG = os.path.join(ROOT, "wavelet-noise-in-ray-tracing_amd")
FP, DP, IP = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int)
LD = np.longdouble
SEEDS = [12345, 5489]
# the default, and offsets that are negative and >= 256, two of them equal
OFFSET_SETS = {"default": RC.DEFAULT_OFFSETS, "wide": ((-3, 260, 7), (511, -129, 1000), (-3, 260, 7))}


@pytest.fixture(scope="module")
def libs():
    for name in ("libwnoise_host.so", "libwnoise_hip.so"):
        if not os.path.exists(os.path.join(PKG, name)):
            import __graft_entry__
            __graft_entry__.build()
    host = C.CDLL(os.path.join(PKG, "libwnoise_host.so"))
    host.wnhost_perlin_grad.restype = C.c_double
    host.wnhost_perlin_grad.argtypes = [IP, C.c_double, C.c_double, C.c_double, DP]
    for name, args in (("wnhost_perlin_curl", [IP, C.c_double, C.c_double, C.c_double, IP, DP]),
                       ("wnhost_perlin_turb_curl", [IP, FP, C.c_int, IP, DP]),
                       ("wnhost_perlin_fractal_curl", [IP, FP, IP, DP])):
        getattr(host, name).restype = None
        getattr(host, name).argtypes = args
    hip = C.CDLL(os.path.join(PKG, "libwnoise_hip.so"))  # wn_perlin_permutation is a host helper: no device needed
    return host, hip


def perm_table(hip, seed):
    p = np.zeros(512, np.int32)
    assert hip.wn_perlin_permutation(C.c_uint32(seed), p.ctypes.data_as(C.c_void_p)) == 0
    return p


def host_curl(host, perm, kind, pts, offsets, depth=0):
    """The host evaluator at every row of pts (float64 for "noise64", else float32): (N, 3) float64."""
    pp = perm.ctypes.data_as(IP)
    off = np.ascontiguousarray(np.asarray(offsets, np.int32).reshape(9))
    op = off.ctypes.data_as(IP)
    v = np.zeros(3)
    vp = v.ctypes.data_as(DP)
    out = np.empty((len(pts), 3))
    if kind == "noise64":
        for i, (x, y, z) in enumerate(np.ascontiguousarray(pts, np.float64).tolist()):
            host.wnhost_perlin_curl(pp, x, y, z, op, vp)
            out[i] = v
        return out
    pts = np.ascontiguousarray(pts, np.float32)
    for i in range(len(pts)):
        q = pts[i].ctypes.data_as(FP)
        if kind == "noise32":
            host.wnhost_perlin_curl(pp, float(pts[i, 0]), float(pts[i, 1]), float(pts[i, 2]), op, vp)
        elif kind == "turb":
            host.wnhost_perlin_turb_curl(pp, q, depth, op, vp)
        else:
            host.wnhost_perlin_fractal_curl(pp, q, op, vp)
        out[i] = v
    return out


# ---- the host evaluators against the reference ---------------------------------------------------------------------------------
def _point_sets(seed):
    rng = np.random.default_rng(seed)
    return {"random": np.concatenate([rng.uniform(-300.0, 300.0, (6000, 3)), rng.uniform(-4.0, 4.0, (2000, 3))]),
            "faces": R.face_points(rng, 3000)}


@pytest.mark.parametrize("pset", ["random", "faces"])
@pytest.mark.parametrize("oset", list(OFFSET_SETS))
@pytest.mark.parametrize("kind,depth", [("noise64", 0), ("turb", 1), ("turb", 7), ("turb", 8), ("turb", 12), ("fractal", 6)])
@pytest.mark.parametrize("seed", SEEDS)
def test_host_curl_is_within_bound_of_the_reference(libs, seed, kind, depth, oset, pset):
    """Every component within 2 * 1e-12 per octave summed of the long-double reference (a component is the difference of
    two gradient channels)."""
    host, hip = libs
    perm = perm_table(hip, seed)
    pts = _point_sets(seed + depth)[pset]
    if kind != "noise64":
        pts = pts.astype(np.float32)
    off = OFFSET_SETS[oset]
    got = host_curl(host, perm, kind, pts, off, depth)
    rkind = "noise" if kind == "noise64" else kind
    want = RC.velocity(perm, rkind, pts, depth, off).astype(np.float64)
    err = np.abs(got - want).max(0)
    print(kind, depth, seed, oset, pset, "max |host - reference| per component", err)
    assert (err <= RC.bound(rkind, depth)).all(), err


def test_turb_depth_zero_is_zero(libs):
    host, hip = libs
    perm = perm_table(hip, 12345)
    pts = np.random.default_rng(10).uniform(-300.0, 300.0, (50, 3)).astype(np.float32)
    assert (host_curl(host, perm, "turb", pts, OFFSET_SETS["wide"], 0) == 0.0).all()


# ---- composition with the gradient, bit for bit ----------------------------------------------------------------------------------
def exact_shift(p, off):
    """q_k = p + o_k in fp64 for float32-valued p, [3 (potential), N, 3], and the rows where every q_k is exact and lands
    in the shifted cell with the same fractional parts."""
    o = np.asarray(off, np.float64).reshape(3, 1, 3)
    q = p[None] + o
    fp, fq = np.floor(p), np.floor(q)
    ok = ((q - o == p[None]) & (fq == fp[None] + o) & (q - fq == (p - fp)[None])).all(axis=(0, 2))
    return q, ok


@pytest.mark.parametrize("lim", [300.0, 4.0])
@pytest.mark.parametrize("seed", SEEDS)
def test_noise_curl_is_the_subtraction_of_gradient_channels(libs, seed, lim):
    """wnhost_perlin_curl(p, o) has the bits of the fp64 subtraction of wnhost_perlin_grad channels at q_k = p + o_k,
    for float32-valued p and |o| <= 300 (then q - o == p, floor(q) == floor(p) + o and the fractional parts agree: asserted
    per point; at most 0.1 % of the points may fail that and are dropped)."""
    host, hip = libs
    perm = perm_table(hip, seed)
    rng = np.random.default_rng(seed + 1)
    p = rng.uniform(-lim, lim, (6000, 3)).astype(np.float32).astype(np.float64)
    off = rng.integers(-300, 301, (3, 3))
    q, ok = exact_shift(p, off)
    assert (~ok).mean() <= 1e-3, (~ok).sum()
    got = host_curl(host, perm, "noise64", p, off)
    pp = perm.ctypes.data_as(IP)
    g = np.zeros(3)
    J = np.empty((3, len(p), 3))
    for k in range(3):
        for i, (x, y, z) in enumerate(q[k].tolist()):
            host.wnhost_perlin_grad(pp, x, y, z, g.ctypes.data_as(DP))
            J[k, i] = g
    want = np.stack([J[2, :, 1] - J[1, :, 2], J[0, :, 2] - J[2, :, 0], J[1, :, 0] - J[0, :, 1]], axis=-1)
    assert (bits(got[ok]) == bits(want[ok])).all()


# ---- the field is divergence-free ------------------------------------------------------------------------------------------------
def _divergence(field, p, h):
    """Central-difference divergence of field (points -> [N, 3]) in long double."""
    div = np.zeros(len(p), LD)
    for ax in range(3):
        e = np.zeros(3, LD)
        e[ax] = h
        div += (field(p + e)[:, ax] - field(p - e)[:, ax]) / (2 * h)
    return div


def test_reference_field_is_divergence_free(libs):
    """Central differences of the REFERENCE velocity in long double at h = 2^-6 and 2^-8, on 4000 points whose fractional
    parts lie in [2^-5, 1 - 2^-5] (p +- h stays in the cell).  A second-order estimate of a divergence that is 0
    falls 16x per 4x in h; required: at least 8x (a factor 2 of margin for the higher-order terms).  The same estimator
    on the control field grad psi0 (whose divergence, the Laplacian, is not 0) must change by less than 10 %.
    Measured (seed 12345, default offsets): max |div_h v| 1.42e-2 -> 8.86e-4, 16.0x; control 19.35 -> 19.38, 0.13 %."""
    _, hip = libs
    perm = perm_table(hip, 12345)
    rng = np.random.default_rng(77)
    cell = rng.integers(-300, 300, (4000, 3)).astype(LD)
    p = cell + rng.uniform(2.0 ** -5, 1 - 2.0 ** -5, (4000, 3)).astype(LD)
    steps = [LD(2.0) ** -6, LD(2.0) ** -8]
    curl = [float(np.abs(_divergence(lambda q: RC.velocity(perm, "noise", q), p, h)).max()) for h in steps]
    ctrl = [float(np.abs(_divergence(lambda q: RC.jacobian(perm, "noise", q)[:, 0, :], p, h)).max()) for h in steps]
    print("max |div_h v|", curl, "ratio", curl[0] / curl[1], "; control", ctrl, "change", abs(ctrl[0] / ctrl[1] - 1))
    assert curl[0] >= 8 * curl[1], curl
    assert abs(ctrl[0] / ctrl[1] - 1) < 0.10 and ctrl[1] > 1.0, ctrl


# ---- the new header's symbols ----------------------------------------------------------------------------------------------------
NAMES = {"wn_perlin_curl_points", "wn_perlin_curl_points_vec3", "wn_perlin_curl_grid"}


def test_header_symbols_are_exported_and_bound(libs):
    text = open(os.path.join(ROOT, "include", "wnoise_perlin_curl.h")).read()
    assert set(re.findall(r"WN_API\s+[\w\s\*]+?\b(wn_\w+)\s*\(", text)) == NAMES
    capi = importlib.import_module("wavelet-noise-in-ray-tracing_amd._capi")
    lib = capi.load()
    assert set(capi.PERLIN_CURL_SIGNATURES) == NAMES
    assert not NAMES & set(capi.SIGNATURES)
    for n in NAMES:
        fn = getattr(lib, n)  # exported
        assert fn.argtypes == capi.PERLIN_CURL_SIGNATURES[n][1] and fn.restype is capi.PERLIN_CURL_SIGNATURES[n][0]
    assert (capi.WN_PERLIN_CURL_NOISE, capi.WN_PERLIN_CURL_TURB, capi.WN_PERLIN_CURL_FRACTAL) == (0, 1, 2)
    for name, val in re.findall(r"#define (WN_PERLIN_CURL_\w+)\s+(\d+)", text):
        assert getattr(capi, name) == int(val)


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful without a GPU")
def test_no_cpu_fallback(libs):
    capi = importlib.import_module("wavelet-noise-in-ray-tracing_amd._capi")
    lib = capi.load()
    off = (C.c_int32 * 9)(*range(9))
    g = capi.wn_grid(8, 8, 8, 0, 8, 4.0, 16.0, 1.0, 0, 0.0, 1.0, 0)
    assert lib.wn_perlin_curl_points(None, None, 4, off, None, None) == capi.WN_ERR_NO_DEVICE
    assert b"no CPU fallback" in lib.wn_last_error()
    assert lib.wn_perlin_curl_points_vec3(None, None, 4, 1, 7, off, None, None) == capi.WN_ERR_NO_DEVICE
    assert lib.wn_perlin_curl_grid(None, C.byref(g), 2, 0, off, None, None) == capi.WN_ERR_NO_DEVICE
