"""CPU checks of particle advection through wavelet curl noise (include/wnoise_advect.h): the host's scalar tracer
wnhost_eval3d_curl_advect (host/scalar_eval.h, in libwnoise_host.so), which runs the time step the device kernel runs
(wn::advect_step, csrc/wn_eval.hpp).

 1. composition: the tracer has the bits of numpy float32 stepping, one separately rounded operation per statement
    (tests/_advect.py), around wnhost_eval3d_curl; trajectory snapshots are the intermediate positions;
 2. the methods are the named methods: on a tile whose curl is the linear field v = A (p - 8) one step satisfies
    p' = p + h Phi(hA) v(p) with Phi = I (Euler), I + hA/2 (midpoint), I + hA/2 + (hA)^2/6 + (hA)^3/24 (RK4), to 1e-4:
    in float64 each method meets its own Phi to 6e-7 and misses every other method's by at least 0.06; float32 stepping at
    |p| <= 11 with coefficients <= 25 in magnitude adds a few 1e-5 at most;
 3. sizeof(wn_advect) == 32, in the C header's layout and in the package's ctypes mirror.
Nothing touches a device."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

from conftest import ROOT, bits

import _advect as A
import _ref64_curl

MIXED = ((0, 0, 0), (1, 2, 3), (-5, 7, 130))


@pytest.fixture(scope="module")
def host():
    return A.load_host()


def offsets_of(name, coef):
    return _ref64_curl.default_offsets(_ref64_curl.tile_size(coef)) if name == "default" else MIXED


@pytest.mark.parametrize("case", A.CASES, ids=A.CASE_IDS)
@pytest.mark.parametrize("oset", ["default", "mixed"])
@pytest.mark.parametrize("key", ["tile3d_8_7", "tile3d_5odd_11"])
def test_composition_bit_for_bit(host, gold, key, oset, case):
    method, steps, h, gain, drift = case
    coef = np.ascontiguousarray(gold[key], np.float32)
    off = offsets_of(oset, coef)
    pts = A.points()
    path = A.trace_f32(method, steps, pts, h, gain, drift, lambda q: A.host_curl(host, coef, q, off))
    got, traj = A.host_advect(host, coef, pts, off, A.advect_struct(method, steps, h, gain, drift, 1))
    assert (bits(got) == bits(path[-1])).all()
    assert traj.shape == (steps + 1, len(pts), 3)
    assert (bits(traj) == bits(np.stack(path))).all()
    if steps == 0:
        assert (bits(got) == bits(pts)).all()
    # no trajectory, and every second step: the same final position, snapshots 0, 2, ...
    plain, none = A.host_advect(host, coef, pts, off, A.advect_struct(method, steps, h, gain, drift, 0))
    assert none is None and (bits(plain) == bits(got)).all()
    got2, traj2 = A.host_advect(host, coef, pts, off, A.advect_struct(method, steps, h, gain, drift, 2))
    assert (bits(got2) == bits(got)).all()
    assert (bits(traj2) == bits(np.stack(path[::2]))).all()


def test_empty_tile_is_pure_drift_and_bad_arguments_are_refused(host):
    pts = A.points()
    empty = np.empty(0, np.float32)
    path = A.trace_f32(A.RK4, 3, pts, 0.37, 0.75, A.DRIFT, lambda q: np.zeros_like(q))
    got, _ = A.host_advect(host, empty, pts, MIXED, A.advect_struct(A.RK4, 3, 0.37, 0.75, A.DRIFT))
    assert (bits(got) == bits(path[-1])).all()
    p = np.zeros(3, np.float32)
    out = np.full(3, 7.0, np.float32)
    off = np.zeros(9, np.int32)
    bad = [A.advect_struct(3, 1, 0.1, 1.0, A.ZERO), A.advect_struct(-1, 1, 0.1, 1.0, A.ZERO),
           A.advect_struct(A.RK4, -1, 0.1, 1.0, A.ZERO), A.advect_struct(A.RK4, 1, 0.1, 1.0, A.ZERO, -1),
           A.advect_struct(A.RK4, 1, np.inf, 1.0, A.ZERO), A.advect_struct(A.RK4, 1, 0.1, np.nan, A.ZERO),
           A.advect_struct(A.RK4, 1, 0.1, 1.0, (0.0, -np.inf, 0.0)), A.advect_struct(A.RK4, 1, 0.1, 1.0, A.ZERO, 1)]
    for adv in bad:   # the last one: a trajectory without a buffer
        assert host.wnhost_eval3d_curl_advect(None, 0, p.ctypes.data_as(A.FP), off.ctypes.data_as(A.IP), C.byref(adv),
                                              out.ctypes.data_as(A.FP), None) == 1
    assert host.wnhost_eval3d_curl_advect(None, 0, p.ctypes.data_as(A.FP), off.ctypes.data_as(A.IP), None,
                                          out.ctypes.data_as(A.FP), None) == 1
    assert (out == 7.0).all()


def phi(method, hA):
    eye = np.eye(3)
    if method == A.EULER:
        return eye
    if method == A.MIDPOINT:
        return eye + hA / 2.0
    return eye + hA / 2.0 + hA @ hA / 6.0 + hA @ hA @ hA / 24.0


@pytest.mark.parametrize("method", [A.EULER, A.MIDPOINT, A.RK4], ids=["euler", "midpoint", "rk4"])
def test_the_methods_are_the_named_methods(host, method):
    g = np.arange(16, dtype=np.float64) - 8.0
    coef = np.broadcast_to(-0.5 * (g[None, None, :] ** 2 + g[None, :, None] ** 2), (16, 16, 16)).astype(np.float32)
    off = ((0, 0, 0),) * 3
    Amat = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [-1.0, 1.0, 0.0]])
    pts = np.random.default_rng(12).uniform(6.5, 9.5, (500, 3)).astype(np.float32)
    v = A.host_curl(host, coef, pts, off).astype(np.float64)
    assert np.abs(v - (pts.astype(np.float64) - 8.0) @ Amat.T).max() <= 1e-4    # the field is the linear one
    h = 0.5
    got, _ = A.host_advect(host, coef, pts, off, A.advect_struct(method, 1, h, 1.0, A.ZERO))
    errs = {}
    for m in (A.EULER, A.MIDPOINT, A.RK4):
        want = pts.astype(np.float64) + h * v @ phi(m, h * Amat).T
        errs[m] = float(np.abs(got.astype(np.float64) - want).max())
    print("one step against Phi of euler / midpoint / rk4:", errs)
    assert errs[method] <= 1e-4, errs
    assert all(e > 1e-4 for m, e in errs.items() if m != method), errs


def test_struct_size_and_symbols():
    header = open(os.path.join(ROOT, "include", "wnoise_advect.h")).read()
    body = re.search(r"typedef struct wn_advect \{(.*?)\} wn_advect;", header, re.S).group(1)
    fields = re.findall(r"^\s*(int32_t|float)\s+(\w+)(?:\[(\d+)\])?;", body, re.M)
    assert [(t, n, int(k or 1)) for t, n, k in fields] == [("int32_t", "method", 1), ("int32_t", "steps", 1), ("float", "h", 1),
                                                         ("float", "gain", 1), ("float", "drift", 3), ("int32_t", "traj_every", 1)]
    assert C.sizeof(A.wn_advect) == 32
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(A.PKG, "libwnoise_hip.so")):
        ge.build()
    capi = importlib.import_module("wavelet-noise-in-ray-tracing_amd._capi")
    assert C.sizeof(capi.wn_advect) == 32
    assert [(n, C.sizeof(t)) for n, t in capi.wn_advect._fields_] == [(n, C.sizeof(t)) for n, t in A.wn_advect._fields_]
    lib = capi.load()
    names = sorted(set(re.findall(r"WN_API\s+[\w\s\*]+?\b(wn_\w+)\s*\(", header)))
    assert len(names) == 3, names
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/wnoise_advect.h but not exported"
    assert set(capi.ADVECT_SIGNATURES) == set(names)
    assert not set(names) & set(capi.SIGNATURES)
    assert 1 <= lib.wn_advect_launch_steps() <= 64   # tests/test_gpu_advect.py chains launches of that many RK4 steps
