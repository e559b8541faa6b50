"""CPU checks of particle advection through Perlin curl noise (include/wnoise_perlin_advect.h): the host's scalar tracer
wnhost_perlin_curl_advect (host/scalar_eval.h, in libwnoise_host.so), which runs the time step the device kernel runs
(wn::advect_step<METHOD, double>, csrc/wn_eval.hpp).

 1. composition: the tracer has the bits of numpy float64 stepping, one separately rounded operation per statement
    (tests/_perlin_advect.py), around wnhost_perlin_curl at the float64 stage point (noise) or wnhost_perlin_turb_curl /
    wnhost_perlin_fractal_curl at the stage point rounded to float32; trajectory snapshots (every step, every second one)
    are the intermediate positions; steps == 0 copies the input;
 2. the point set tells the two point types apart: at nextafter(k, -inf) the velocity at q differs from the one at (float)q;
 3. a kind, depth or wn_advect the C ABI refuses is refused, and nothing is written;
 4. the new header's symbols are exported and bound by the package, outside SIGNATURES.
Nothing touches a device."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

from conftest import ROOT, bits

import _perlin_advect as PA

SEED = 12345


@pytest.fixture(scope="module")
def host():
    return PA.load_host()


@pytest.fixture(scope="module")
def perm(host):
    return PA.perm_table(SEED)


@pytest.mark.parametrize("case", PA.CASES, ids=PA.CASE_IDS)
@pytest.mark.parametrize("oset", list(PA.OFFSET_SETS))
@pytest.mark.parametrize("kind,depth", PA.KINDS, ids=PA.KIND_IDS)
def test_composition_bit_for_bit(host, perm, kind, depth, oset, case):
    method, steps, h, gain, drift = case
    off = PA.OFFSET_SETS[oset]
    pts = PA.points()
    path = PA.trace_f64(method, steps, pts, h, gain, drift, PA.host_velocity(host, perm, kind, depth, off))
    got, traj = PA.host_advect(host, perm, kind, depth, pts, off, PA.advect_struct(method, steps, h, gain, drift, 1))
    assert (bits(got) == bits(path[-1])).all()
    assert traj.shape == (steps + 1, len(pts), 3)
    assert (bits(traj) == bits(np.stack(path))).all()
    if steps == 0:
        assert (bits(got) == bits(pts)).all()
    # no trajectory, and every second step: the same final position, snapshots 0, 2, ...
    plain, none = PA.host_advect(host, perm, kind, depth, pts, off, PA.advect_struct(method, steps, h, gain, drift, 0))
    assert none is None and (bits(plain) == bits(got)).all()
    got2, traj2 = PA.host_advect(host, perm, kind, depth, pts, off, PA.advect_struct(method, steps, h, gain, drift, 2))
    assert (bits(got2) == bits(got)).all()
    assert (bits(traj2) == bits(np.stack(path[::2]))).all()


def test_turb_depth_zero_is_pure_drift(host, perm):
    pts = PA.points()
    still = PA.trace_f64(PA.RK4, 3, pts, 0.37, 0.75, PA.DRIFT, lambda q: np.zeros_like(q))
    got, _ = PA.host_advect(host, perm, PA.TURB, 0, pts, PA.DEFAULT_OFFSETS, PA.advect_struct(PA.RK4, 3, 0.37, 0.75, PA.DRIFT))
    assert (bits(got) == bits(still[-1])).all()


def test_the_point_set_pins_where_the_float_rounding_happens(host, perm):
    """At nextafter(k, -inf) the double lies in cell k - 1 and its float rounding in cell k: turb evaluated at the double
    itself (as noise is) would differ from turb at (float)q on those points, so a tracer that rounded in the wrong place
    would fail the composition above."""
    pts = PA.points()[325:]
    off = PA.DEFAULT_OFFSETS
    at_float = PA.host_velocity(host, perm, PA.TURB, 1, off)(pts)
    at_double = PA.host_velocity(host, perm, PA.NOISE, 0, off)(pts)   # one turb octave at the double point is noise there
    differ = (bits(at_float) != bits(at_double)).any(axis=1)
    print("points whose velocity at q and at (float)q differ in bits:", int(differ.sum()), "of", len(pts))
    assert differ.any()
    rounded = pts.astype(np.float32).astype(np.float64)
    assert (bits(at_float) == bits(PA.host_velocity(host, perm, PA.NOISE, 0, off)(rounded))).all()


def test_bad_arguments_are_refused(host, perm):
    p = np.zeros(3)
    out = np.full(3, 7.0)
    off = np.zeros(9, np.int32)
    pp, op = perm.ctypes.data_as(PA.IP), off.ctypes.data_as(PA.IP)

    def call(kind, depth, adv, traj=None):
        return host.wnhost_perlin_curl_advect(pp, kind, depth, p.ctypes.data_as(PA.DP), op, None if adv is None else C.byref(adv),
                                              out.ctypes.data_as(PA.DP), traj)
    good = PA.advect_struct(PA.RK4, 1, 0.1, 1.0, PA.ZERO)
    bad = [PA.advect_struct(3, 1, 0.1, 1.0, PA.ZERO), PA.advect_struct(-1, 1, 0.1, 1.0, PA.ZERO),
           PA.advect_struct(PA.RK4, -1, 0.1, 1.0, PA.ZERO), PA.advect_struct(PA.RK4, 1, 0.1, 1.0, PA.ZERO, -1),
           PA.advect_struct(PA.RK4, 1, np.inf, 1.0, PA.ZERO), PA.advect_struct(PA.RK4, 1, 0.1, np.nan, PA.ZERO),
           PA.advect_struct(PA.RK4, 1, 0.1, 1.0, (0.0, -np.inf, 0.0)), PA.advect_struct(PA.RK4, 1, 0.1, 1.0, PA.ZERO, 1)]
    for adv in bad:   # the last one: a trajectory without a buffer
        assert call(PA.NOISE, 0, adv) == 1
    assert call(PA.NOISE, 0, None) == 1
    assert call(3, 0, good) == 1 and call(-1, 0, good) == 1 and call(PA.TURB, -1, good) == 1
    assert (out == 7.0).all()
    assert call(PA.NOISE, -1, good) == 0 and call(PA.FRACTAL, -1, good) == 0    # depth is read by turb only
    assert (out != 7.0).all()


NAMES = {"wn_perlin_curl_advect_points", "wn_perlin_advect_launch_steps"}


def test_header_symbols_are_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "wnoise_perlin_advect.h")).read()
    assert set(re.findall(r"WN_API\s+[\w\s\*]+?\b(wn_\w+)\s*\(", text)) == NAMES
    assert '#include "wnoise_perlin_curl.h"' in text and '#include "wnoise_advect.h"' in text
    if not os.path.exists(os.path.join(PA.PKG, "libwnoise_hip.so")):
        import __graft_entry__
        __graft_entry__.build()
    capi = importlib.import_module("wavelet-noise-in-ray-tracing_amd._capi")
    lib = capi.load()
    assert set(capi.PERLIN_ADVECT_SIGNATURES) == NAMES
    assert not NAMES & (set(capi.SIGNATURES) | set(capi.ADVECT_SIGNATURES) | set(capi.PERLIN_CURL_SIGNATURES))
    for n in NAMES:
        fn = getattr(lib, n)  # exported
        assert fn.argtypes == capi.PERLIN_ADVECT_SIGNATURES[n][1] and fn.restype is capi.PERLIN_ADVECT_SIGNATURES[n][0]


def test_launch_steps_follow_the_octave_budget():
    """wn_perlin_advect_launch_steps is max(1, budget / (stages * octaves)) with one budget: stages 1, 2, 4 by method,
    octaves 1 (noise), max(depth, 1) (turb), 6 (fractal_noise).  No device is needed."""
    capi = importlib.import_module("wavelet-noise-in-ray-tracing_amd._capi")
    L = capi.load().wn_perlin_advect_launch_steps
    budget = L(PA.NOISE, 0, PA.EULER)
    text = open(os.path.join(PA.PKG, "csrc", "wn_perlin_advect.hip")).read()
    assert budget == int(re.search(r"constexpr int kPerlinAdvectOctaveBudget = (\d+);", text).group(1)) >= 1
    for method, stages in ((PA.EULER, 1), (PA.MIDPOINT, 2), (PA.RK4, 4)):
        assert L(PA.NOISE, 99, method) == max(1, budget // stages)
        assert L(PA.FRACTAL, 99, method) == max(1, budget // (stages * 6))
        for depth in (0, 1, 7, 8, 1000, 2 ** 31 - 1):
            assert L(PA.TURB, depth, method) == max(1, budget // (stages * max(depth, 1))), (depth, method)
