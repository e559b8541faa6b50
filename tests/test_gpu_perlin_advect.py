"""GPU: particles moved through Perlin curl noise inside one kernel (csrc/wn_perlin_advect.hip,
include/wnoise_perlin_advect.h).  Every comparison is bit for bit.  The point set is tests/_perlin_advect.py's 350 float64
points (two workgroups, the second ragged) unless a test names another size.

 * composition: wn_perlin_curl_advect_points has the bits of wn_perlin_curl_points (noise) / wn_perlin_curl_points_vec3 at
   q.astype(float32) (turb, fractal_noise) on the device plus the time step written out in numpy float64, one separately
   rounded operation per statement (tests/_perlin_advect.py);
 * host twin: the bits of wnhost_perlin_curl_advect;
 * trajectory: snapshot t has the bits of a separate call of t * e steps, the final position those of a call without one;
 * launch chaining: L + 1 steps have the bits of L steps followed by one more, L = wn_perlin_advect_launch_steps(..), and a
   trajectory over 2 L + 1 steps those of the chained calls;
 * sizes: n = 1, n = 257, and a list that takes the grid-stride loop through a second trip;
 * in place: xyz_out == xyz_in has the out-of-place bits; a partial overlap is refused;
 * exact output: guard doubles around xyz_out and traj stay untouched from pointers that are not 16-byte aligned;
 * argument checks, the C++ members (tests/host_src/perlin_advect_api_check.cpp) and perlin.advect_curl.
"""
import ctypes as C
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _perlin_advect as PA  # noqa: E402
from _frame import Frame  # noqa: E402
from conftest import bits  # noqa: E402

PKG = PA.PKG
SEED = 12345
WIDE = PA.OFFSET_SETS["wide"]
f64 = np.float64


@pytest.fixture(scope="module")
def wn():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU (the product has no CPU path)"
    return importlib.import_module("wavelet-noise-in-ray-tracing_amd")


@pytest.fixture(scope="module")
def nm(wn):
    return importlib.import_module("wavelet-noise-in-ray-tracing_amd.noise")


@pytest.fixture(scope="module")
def per(wn):
    return wn.perlin(SEED)


@pytest.fixture(scope="module")
def pts():
    return PA.points()


def cuda(a, dtype=f64):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _np(t):
    return t.cpu().numpy()


def adv_ptr(nm, adv):
    """tests/_advect.py's mirror of wn_advect as the package's own pointer type (the layouts are compared on the CPU)."""
    return None if adv is None else C.cast(C.pointer(adv), C.POINTER(nm._capi.wn_advect))


def offsets9(per, offsets):
    return per._curl_offsets(offsets)


def abi(nm, per, kind, depth, off, xin, n, adv, xout, traj=None):
    """wn_perlin_curl_advect_points on raw pointers; per: the perlin object, or None for a NULL perm."""
    return nm._lib.wn_perlin_curl_advect_points(per._h if per is not None else None, xin, n, kind, depth, off, adv_ptr(nm, adv),
                                                xout, traj, nm._stream())


def advect(nm, per, kind, depth, offsets, p, adv):
    """The C ABI on a host array: the final (N, 3) positions and the (S, N, 3) trajectory (None without one)."""
    import torch
    x = cuda(p)
    n = x.shape[0]
    out = torch.empty((n, 3), dtype=torch.float64, device="cuda")
    snaps = adv.steps // adv.traj_every + 1 if adv.traj_every else 0
    traj = torch.empty((snaps, n, 3), dtype=torch.float64, device="cuda") if snaps else None
    rc = abi(nm, per, kind, depth, offsets9(per, offsets), nm._ptr(x), n, adv, nm._ptr(out), nm._ptr(traj))
    assert rc == 0, nm._lib.wn_last_error()
    return _np(out), (_np(traj) if snaps else None)


def gpu_velocity(per, kind, depth, offsets):
    """velocity(q) for trace_f64 from the device's own point entry points: wn_perlin_curl_points at the float64 points
    (noise), wn_perlin_curl_points_vec3 at q.astype(float32) (turb, fractal_noise)."""
    def velocity(q):
        assert q.dtype == f64
        if kind == PA.NOISE:
            return _np(per.noise_curl(cuda(q), offsets))
        q32 = cuda(q.astype(np.float32), np.float32)
        return _np(per.turb_curl(q32, depth, offsets) if kind == PA.TURB else per.fractal_noise_curl(q32, offsets))
    return velocity


# ---- composition -----------------------------------------------------------------------------------------------------------
MAIN_KINDS = [(PA.NOISE, 0), (PA.TURB, 7), (PA.FRACTAL, 0)]
COMPOSITION = [(k, d, c) for k, d in MAIN_KINDS for c in range(len(PA.CASES))] + \
              [(PA.TURB, d, c) for d in (0, 1) for c in (2, 6, 11)]


def kind_id(kind, depth):
    return PA.KIND_NAMES[kind] + (str(depth) if kind == PA.TURB else "")


@pytest.mark.gpu
@pytest.mark.parametrize("kind,depth,case", COMPOSITION, ids=[f"{kind_id(k, d)}_{PA.CASE_IDS[c]}" for k, d, c in COMPOSITION])
def test_composition_bit_for_bit(nm, per, pts, kind, depth, case):
    method, steps, h, gain, drift = PA.CASES[case]
    off = WIDE if case % 2 else None       # None: the library's own default
    want = PA.trace_f64(method, steps, pts, h, gain, drift, gpu_velocity(per, kind, depth, off))
    got, traj = advect(nm, per, kind, depth, off, pts, PA.advect_struct(method, steps, h, gain, drift, 1))
    assert got.shape == (len(pts), 3) and traj.shape == (steps + 1, len(pts), 3)
    assert (bits(got) == bits(want[-1])).all()
    assert (bits(traj) == bits(np.stack(want))).all()
    if steps == 0:
        assert (bits(got) == bits(pts)).all()
    if kind == PA.TURB and depth == 0:     # v = 0: pure drift
        still = PA.trace_f64(method, steps, pts, h, gain, drift, lambda q: np.zeros_like(q))
        assert (bits(got) == bits(still[-1])).all()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,depth", MAIN_KINDS, ids=[kind_id(k, d) for k, d in MAIN_KINDS])
@pytest.mark.parametrize("case", [3, 7, 13], ids=[PA.CASE_IDS[c] for c in (3, 7, 13)])
def test_host_twin(nm, per, pts, kind, depth, case):
    method, steps, h, gain, drift = PA.CASES[case]
    host = PA.load_host()
    perm = np.ascontiguousarray(per.p, np.int32)
    adv = PA.advect_struct(method, steps, h, gain, drift, 2)
    got, traj = advect(nm, per, kind, depth, WIDE, pts, adv)
    want, wtraj = PA.host_advect(host, perm, kind, depth, pts, WIDE, adv)
    assert (bits(got) == bits(want)).all()
    assert (bits(traj) == bits(wtraj)).all()


# ---- trajectory, chaining, sizes -------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("every", [1, 2])
@pytest.mark.parametrize("kind,depth", [(PA.NOISE, 0), (PA.TURB, 7)], ids=["noise", "turb7"])
def test_trajectory(nm, per, pts, kind, depth, every):
    def run(steps, e=0):
        return advect(nm, per, kind, depth, WIDE, pts, PA.advect_struct(PA.RK4, steps, 0.37, 0.75, PA.DRIFT, e))
    final, traj = run(5, every)
    assert traj.shape == (5 // every + 1, len(pts), 3)
    assert (bits(traj[0]) == bits(pts)).all()
    for snap in range(traj.shape[0]):
        assert (bits(traj[snap]) == bits(run(snap * every)[0])).all(), snap
    assert (bits(final) == bits(run(5)[0])).all()
    assert not (bits(final) == bits(traj[-2])).all()


@pytest.mark.gpu
@pytest.mark.parametrize("method", [PA.EULER, PA.MIDPOINT, PA.RK4], ids=["euler", "midpoint", "rk4"])
@pytest.mark.parametrize("kind,depth", [(PA.TURB, 8), (PA.NOISE, 0)], ids=["turb8", "noise"])
def test_launch_chaining(nm, per, pts, kind, depth, method):
    """h is small: the longest trace here is 2 L + 1 steps of the cheapest kernel."""
    L = nm._lib.wn_perlin_advect_launch_steps(kind, depth, method)
    assert L >= 1
    h = -0.01

    def run(p, steps, e=0):
        return advect(nm, per, kind, depth, WIDE, p, PA.advect_struct(method, steps, h, 0.75, PA.DRIFT, e))
    whole = run(pts, L + 1)[0]
    first = run(pts, L)[0]
    assert (bits(whole) == bits(run(first, 1)[0])).all()
    assert not (bits(whole) == bits(first)).all()
    # three launches, with the snapshots at every second step crossing their boundaries, against the chained calls'
    steps = 2 * L + 1
    final, traj = run(pts, steps, 2)
    second, traj1 = run(first, L, 1)        # steps L .. 2 L, every one a snapshot
    assert (bits(final) == bits(run(second, 1)[0])).all()
    _, traj0 = run(pts, L, 1)               # steps 0 .. L
    chained = np.concatenate([traj0, traj1[1:]])      # the positions after steps 0 .. 2 L
    assert traj.shape[0] == steps // 2 + 1 == L + 1
    assert (bits(traj) == bits(chained[::2])).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 257])
@pytest.mark.parametrize("kind,depth", MAIN_KINDS, ids=[kind_id(k, d) for k, d in MAIN_KINDS])
def test_sizes(nm, per, pts, kind, depth, n):
    """One particle, and one particle more than a workgroup: each has the bits it has in the 350-point list."""
    adv = PA.advect_struct(PA.RK4, 3, 0.37, 1.0, PA.DRIFT, 1)
    full, full_traj = advect(nm, per, kind, depth, WIDE, pts, adv)
    got, traj = advect(nm, per, kind, depth, WIDE, pts[-n:], adv)
    assert (bits(got) == bits(full[-n:])).all()
    assert (bits(traj) == bits(full_traj[:, -n:])).all()


def stride_cap():
    """The workgroup cap of the kernel's grid-stride launch, read out of csrc/: kPerlinAdvectBlockCap if the kernel has one of
    its own, else wn::kStrideBlockCap, the default of wn::stride_blocks."""
    import test_stride_caps as sc
    own = sc.source("wn_perlin_advect.hip")
    if "kPerlinAdvectBlockCap" in own:
        assert "stride_blocks(n, kPerlinAdvectBlockCap)" in own
        return sc.constexpr("kPerlinAdvectBlockCap", own)
    assert re.search(r"dim3\(wn::stride_blocks\(n\)\)", own)
    return sc.constexpr("kStrideBlockCap", sc.source("wn_internal.hpp"))


@pytest.mark.gpu
def test_second_trip(nm, per):
    """n = cap * 256 + 3 * 256 + 77: the first 3 * 256 + 77 lanes take the loop a second time (about 100 MB per buffer).
    noise, midpoint, 2 steps, a snapshot per step, against the composition computed from wn_perlin_curl_points with the
    step arithmetic in numpy on the host."""
    n = stride_cap() * 256 + 3 * 256 + 77
    big = np.random.default_rng(7).uniform(-300.0, 300.0, (n, 3))
    method, steps, h, gain = PA.MIDPOINT, 2, 0.37, 0.75
    want = PA.trace_f64(method, steps, big, h, gain, PA.DRIFT, gpu_velocity(per, PA.NOISE, 0, WIDE))
    adv = PA.advect_struct(method, steps, h, gain, PA.DRIFT, 1)
    xin = Frame.holding(big, 0)
    out, traj = Frame(3 * n, 1, dtype=f64), Frame(3 * 3 * n, 0, dtype=f64)
    assert abi(nm, per, PA.NOISE, 0, offsets9(per, WIDE), xin.ptr, n, adv, out.ptr, traj.ptr) == 0, nm._lib.wn_last_error()
    assert (bits(out.result(what="xyz_out").reshape(n, 3)) == bits(want[-1])).all()
    path = traj.result(what="traj").reshape(3, n, 3)
    for s in range(3):
        assert (bits(path[s]) == bits(want[s])).all(), s
    assert (bits(xin.result(what="xyz_in").reshape(n, 3)) == bits(big)).all()


# ---- in place, exact output ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_in_place_and_overlap_refusal(nm, per, pts):
    import torch
    n = len(pts)
    off = offsets9(per, WIDE)
    L = nm._lib.wn_perlin_advect_launch_steps(PA.TURB, 7, PA.RK4)
    adv = PA.advect_struct(PA.RK4, L + 2, 0.05, 1.0, PA.DRIFT)      # two launches
    src = cuda(pts)
    out = torch.empty_like(src)
    assert abi(nm, per, PA.TURB, 7, off, nm._ptr(src), n, adv, nm._ptr(out)) == 0
    assert (bits(_np(src)) == bits(pts)).all()                      # the input is left alone
    buf = torch.zeros(3 * n + 64, dtype=torch.float64, device="cuda")
    buf[:3 * n] = src.reshape(-1)
    assert abi(nm, per, PA.TURB, 7, off, nm._ptr(buf), n, adv, nm._ptr(buf)) == 0
    assert (bits(_np(buf[:3 * n]).reshape(n, 3)) == bits(_np(out))).all()
    # any other overlap, in front or behind, by one double, by one record or by all but one double
    INVALID = nm._capi.WN_ERR_INVALID
    base = buf.data_ptr()
    for shift in (8, 24, 8 * (3 * n - 1)):
        assert abi(nm, per, PA.TURB, 7, off, C.c_void_p(base), n, adv, C.c_void_p(base + shift)) == INVALID
        assert abi(nm, per, PA.TURB, 7, off, C.c_void_p(base + shift), n, adv, C.c_void_p(base)) == INVALID
    assert b"overlaps" in nm._lib.wn_last_error()
    # ranges that touch do not overlap
    two = torch.zeros(6 * 16, dtype=torch.float64, device="cuda")
    assert abi(nm, per, PA.TURB, 7, off, nm._ptr(two), 16, adv, C.c_void_p(two.data_ptr() + 8 * 48)) == 0
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("lead", [0, 1, 2, 3])
@pytest.mark.parametrize("kind,depth", MAIN_KINDS, ids=[kind_id(k, d) for k, d in MAIN_KINDS])
def test_exact_output(nm, per, pts, kind, depth, lead):
    """Guard doubles around xyz_out and traj, from pointers 8 * lead bytes past a 256-byte boundary (the input list too);
    steps = L + 2 with a snapshot every second step: two launches."""
    n = len(pts)
    off = offsets9(per, WIDE)
    steps = nm._lib.wn_perlin_advect_launch_steps(kind, depth, PA.RK4) + 2
    snaps = steps // 2 + 1
    adv = PA.advect_struct(PA.RK4, steps, 0.05, 0.75, PA.DRIFT, 2)
    ref_out, ref_traj = advect(nm, per, kind, depth, WIDE, pts, adv)
    fin = Frame.holding(pts, lead)
    out, traj = Frame(3 * n, lead, dtype=f64), Frame(snaps * 3 * n, (lead + 1) % 4, dtype=f64)
    assert abi(nm, per, kind, depth, off, fin.ptr, n, adv, out.ptr, traj.ptr) == 0
    assert (bits(out.result(what="xyz_out")) == bits(ref_out.reshape(-1))).all()
    assert (bits(traj.result(what="traj")) == bits(ref_traj.reshape(-1))).all()
    assert (bits(fin.result(what="xyz_in")) == bits(pts.reshape(-1))).all()
    # without a trajectory nothing is read from or written to traj
    out2, untouched = Frame(3 * n, lead, dtype=f64), Frame(3 * n, lead, dtype=f64)
    adv.traj_every = 0
    assert abi(nm, per, kind, depth, off, fin.ptr, n, adv, out2.ptr, untouched.ptr) == 0
    assert (bits(out2.result(what="xyz_out")) == bits(ref_out.reshape(-1))).all()
    untouched.result(written=np.zeros(3 * n, bool), what="traj with traj_every == 0")


# ---- argument checks -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_argument_checks(nm, per):
    import torch
    INVALID, OK = nm._capi.WN_ERR_INVALID, nm._capi.WN_OK
    off = offsets9(per, WIDE)
    src = np.random.default_rng(3).uniform(-9.0, 9.0, (4, 3))
    p = cuda(src)
    o = torch.empty((4, 3), dtype=torch.float64, device="cuda")
    tr = torch.empty((8, 4, 3), dtype=torch.float64, device="cuda")
    good = PA.advect_struct(PA.RK4, 2, 0.1, 1.0, PA.ZERO, 1)
    pp, op, tp = nm._ptr(p), nm._ptr(o), nm._ptr(tr)
    for kind, depth in PA.KINDS:
        assert abi(nm, per, kind, depth, off, pp, 4, good, op, tp) == OK
    # kind, depth, perm, offsets and the buffers, as wn_perlin_curl_points_vec3 checks them
    assert abi(nm, per, 3, 0, off, pp, 4, good, op, tp) == INVALID
    assert abi(nm, per, -1, 0, off, pp, 4, good, op, tp) == INVALID
    assert abi(nm, per, PA.TURB, -1, off, pp, 4, good, op, tp) == INVALID
    assert abi(nm, per, PA.NOISE, -1, off, pp, 4, good, op, tp) == OK          # depth is read by turb only
    assert abi(nm, per, PA.FRACTAL, -1, off, pp, 4, good, op, tp) == OK
    assert abi(nm, None, PA.NOISE, 0, off, pp, 4, good, op, tp) == INVALID     # NULL perm
    assert abi(nm, per, PA.NOISE, 0, None, pp, 4, good, op, tp) == INVALID     # NULL offsets9_host
    assert abi(nm, per, PA.NOISE, 0, off, None, 4, good, op, tp) == INVALID    # NULL xyz_in_dev
    assert abi(nm, per, PA.NOISE, 0, off, pp, 4, good, None, tp) == INVALID    # NULL xyz_out_dev
    # wn_advect, with the wavelet call's messages
    assert abi(nm, per, PA.NOISE, 0, off, pp, 4, None, op, tp) == INVALID
    assert b"wn_advect is NULL" in nm._lib.wn_last_error()
    assert abi(nm, per, PA.NOISE, 0, off, pp, 4, good, op, None) == INVALID    # a trajectory without a buffer
    assert b"traj_dev is NULL" in nm._lib.wn_last_error()
    bad = [(PA.advect_struct(3, 2, 0.1, 1.0, PA.ZERO), b"method"), (PA.advect_struct(-1, 2, 0.1, 1.0, PA.ZERO), b"method"),
           (PA.advect_struct(PA.RK4, -1, 0.1, 1.0, PA.ZERO), b"steps"), (PA.advect_struct(PA.RK4, 2, 0.1, 1.0, PA.ZERO, -1), b"traj_every"),
           (PA.advect_struct(PA.RK4, 2, np.inf, 1.0, PA.ZERO), b"finite"), (PA.advect_struct(PA.RK4, 2, np.nan, 1.0, PA.ZERO), b"finite"),
           (PA.advect_struct(PA.RK4, 2, 0.1, -np.inf, PA.ZERO), b"finite"), (PA.advect_struct(PA.RK4, 2, 0.1, np.nan, PA.ZERO), b"finite")] + \
          [(PA.advect_struct(PA.RK4, 2, 0.1, 1.0, tuple(np.nan if i == c else 0.0 for i in range(3))), b"finite") for c in range(3)] + \
          [(PA.advect_struct(PA.RK4, 2, 0.1, 1.0, tuple(np.inf if i == c else 0.0 for i in range(3))), b"finite") for c in range(3)]
    for adv, word in bad:
        assert abi(nm, per, PA.NOISE, 0, off, pp, 4, adv, op, tp) == INVALID, (adv.method, adv.steps, adv.h, adv.gain, list(adv.drift))
        assert word in nm._lib.wn_last_error()
        assert abi(nm, per, PA.NOISE, 0, off, None, 0, adv, None, None) == INVALID   # ... whatever n is
    # nothing to do; and no trajectory: traj_dev is not looked at
    assert abi(nm, per, PA.NOISE, 0, off, None, 0, good, None, None) == OK
    assert abi(nm, per, PA.NOISE, 0, off, pp, 4, PA.advect_struct(PA.RK4, 2, 0.1, 1.0, PA.ZERO, 0), op, None) == OK
    # steps == 0: a bitwise copy, and snapshot 0 with it
    o.fill_(7.0)
    tr.fill_(7.0)
    assert abi(nm, per, PA.TURB, 7, off, pp, 4, PA.advect_struct(PA.RK4, 0, 0.1, 1.0, PA.DRIFT, 3), op, tp) == OK
    torch.cuda.synchronize()
    assert (bits(_np(o)) == bits(src)).all() and (bits(_np(tr[0])) == bits(src)).all() and (_np(tr[1:]) == 7.0).all()
    # the Python member
    with pytest.raises(ValueError):
        per.advect_curl(p, 0.1, 1, method="heun")
    with pytest.raises(ValueError):
        per.advect_curl(p, 0.1, 1, kind="worley")
    with pytest.raises(nm._capi.WnError):
        per.advect_curl(p, 0.1, -1)
    with pytest.raises(nm._capi.WnError):
        per.advect_curl(p, float("inf"), 1)
    assert per.advect_curl(torch.empty((0, 3), dtype=torch.float64, device="cuda"), 0.1, 3).shape == (0, 3)


# ---- the class surfaces ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_host_classes_match_the_c_abi(tmp_path):
    exe = tmp_path / "perlin_advect_api_check"
    src = os.path.join(HERE, "host_src", "perlin_advect_api_check.cpp")
    build = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                            "-I" + os.path.join(PKG, "host"), src, "-o", str(exe), "-L" + PKG, "-lwnoise_host",
                            "-lwnoise_hip", "-Wl,-rpath," + PKG], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run(["timeout", "-k", "10", "300", str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "mismatches 0" in run.stdout, run.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("kind,depth", [(PA.NOISE, 0), (PA.TURB, 7), (PA.TURB, 3), (PA.FRACTAL, 0)],
                         ids=["noise", "turb7", "turb3", "fractal"])
def test_python_mirror(nm, per, pts, kind, depth):
    """perlin.advect_curl returns the C ABI's bits: positional defaults (rk4, the default offsets, gain 1, no drift, no
    trajectory), and every argument given."""
    name = PA.KIND_NAMES[kind]
    got = per.advect_curl(cuda(pts), 0.37, 3, kind=name, depth=depth)
    assert got.dtype.is_floating_point and got.element_size() == 8 and got.shape == (len(pts), 3) and got.is_cuda
    want, _ = advect(nm, per, kind, depth, None, pts, PA.advect_struct(PA.RK4, 3, 0.37, 1.0, PA.ZERO))
    assert (bits(_np(got)) == bits(want)).all()
    got, traj = per.advect_curl(pts, -0.37, 3, name, depth, "midpoint", WIDE, 0.75, PA.DRIFT, trajectory_every=2)
    want, wtraj = advect(nm, per, kind, depth, WIDE, pts, PA.advect_struct(PA.MIDPOINT, 3, -0.37, 0.75, PA.DRIFT, 2))
    assert traj.shape == (2, len(pts), 3)
    assert (bits(_np(got)) == bits(want)).all() and (bits(_np(traj)) == bits(wtraj)).all()
