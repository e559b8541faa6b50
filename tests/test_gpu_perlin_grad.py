"""GPU: analytic gradients of perlin::noise, turb and fractal_noise (csrc/wn_perlin_grad.hip) on point lists and dense
grids.

 * points: every channel has the bits of the host evaluators (wnhost_perlin_grad / _turb_grad / _fractal_grad), the value
   channel those of wn_perlin_points / _points_vec3 / _turb_points / _fractal_points, and every point lies within
   1e-12 per octave of the long-double reference (tests/_ref64_perlin_grad.py);
 * grids: every channel has the bits of (float)(point entry point) * out_scale at the lattice's float32 coordinates and
   channel 0 those of wn_perlin_grid / _turb_grid / _fractal_grid -- on lattices that reach the run form with one cell
   per run (the BASELINE 512 x 512 x 8, octave 4), with several cells per run (coarse and non-dyadic steps) and the
   generic kernel (nx < 128, depth 12, depth 0); nx not a multiple of 4 and an unaligned output pointer; WN_Z_CONST;
   out_scale != 1; a volume cut into three uneven z-slabs has the whole volume's bits;
 * routing: one child process under `rocprofv3 --kernel-trace` shows the run-form gradient kernel on the 512-wide
   lattices and the generic one on the narrow and deep ones;
 * argument checks: a misaligned out4, NULL pointers and a negative depth are refused;
 * host classes: tests/host_src/perlin_grad_api_check.cpp against the C ABI.
"""
import csv
import ctypes as C
import glob
import importlib
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _ref64  # noqa: E402
import _ref64_perlin_grad as R  # noqa: E402

pytestmark = pytest.mark.gpu

PKG = os.path.join(ROOT, "wavelet-noise-in-ray-tracing_amd")
FP, DP, IP = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int)
SEEDS = [12345, 5489]


def bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _np(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def wn():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU (the product has no CPU path)"
    return importlib.import_module("wavelet-noise-in-ray-tracing_amd")


@pytest.fixture(scope="module")
def nm(wn):
    return importlib.import_module("wavelet-noise-in-ray-tracing_amd.noise")


@pytest.fixture(scope="module")
def perlins(wn):
    return {s: wn.perlin(s) for s in SEEDS}


@pytest.fixture(scope="module")
def host():
    lib = C.CDLL(os.path.join(PKG, "libwnoise_host.so"))
    for name, args in (("wnhost_perlin_grad", [IP, C.c_double, C.c_double, C.c_double, DP]),
                       ("wnhost_perlin_turb_grad", [IP, FP, C.c_int, DP]), ("wnhost_perlin_fractal_grad", [IP, FP, DP])):
        getattr(lib, name).restype = C.c_double
        getattr(lib, name).argtypes = args
    return lib


def host_records(host, perm, kind, pts, depth=0):
    pp = np.ascontiguousarray(perm, np.int32)
    ppp = pp.ctypes.data_as(IP)
    g = np.zeros(3)
    gp = g.ctypes.data_as(DP)
    out = np.empty((len(pts), 4))
    for i in range(len(pts)):
        if kind in ("noise64", "noise32"):
            x, y, z = (float(v) for v in pts[i])
            out[i, 0] = host.wnhost_perlin_grad(ppp, x, y, z, gp)
        elif kind == "turb":
            out[i, 0] = host.wnhost_perlin_turb_grad(ppp, pts[i].ctypes.data_as(FP), depth, gp)
        else:
            out[i, 0] = host.wnhost_perlin_fractal_grad(ppp, pts[i].ctypes.data_as(FP), gp)
        out[i, 1:] = g
    return out


def point_set(seed, dtype):
    rng = np.random.default_rng(seed)
    p = np.concatenate([rng.uniform(-300.0, 300.0, (30000, 3)), rng.uniform(-4.0, 4.0, (8000, 3)),
                        R.face_points(rng, 8000)])
    return np.ascontiguousarray(p.astype(dtype))


# ---- points ----------------------------------------------------------------------------------------------------------------
POINT_CASES = [("noise64", 0), ("noise32", 0), ("turb", 0), ("turb", 1), ("turb", 7), ("turb", 8), ("turb", 12),
               ("fractal", 6)]


@pytest.mark.parametrize("kind,depth", POINT_CASES, ids=[f"{k}_{d}" for k, d in POINT_CASES])
@pytest.mark.parametrize("seed", SEEDS)
def test_points(wn, perlins, host, seed, kind, depth):
    import torch
    p = perlins[seed]
    pts = point_set(seed + depth, np.float64 if kind == "noise64" else np.float32)
    td = torch.from_numpy(pts).cuda()
    if kind in ("noise64", "noise32"):
        got, val = _np(p.noise_gradient(td)), _np(p.noise(td))
    elif kind == "turb":
        got, val = _np(p.turb_gradient(td, depth)), _np(p.turb(td, depth))
    else:
        got, val = _np(p.fractal_noise_gradient(td)), _np(p.fractal_noise(td))
    assert got.shape == (len(pts), 4) and got.dtype == np.float64
    assert (bits64(got[:, 0]) == bits64(val)).all()
    sample = np.random.default_rng(5).choice(len(pts), 6000, replace=False)
    sample[:200] = np.arange(len(pts) - 200, len(pts))  # face points among them
    want_host = host_records(host, p.p, kind, pts[sample], depth)
    assert (bits64(got[sample]) == bits64(want_host)).all()
    rkind = "noise" if kind.startswith("noise") else kind
    want, s = R.eval_records(p.p, rkind, pts, depth)
    keep = np.ones(len(pts), bool)
    if kind == "turb" and depth:
        keep = (np.abs(s) >= 1e-10) | (s == 0.0)
    err = np.abs(got - want)[keep].max(0)
    print(kind, depth, seed, "max |gpu - reference| per channel", err)
    assert (err <= R.bound(rkind, depth)).all(), err
    if kind == "turb" and depth == 0:
        assert (got == 0.0).all()


# ---- grids -----------------------------------------------------------------------------------------------------------------
def _filled(count):
    import torch
    return torch.full((count,), float("nan"), dtype=torch.float32, device="cuda")


def run_grid(wn, nm, p, call, value=False, z=None, offset=0):
    """One dense-grid call.  call = (kind, depth, den, nx, ny, z0, z1, octave, z_const or None, out_scale)."""
    kind, depth, den, nx, ny, z0, z1, octave, zc, scale = call
    if z is not None:
        z0, z1 = z
    g = wn.GridSpec(den, nx, ny, z0, z1, octave_scale=float(np.float32(2.0 ** octave)), out_scale=scale,
                    z_mode=nm.WN_Z_LATTICE if zc is None else nm.WN_Z_CONST, z_const=0.0 if zc is None else zc)
    vol = g.nz * ny * nx
    chans = 1 if value else 4
    buf = _filled(chans * vol + offset + 8)
    out = C.c_void_p(buf.data_ptr() + 4 * offset)
    gc = g.c()
    lib, st = nm._lib, nm._stream()
    if kind == "noise":
        fn = lib.wn_perlin_grid if value else lib.wn_perlin_grad_grid
        nm.check(fn(p._h, C.byref(gc), out, st))
    elif kind == "turb":
        fn = lib.wn_perlin_turb_grid if value else lib.wn_perlin_turb_grad_grid
        nm.check(fn(p._h, C.byref(gc), depth, out, st))
    else:
        fn = lib.wn_perlin_fractal_grid if value else lib.wn_perlin_fractal_grad_grid
        nm.check(fn(p._h, C.byref(gc), out, st))
    o = _np(buf)
    assert np.isnan(o[:offset]).all() and np.isnan(o[offset + chans * vol:]).all()  # nothing outside the volumes
    return o[offset:offset + chans * vol].reshape(chans, g.nz, ny, nx)


def lattice_points(call):
    kind, depth, den, nx, ny, z0, z1, octave, zc, scale = call
    os_ = np.float32(2.0 ** octave)
    px, py = (_ref64.lattice_coords(np.arange(k), den, 4.0, os_, 1.0) for k in (nx, ny))
    pz = _ref64.lattice_coords(np.arange(z0, z1), den, 4.0, os_, 1.0) if zc is None else np.float32([zc])
    pts = np.stack(np.broadcast_arrays(px[None, None, :], py[None, :, None], pz[:, None, None]), -1).reshape(-1, 3)
    return np.ascontiguousarray(pts, np.float32)


# (kind, depth, den, nx, ny, z0, z1, octave, z_const or None, out_scale)
GRIDS = {
    # the run form, one cell per run: the BASELINE lattice (step 1/8) and turb / fractal_noise on p = (i/den)*4
    "noise_baseline": ("noise", 0, 512, 512, 512, 0, 8, 4, None, 1.0),
    "turb7_baseline": ("turb", 7, 512, 512, 64, 0, 8, 0, None, 1.0),
    "turb8_scaled": ("turb", 8, 512, 512, 24, 3, 6, 0, None, -2.5),
    "turb1": ("turb", 1, 512, 256, 9, 0, 2, 2, None, 1.0),
    "fractal": ("fractal", 6, 512, 512, 40, 0, 4, 0, None, 0.75),
    # the run form, several cells per run: a coarse dyadic step (2 per sample), and steps that are no power of two, so
    # that the lanes of a wave change cells at different samples
    "noise_coarse": ("noise", 0, 512, 512, 20, 0, 3, 8, None, 1.0),
    "noise_nondyadic": ("noise", 0, 300, 300, 17, -2, 3, 5, None, 1.0),
    "turb5_nondyadic": ("turb", 5, 91, 200, 11, 0, 3, 2, None, 1.5),
    "fractal_nondyadic": ("fractal", 6, 77, 131, 9, 1, 3, 3, None, 1.0),
    # rows that are no multiple of 4 samples, negative planes
    "noise_odd_rows": ("noise", 0, 512, 515, 10, -3, 2, 4, None, 1.0),
    # WN_Z_CONST
    "noise_zconst": ("noise", 0, 512, 512, 33, 0, 1, 4, 16.0, 1.0),
    "turb7_zconst": ("turb", 7, 512, 384, 12, 0, 1, 0, 0.37, 2.0),
    # the generic kernel: narrow rows, depth 12, depth 0
    "noise_narrow": ("noise", 0, 64, 64, 30, 0, 5, 3, None, 1.0),
    "turb7_narrow": ("turb", 7, 100, 100, 7, -1, 2, 0, None, -0.5),
    "turb12_deep": ("turb", 12, 512, 512, 6, 0, 2, 0, None, 1.0),
    "turb0": ("turb", 0, 512, 512, 4, 0, 2, 0, None, 1.0),
    "fractal_narrow": ("fractal", 6, 50, 50, 13, 0, 3, 1, None, 3.0),
}


def point_records(p, call, pts):
    import torch
    td = torch.from_numpy(pts).cuda()
    kind, depth = call[0], call[1]
    if kind == "noise":
        return p.noise_gradient(td)
    if kind == "turb":
        return p.turb_gradient(td, depth)
    return p.fractal_noise_gradient(td)


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("name", sorted(GRIDS))
def test_grid_has_the_point_kernels_bits(wn, nm, perlins, name, offset):
    import torch
    call = GRIDS[name]
    p = perlins[12345]
    got = run_grid(wn, nm, p, call, offset=offset)
    assert (bits32(got[0]) == bits32(run_grid(wn, nm, p, call, value=True)[0])).all()
    pts = lattice_points(call)
    rec = point_records(p, call, pts)
    pk = _np(rec.to(torch.float32)) * np.float32(call[9])  # (float)channel * out_scale
    assert (bits32(got.reshape(4, -1).T) == bits32(pk)).all()
    if call[0] == "turb" and call[1] == 0:
        assert (got == 0.0).all()


@pytest.mark.parametrize("name", ["noise_baseline", "turb7_baseline", "fractal_nondyadic", "turb12_deep"])
def test_grid_is_within_bound_of_the_reference(wn, nm, perlins, name):
    """(float)channel * out_scale rounds twice in float32: 2^-23 relative on top of the fp64 bound."""
    call = GRIDS[name]
    kind, depth, scale = call[0], call[1], call[9]
    p = perlins[12345]
    got = run_grid(wn, nm, p, call).reshape(4, -1).T.astype(np.float64)
    pts = lattice_points(call)
    want, s = R.eval_records(p.p, kind, pts, depth)
    keep = np.ones(len(pts), bool) if s is None else (np.abs(s) >= 1e-10) | (s == 0.0)
    err = np.abs(got - want * scale)
    tol = (R.bound(kind, depth) + np.abs(want) * 2.0 ** -23) * abs(scale)
    assert (err <= tol)[keep].all(), float((err - tol)[keep].max())


@pytest.mark.parametrize("name", ["noise_baseline", "turb7_baseline", "noise_nondyadic", "turb7_narrow"])
def test_slabs_have_the_whole_volumes_bits(wn, nm, perlins, name):
    call = list(GRIDS[name])
    call[5], call[6] = -5, 14  # 19 planes
    call[4] = min(call[4], 24)
    call = tuple(call)
    p = perlins[5489]
    whole = run_grid(wn, nm, p, call)
    parts = [run_grid(wn, nm, p, call, z=z) for z in ((-5, -4), (-4, 7), (7, 14))]
    assert (bits32(np.concatenate(parts, axis=1)) == bits32(whole)).all()


def test_volume_helpers(wn, perlins):
    p = perlins[12345]
    got = _np(wn.perlin_gradient_volume(p, 512, 512, 16, 0, 3, 4))
    assert got.shape == (4, 3, 16, 512) and np.isfinite(got).all()
    assert (bits32(got[0]) == bits32(_np(wn.perlin_volume(p, 512, 512, 16, 0, 3, 4)))).all()
    got = _np(wn.turb_gradient_volume(p, 512, 512, 16, 0, 3, 7))
    assert got.shape == (4, 3, 16, 512) and np.isfinite(got).all()
    assert (bits32(got[0]) == bits32(_np(wn.turb_volume(p, 512, 512, 16, 0, 3, 7)))).all()


# ---- routing -----------------------------------------------------------------------------------------------------------------
RUN, GENERIC = "perlin_grad_grid_run_kernel<{}>", "perlin_grad_grid_generic_kernel"
ROUTES = [("noise_baseline", RUN.format(0)), ("turb7_baseline", RUN.format(1)), ("turb8_scaled", RUN.format(1)),
          ("fractal", RUN.format(2)), ("noise_coarse", RUN.format(0)), ("noise_nondyadic", RUN.format(0)),
          ("noise_odd_rows", RUN.format(0)), ("turb7_zconst", RUN.format(1)), ("noise_narrow", GENERIC),
          ("turb7_narrow", GENERIC), ("turb12_deep", GENERIC), ("turb0", GENERIC), ("fractal_narrow", GENERIC)]


def kernel_label(name):
    m = re.search(r"perlin_grad_grid_(run|generic)_kernel(?:<(\d+)>|ILi(\d+)E)?", name)
    if not m:
        return None
    if m.group(1) == "generic":
        return GENERIC
    return RUN.format(m.group(2) if m.group(2) is not None else m.group(3))


def test_kernel_label_parses_both_name_forms():
    assert kernel_label("void (anonymous namespace)::perlin_grad_grid_run_kernel<1>((anonymous namespace)::PerlinGradGridArgs)") == RUN.format(1)
    assert kernel_label("_ZN12_GLOBAL__N_127perlin_grad_grid_run_kernelILi2EEEvNS_18PerlinGradGridArgsE") == RUN.format(2)
    assert kernel_label("_ZN12_GLOBAL__N_131perlin_grad_grid_generic_kernelENS_18PerlinGradGridArgsE") == GENERIC
    assert kernel_label("void (anonymous namespace)::perlin_grid_run_kernel<0, 8>((anonymous namespace)::PerlinGridArgs)") is None


def test_routes_reach_the_kernels_they_name(tmp_path):
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    assert os.path.exists(prof), "rocprofv3 is needed to observe which kernel ran"
    out_dir = tmp_path / "trace"
    cmd = ["timeout", "-k", "10", "300", prof, "--kernel-trace", "--output-format", "csv", "-d", str(out_dir),
           "--", sys.executable, os.path.abspath(__file__), "--child"]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
    assert res.returncode == 0, f"exit {res.returncode}\n{res.stdout[-3000:]}\n{res.stderr[-3000:]}"
    files = glob.glob(str(out_dir / "**" / "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, (files, res.stdout[-2000:])
    with open(files[0], newline="") as f:
        rows = list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    got = [lab for lab in (kernel_label(r["Kernel_Name"]) for r in rows) if lab is not None]
    want = [k for _, k in ROUTES]
    assert got == want, list(zip([n for n, _ in ROUTES], want, got))


def _child():
    import torch
    wn_ = importlib.import_module("wavelet-noise-in-ray-tracing_amd")
    nm_ = importlib.import_module("wavelet-noise-in-ray-tracing_amd.noise")
    p = wn_.perlin(12345)
    for name, _ in ROUTES:
        run_grid(wn_, nm_, p, GRIDS[name])
    torch.cuda.synchronize()


# ---- argument checks ---------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments(wn, nm, perlins):
    import torch
    lib, st, ok, bad = nm._lib, nm._stream(), nm._capi.WN_OK, nm._capi.WN_ERR_INVALID
    h = perlins[12345]._h
    p32 = torch.zeros((4, 3), dtype=torch.float32, device="cuda")
    p64 = torch.zeros((4, 3), dtype=torch.float64, device="cuda")
    out = torch.empty(40, dtype=torch.float64, device="cuda")
    mis = C.c_void_p(out.data_ptr() + 8)
    # a misaligned out4
    assert lib.wn_perlin_grad_points(h, nm._ptr(p64), 4, mis, st) == bad
    assert lib.wn_perlin_grad_points_vec3(h, nm._ptr(p32), 4, mis, st) == bad
    assert lib.wn_perlin_turb_grad_points(h, nm._ptr(p32), 4, 7, mis, st) == bad
    assert lib.wn_perlin_fractal_grad_points(h, nm._ptr(p32), 4, mis, st) == bad
    # NULL pointers; n == 0 with NULL pointers
    assert lib.wn_perlin_grad_points(h, None, 4, nm._ptr(out), st) == bad
    assert lib.wn_perlin_grad_points(h, nm._ptr(p64), 4, None, st) == bad
    assert lib.wn_perlin_grad_points(None, nm._ptr(p64), 4, nm._ptr(out), st) == bad
    assert lib.wn_perlin_grad_points_vec3(h, None, 4, nm._ptr(out), st) == bad
    assert lib.wn_perlin_turb_grad_points(h, None, 4, 7, nm._ptr(out), st) == bad
    assert lib.wn_perlin_fractal_grad_points(h, nm._ptr(p32), 4, None, st) == bad
    assert lib.wn_perlin_grad_points(h, None, 0, None, st) == ok
    assert lib.wn_perlin_turb_grad_points(h, None, 0, 7, None, st) == ok
    # a negative depth
    assert lib.wn_perlin_turb_grad_points(h, nm._ptr(p32), 4, -1, nm._ptr(out), st) == bad
    g = wn.GridSpec(64, 4, 2, 0, 1).c()
    f32 = torch.empty(64, dtype=torch.float32, device="cuda")
    assert lib.wn_perlin_turb_grad_grid(h, C.byref(g), -1, nm._ptr(f32), st) == bad
    assert lib.wn_perlin_grad_grid(h, C.byref(g), None, st) == bad
    assert lib.wn_perlin_grad_grid(h, None, nm._ptr(f32), st) == bad
    assert lib.wn_perlin_grad_grid(None, C.byref(g), nm._ptr(f32), st) == bad
    assert lib.wn_perlin_fractal_grad_grid(h, C.byref(g), None, st) == bad
    # an empty lattice is fine, with or without an output pointer
    e = wn.GridSpec(64, 4, 2, 3, 3).c()
    assert lib.wn_perlin_grad_grid(h, C.byref(e), None, st) == ok
    assert lib.wn_perlin_turb_grad_grid(h, C.byref(e), 7, None, st) == ok
    torch.cuda.synchronize()


# ---- host classes --------------------------------------------------------------------------------------------------------------
def test_host_classes_match_the_c_abi(tmp_path):
    exe = tmp_path / "perlin_grad_api_check"
    src = os.path.join(HERE, "host_src", "perlin_grad_api_check.cpp")
    build = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                            "-I" + os.path.join(PKG, "host"), src, "-o", str(exe), "-L" + PKG, "-lwnoise_host",
                            "-lwnoise_hip", "-Wl,-rpath," + PKG], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run(["timeout", "-k", "10", "300", str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "mismatches 0" in run.stdout, run.stdout


if __name__ == "__main__" and "--child" in sys.argv:
    _child()
