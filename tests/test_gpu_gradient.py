"""GPU: analytic gradients of 3-D wavelet noise (csrc/wn_wavelet_grad.hip) on point lists and dense grids.

 * points: the value channel has the bits of wn_eval3d_points / wn_multiband3d_points, all four channels the bits of the
   host's scalar evaluator (wnhost_eval3d_grad) and lie within G of the float64 reference (tests/_ref64_grad.py);
 * grids, WN_GRID_EXACT: channel 0 has the bits of the exact value grid, all four the bits of the point kernel at the
   lattice's float32 coordinates;
 * grids, default tier: every channel within G of the exact tier and of the float64 reference; a volume cut into
   z-slabs has the bits of the whole volume;
 * routing: ROUTES names the kernel each call must reach, on both sides of every edge of the brick kernel's regime
   (grad_sep_try); a child process runs the calls under `rocprofv3 --kernel-trace` and the traced names are compared;
 * host classes: tests/host_src/grad_api_check.cpp against the C ABI.

G = 1e-5 * |out_scale| (multiband: * sum_b |w_b| 2^(first_band+b+1) / out_div), absolute, per channel.
Run as `python tests/test_gpu_gradient.py --child` it is the routing child: the calls of ROUTES, one after the other.
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
import _ref64_grad  # noqa: E402

PKG = os.path.join(ROOT, "wavelet-noise-in-ray-tracing_amd")
INV = float(np.float32(1.0) / np.sqrt(np.float32(0.18402)))
W8 = [1.0, 0.5, 2.0, 1.0, 0.25, 1.5, 0.75, 1.0]

SEP = "grad3d_grid_sep_kernel<{}>"
DIRECT_PADDED, DIRECT_LINEAR = "grad3d_grid_direct_kernel<true>", "grad3d_grid_direct_kernel<false>"
POINTS = "grad3d_points_kernel<{},{}>"


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def load_tiles(wn):
    """Noise objects and their coefficients: t128 (128^3, seed 12345, generated on the device), t8 / t6 (tests/golden;
    6 is not a power of two) and the empty tile."""
    gold = np.load(os.path.join(HERE, "golden", "ref_vectors.npz"))
    objs, coefs = {}, {}
    n128 = wn.WaveletNoise(128, 12345)
    n128.generateNoiseTile3D()
    objs["t128"], coefs["t128"] = n128, n128.getNoiseCoefficients()
    for name, key in (("t8", "tile3d_8_7"), ("t6", "tile3d_5odd_11")):
        coefs[name] = gold[key]
        objs[name] = wn.WaveletNoise.from_coefficients(gold[key], 3)
    objs["empty"], coefs["empty"] = wn.WaveletNoise(128, 1), np.empty(0, np.float32)
    return objs, coefs


# ---- calls ---------------------------------------------------------------------------------------------------------------
# ("p", tile, npts)                                   evaluate3DGradient on npts random points
# ("mp", tile, npts, s, first, nb, w)                 WMultibandNoiseGradient
# ("g", tile, den, nx, ny, z0, z1, octave)            wavelet_gradient_volume: step 8 * 2^octave / den
# ("gs", tile, den, nx, ny, z0, z1, base_range, zc)   wn_eval3d_grad_grid from a GridSpec (octave 4, post 2);
#                                                     zc not None: WN_Z_CONST at zc
# ("m", tile, den, nx, ny, z0, z1, s, first, nb, w)   multiband_gradient_volume: band b has step 8 * 2^(first+b) / den
# ("mc", tile, den, nx, ny, zc, s, first, nb, w)      wn_multiband3d_grad_grid with WN_Z_CONST
def run_call(wn, objs, call, exact=False, out=None):
    """`out` (grid calls): a flat float32 device tensor of at least 4 * nz * ny * nx elements to write into, else a fresh
    one."""
    import torch
    nm = importlib.import_module("wavelet-noise-in-ray-tracing_amd.noise")
    kind, tile = call[0], objs[call[1]]
    if kind in ("p", "mp"):
        pts = torch.from_numpy(np.random.default_rng(call[2]).uniform(-300, 300, (call[2], 3)).astype(np.float32)).cuda()
        if kind == "p":
            return tile.evaluate3DGradient(pts)
        return tile.WMultibandNoiseGradient(pts, *call[3:])
    if kind == "g":
        return wn.wavelet_gradient_volume(tile, *call[2:], exact=exact, out=out)
    if kind == "m":
        den, nx, ny, z0, z1, s, first, nb, w = call[2:]
        return wn.multiband_gradient_volume(tile, den, nx, ny, z0, z1, s, first, nb, w, exact=exact, out=out)
    flags = nm.WN_GRID_EXACT if exact else nm.WN_GRID_DEFAULT
    if kind == "gs":
        den, nx, ny, z0, z1, rng_, zc = call[2:]
        g = wn.GridSpec(den, nx, ny, z0, z1, base_range=rng_, octave_scale=16.0, post_scale=2.0, out_scale=INV, flags=flags,
                        z_mode=nm.WN_Z_LATTICE if zc is None else nm.WN_Z_CONST, z_const=0.0 if zc is None else zc)
        out = nm._grad_out(g, out)
        gc = g.c()
        nm.check(nm._lib.wn_eval3d_grad_grid(tile._handle(3), C.byref(gc), nm._ptr(out), nm._stream()))
        return out[: 4 * g.nz * ny * nx].view(4, g.nz, ny, nx)
    assert kind == "mc", kind
    den, nx, ny, zc, s, first, nb, w = call[2:]
    g = wn.GridSpec(den, nx, ny, z_mode=nm.WN_Z_CONST, z_const=zc, flags=flags)
    out = nm._grad_out(g, out)
    gc = g.c()
    wa = (C.c_float * nb)(*[float(x) for x in w])
    nm.check(nm._lib.wn_multiband3d_grad_grid(tile._handle(3), C.byref(gc), float(s), int(first), int(nb), wa, 0.18402,
                                              nm._ptr(out), nm._stream()))
    return out[: 4 * ny * nx].view(4, 1, ny, nx)


def call_coords(call):
    """float32 coordinates (px, py, pz) of a grid call, in the order lattice_coord forms them."""
    kind = call[0]
    if kind == "g":
        den, nx, ny, z0, z1, octave = call[2:]
        os_ = np.float32(2.0 ** octave)
        return [_ref64.lattice_coords(np.arange(a, b), den, 4.0, os_, 2.0) for a, b in ((0, nx), (0, ny), (z0, z1))]
    if kind == "gs":
        den, nx, ny, z0, z1, rng_, zc = call[2:]
        px, py, pz = [_ref64.lattice_coords(np.arange(a, b), den, rng_, 16.0, 2.0) for a, b in ((0, nx), (0, ny), (z0, z1))]
        return px, py, (pz if zc is None else np.float32([zc]))
    if kind == "m":
        den, nx, ny, z0, z1 = call[2:7]
        return [_ref64.lattice_coords(np.arange(a, b), den) for a, b in ((0, nx), (0, ny), (z0, z1))]
    den, nx, ny, zc = call[2:6]
    return _ref64.lattice_coords(np.arange(nx), den), _ref64.lattice_coords(np.arange(ny), den), np.float32([zc])


def ref64_call(coef, call, zs=None):
    """The float64 reference of a grid call, on planes zs (indices into the slab) or all of them: [4, nz, ny, nx]."""
    px, py, pz = call_coords(call)
    if zs is not None:
        pz = pz[list(zs)]
    if call[0] in ("g", "gs"):
        return _ref64_grad.evaluate_lattice_grad(coef, px, py, pz) * INV
    s, first, nb, w = call[-4:]
    return _ref64_grad.multiband_lattice_grad(coef, px, py, pz, s, first, nb, w, 0.18402)


def call_tol(call):
    if call[0] in ("g", "gs"):
        return _ref64_grad.tolerance(INV)
    s, first, nb, w = call[-4:]
    return _ref64_grad.tolerance(1.0, (s, first, nb, w, 0.18402))


ROUTES = [
    # point lists: the padded tile, or the linear layout when the tile has none (the empty tile)
    ("points", ("p", "t128", 1000), POINTS.format("true", "false")),
    ("points_t6", ("p", "t6", 1000), POINTS.format("true", "false")),
    ("points_empty", ("p", "empty", 1000), POINTS.format("false", "false")),
    ("mb_points", ("mp", "t128", 1000, -16.0, 0, 5, W8[:5]), POINTS.format("true", "true")),
    ("mb_points_empty", ("mp", "empty", 1000, -16.0, 0, 5, W8[:5]), POINTS.format("false", "true")),
    # single band: 4 consecutive samples span at most two mids (step < 1/3), steps >= 0, a tile that is not empty
    ("step_1_3_in", ("g", "t128", 385, 256, 5, 0, 9, 4), SEP.format(1)),      # step .33247
    ("step_1_3_at", ("g", "t128", 384, 256, 5, 0, 9, 4), DIRECT_PADDED),      # step 1/3
    ("headline_slab", ("g", "t128", 512, 512, 8, 0, 9, 4), SEP.format(1)),   # step .25
    ("nx_998", ("g", "t128", 512, 998, 5, 0, 9, 4), SEP.format(1)),          # nx % 4 != 0: scalar stores
    ("narrow", ("g", "t128", 512, 5, 3, 0, 2, 4), SEP.format(1)),
    ("z0_neg", ("g", "t128", 512, 300, 6, -9, 4, 4), SEP.format(1)),
    ("tile6", ("g", "t6", 512, 260, 6, 0, 9, 4), SEP.format(1)),             # any tile size: the box wraps by modulo
    ("tile8", ("g", "t8", 512, 260, 6, 3, 12, 4), SEP.format(1)),
    ("empty_tile", ("g", "empty", 512, 64, 4, 0, 3, 4), DIRECT_LINEAR),
    ("step_pos", ("gs", "t128", 512, 256, 5, 0, 9, 4.0, None), SEP.format(1)),
    ("step_neg", ("gs", "t128", 512, 256, 5, 0, 9, -4.0, None), DIRECT_PADDED),
    ("zconst", ("gs", "t128", 512, 300, 7, 0, 1, 4.0, 2.0), SEP.format(1)),
    ("zconst_neg_step", ("gs", "t128", 512, 300, 7, 0, 1, -4.0, 2.0), DIRECT_PADDED),
    ("coarse", ("g", "t128", 64, 64, 8, 0, 9, 4), DIRECT_PADDED),            # step 2
    # several bands: the top band's step decides; no active band -> the exact kernel
    ("mb5_step_in", ("m", "t128", 385, 256, 5, 0, 9, -16.0, 0, 5, W8[:5]), SEP.format(5)),
    ("mb5_step_at", ("m", "t128", 384, 256, 5, 0, 9, -16.0, 0, 5, W8[:5]), DIRECT_PADDED),
    ("mb1", ("m", "t128", 512, 300, 6, 2, 11, -16.0, 2, 1, [1.0]), SEP.format(1)),
    ("mb2", ("m", "t128", 512, 300, 6, 2, 11, -16.0, 1, 2, W8[:2]), SEP.format(2)),
    ("mb3", ("m", "t128", 512, 300, 6, 2, 11, -16.0, -2, 3, W8[:3]), SEP.format(3)),
    ("mb4", ("m", "t128", 512, 300, 6, 2, 11, -16.0, 0, 4, W8[:4]), SEP.format(4)),
    ("mb5", ("m", "t128", 512, 512, 8, 0, 9, -16.0, 0, 5, W8[:5]), SEP.format(5)),
    ("mb6", ("m", "t128", 512, 300, 6, 2, 11, -16.0, -1, 6, W8[:6]), SEP.format(6)),
    ("mb7", ("m", "t128", 1024, 300, 6, 2, 11, -16.0, -1, 7, W8[:7]), SEP.format(7)),
    ("mb8", ("m", "t128", 4096, 300, 6, -4, 5, -16.0, 0, 8, W8), SEP.format(8)),
    ("mb_s_cut", ("m", "t128", 512, 300, 6, 0, 9, -2.5, 0, 5, W8[:5]), SEP.format(3)),   # s stops after 3 bands
    ("mb_none", ("m", "t128", 512, 300, 6, 0, 9, 0.0, 0, 5, W8[:5]), DIRECT_PADDED),    # s: no band runs
    ("mb_zero_w", ("m", "t128", 512, 300, 6, 0, 9, -16.0, 0, 3, [0.0] * 3), SEP.format(3)),
    ("mb_zconst", ("mc", "t128", 512, 300, 6, 0.37, -16.0, 0, 5, W8[:5]), SEP.format(5)),
    ("mb_tile6", ("m", "t6", 512, 300, 6, 0, 9, -16.0, -1, 4, W8[:4]), SEP.format(4)),
]
GRID_ROUTES = [r for r in ROUTES if r[1][0] not in ("p", "mp")]


def _child():
    import torch
    assert torch.cuda.is_available()
    wn = importlib.import_module("wavelet-noise-in-ray-tracing_amd")
    objs, _ = load_tiles(wn)
    torch.cuda.synchronize()
    for _name, call, _kernel in ROUTES:
        run_call(wn, objs, call)
        torch.cuda.synchronize()
    print(f"gradient dispatch child: {len(ROUTES)} calls")


_DEMANGLED = re.compile(r"(grad3d_[a-z_]+?_kernel)(?:<([^<>]*)>)?")
_MANGLED = re.compile(r"(grad3d_[a-z_]+?_kernel)(?:I((?:L[a-z]\d+E)+)E)?")


def kernel_label(name):
    """'grad3d_grid_sep_kernel<3>' / its mangled form -> 'grad3d_grid_sep_kernel<3>'; booleans as true / false; None for
    other kernels."""
    m = (_MANGLED if name.startswith("_Z") else _DEMANGLED).search(name)
    if not m:
        return None
    if not m.group(2):
        return m.group(1)
    if name.startswith("_Z"):
        args = [("true" if v == "1" else "false") if k == "b" else v for k, v in re.findall(r"L([a-z])(\d+)E", m.group(2))]
    else:
        args = [a.strip() for a in m.group(2).split(",")]
    return f"{m.group(1)}<{','.join(args)}>"


def test_kernel_label_parses_both_name_forms():
    assert kernel_label("_ZN12_GLOBAL__N_122grad3d_grid_sep_kernelILi3EEEvNS_11GradSepArgsE") == SEP.format(3)
    assert kernel_label("void (anonymous namespace)::grad3d_grid_sep_kernel<8>((anonymous namespace)::GradSepArgs)") == SEP.format(8)
    assert kernel_label("_ZN12_GLOBAL__N_120grad3d_points_kernelILb1ELb0EEEvNS_14GradPointsArgsE") == POINTS.format("true", "false")
    assert kernel_label("void (anonymous namespace)::grad3d_points_kernel<false, true>((anonymous namespace)::GradPointsArgs)") == \
        POINTS.format("false", "true")
    assert kernel_label("_ZN12_GLOBAL__N_125grad3d_grid_direct_kernelILb1EEEvNS_14GradDirectArgsE") == DIRECT_PADDED
    assert kernel_label("void (anonymous namespace)::grid3d_sep_kernel<1, 2>((anonymous namespace)::SepArgs)") is None


def test_route_table_covers_every_kernel():
    want = {SEP.format(nb) for nb in range(1, 9)} | {DIRECT_PADDED, DIRECT_LINEAR} | \
           {POINTS.format(p, m) for p in ("true", "false") for m in ("true", "false")}
    assert want <= {k for _, _, k in ROUTES}, want - {k for _, _, k in ROUTES}
    assert len({n for n, _, _ in ROUTES}) == len(ROUTES)


# ---- GPU -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wn():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU (the product has no CPU path)"
    return importlib.import_module("wavelet-noise-in-ray-tracing_amd")


@pytest.fixture(scope="module")
def tiles(wn):
    return load_tiles(wn)


@pytest.fixture(scope="module")
def host():
    lib = C.CDLL(os.path.join(PKG, "libwnoise_host.so"))
    FP = C.POINTER(C.c_float)
    lib.wnhost_eval3d_grad.restype = C.c_float
    lib.wnhost_eval3d_grad.argtypes = [FP, C.c_int, FP, FP]
    return lib


def host_grad(host, coef, pts):
    FP = C.POINTER(C.c_float)
    coef = np.ascontiguousarray(coef, np.float32)
    n = int(round(coef.size ** (1.0 / 3.0))) if coef.size else 0
    cp = coef.ctypes.data_as(FP) if coef.size else None
    pts = np.ascontiguousarray(pts, np.float32)
    out = np.empty((len(pts), 4), np.float32)
    g = np.empty(3, np.float32)
    for i in range(len(pts)):
        out[i, 0] = host.wnhost_eval3d_grad(cp, n, pts[i].ctypes.data_as(FP), g.ctypes.data_as(FP))
        out[i, 1:] = g
    return out


def _np(t):
    return t.detach().cpu().numpy()


def point_sets():
    rng = np.random.default_rng(21)
    return {"random": rng.uniform(-300.0, 300.0, (20000, 3)).astype(np.float32),
            "edges": _ref64.edge_points(3, 5000, 22)}


@pytest.mark.gpu
@pytest.mark.parametrize("tile", ["t128", "t8", "t6", "empty"])
@pytest.mark.parametrize("pset", ["random", "edges"])
def test_points(wn, tiles, host, tile, pset):
    import torch
    objs, coefs = tiles
    pts = point_sets()[pset]
    td = torch.from_numpy(pts).cuda()
    got = _np(objs[tile].evaluate3DGradient(td))
    val = _np(objs[tile].evaluate3D(td))
    assert got.shape == (len(pts), 4)
    assert (bits(got[:, 0]) == bits(val)).all()
    want = _ref64_grad.evaluate3d_grad_points(coefs[tile], pts)
    err = np.abs(got.astype(np.float64) - want).max(0)
    assert (err <= _ref64_grad.tolerance()).all(), err
    sample = np.random.default_rng(5).choice(len(pts), 1500, replace=False)
    assert (bits(got[sample]) == bits(host_grad(host, coefs[tile], pts[sample]))).all()
    if tile == "empty":
        assert (got == 0.0).all()


@pytest.mark.gpu
def test_points_long_list(wn, tiles, host):
    """A list of 2^20 + 12345 points: the value channel against wn_eval3d_points (whose long lists take the z-plane-ordered
    kernels, same bits), a quarter of the points against the float64 reference, a sample against the host."""
    import torch
    objs, coefs = tiles
    pts = np.random.default_rng(8).uniform(-300.0, 300.0, ((1 << 20) + 12345, 3)).astype(np.float32)
    td = torch.from_numpy(pts).cuda()
    got = _np(objs["t128"].evaluate3DGradient(td))
    assert (bits(got[:, 0]) == bits(_np(objs["t128"].evaluate3D(td)))).all()
    sub = slice(0, None, 4)
    err = np.abs(got[sub].astype(np.float64) - _ref64_grad.evaluate3d_grad_points(coefs["t128"], pts[sub])).max(0)
    assert (err <= _ref64_grad.tolerance()).all(), err
    sample = np.random.default_rng(6).choice(len(pts), 2000, replace=False)
    assert (bits(got[sample]) == bits(host_grad(host, coefs["t128"], pts[sample]))).all()


@pytest.mark.gpu
def test_points_reject_misaligned_output(wn, tiles):
    import torch
    nm = importlib.import_module("wavelet-noise-in-ray-tracing_amd.noise")
    objs, _ = tiles
    pts = torch.zeros((4, 3), dtype=torch.float32, device="cuda")
    out = torch.empty(20, dtype=torch.float32, device="cuda")
    rc = nm._lib.wn_eval3d_grad_points(objs["t128"]._handle(3), nm._ptr(pts), 4, C.c_void_p(out.data_ptr() + 4), nm._stream())
    assert rc == nm._capi.WN_ERR_INVALID
    rc = nm._lib.wn_eval3d_grad_points(objs["t128"]._handle(3), None, 4, nm._ptr(out), nm._stream())
    assert rc == nm._capi.WN_ERR_INVALID


MB_CASES = [(s, first, nb) for s in (-16.0, -2.5) for first in (0, -2) for nb in range(1, 9)]


@pytest.mark.gpu
@pytest.mark.parametrize("s,first,nb,zero", [c + (False,) for c in MB_CASES] + [(-16.0, 0, 3, True)],
                         ids=[f"s{s}_f{f}_nb{n}" for s, f, n in MB_CASES] + ["zero_weights"])
def test_multiband_points(wn, tiles, s, first, nb, zero):
    import torch
    objs, coefs = tiles
    w = [0.0] * nb if zero else [W8[(b + nb) % 8] for b in range(nb)]
    rng = np.random.default_rng(nb * 7 + first)
    pts = np.concatenate([rng.uniform(-300.0, 300.0, (3000, 3)), rng.uniform(-4.0, 4.0, (1000, 3))]).astype(np.float32)
    td = torch.from_numpy(pts).cuda()
    got = _np(objs["t128"].WMultibandNoiseGradient(td, s, first, nb, w))
    val = _np(objs["t128"].WMultibandNoise(td, s, first, nb, w))
    assert (bits(got[:, 0]) == bits(val)).all()
    want = _ref64_grad.multiband_grad_points(coefs["t128"], pts, s, first, nb, w, 0.18402)
    err = np.abs(got.astype(np.float64) - want).max(0)
    tol = _ref64_grad.tolerance(1.0, (s, first, nb, w, 0.18402))
    assert (err <= tol).all(), (err, tol)
    if zero:
        assert (got == 0.0).all()


# ---- grids ---------------------------------------------------------------------------------------------------------------
EXACT_CALLS = [
    ("g", "t128", 512, 100, 7, -3, 4, 4),
    ("g", "t128", 64, 64, 8, 0, 9, 4),                        # coarse
    ("gs", "t128", 512, 60, 5, 0, 1, 4.0, 2.0),               # WN_Z_CONST
    ("g", "t6", 512, 70, 5, 0, 6, 4),
    ("g", "empty", 512, 30, 3, 0, 2, 4),
    ("m", "t128", 512, 90, 5, 0, 6, -16.0, 0, 5, W8[:5]),
    ("m", "t128", 512, 40, 5, 2, 5, -2.5, -2, 8, W8),
    ("mc", "t128", 512, 50, 6, 0.37, -16.0, 0, 3, W8[:3]),
]


@pytest.mark.gpu
@pytest.mark.parametrize("call", EXACT_CALLS, ids=[f"{c[0]}_{c[1]}_{i}" for i, c in enumerate(EXACT_CALLS)])
def test_exact_grid_has_the_point_kernels_bits(wn, tiles, call):
    import torch
    nm = importlib.import_module("wavelet-noise-in-ray-tracing_amd.noise")
    objs, coefs = tiles
    tile = objs[call[1]]
    got = _np(run_call(wn, objs, call, exact=True))
    px, py, pz = call_coords(call)
    pts = np.stack(np.broadcast_arrays(px[None, None, :], py[None, :, None], pz[:, None, None]), -1).reshape(-1, 3)
    td = torch.from_numpy(np.ascontiguousarray(pts)).cuda()
    if call[0] in ("g", "gs"):
        pk = _np(tile.evaluate3DGradient(td)) * np.float32(INV)
        vol = _value_grid(wn, nm, tile, call)
    else:
        s, first, nb, w = call[-4:]
        pk = _np(tile.WMultibandNoiseGradient(td, s, first, nb, w))
        vol = _value_grid(wn, nm, tile, call)
    assert (bits(got[0]) == bits(vol)).all()
    assert (bits(got.reshape(4, -1).T) == bits(pk)).all()


def _value_grid(wn, nm, tile, call):
    """The matching WN_GRID_EXACT value grid."""
    import torch
    kind = call[0]
    if kind == "g":
        return _np(wn.wavelet_volume(tile, *call[2:], exact=True))
    if kind == "m":
        den, nx, ny, z0, z1, s, first, nb, w = call[2:]
        return _np(wn.multiband_volume(tile, den, nx, ny, z0, z1, s, first, nb, w, exact=True))
    if kind == "gs":
        den, nx, ny, z0, z1, rng_, zc = call[2:]
        g = wn.GridSpec(den, nx, ny, z0, z1, base_range=rng_, octave_scale=16.0, post_scale=2.0, out_scale=INV,
                        flags=nm.WN_GRID_EXACT, z_mode=nm.WN_Z_CONST, z_const=zc)
        out = g.empty()
        gc = g.c()
        nm.check(nm._lib.wn_eval3d_grid(tile._handle(3), C.byref(gc), nm._ptr(out), nm._stream()))
        return _np(out).reshape(1, ny, nx)
    den, nx, ny, zc, s, first, nb, w = call[2:]
    g = wn.GridSpec(den, nx, ny, z_mode=nm.WN_Z_CONST, z_const=zc, flags=nm.WN_GRID_EXACT)
    out = g.empty()
    gc = g.c()
    wa = (C.c_float * nb)(*[float(x) for x in w])
    nm.check(nm._lib.wn_multiband3d_grid(tile._handle(3), C.byref(gc), float(s), int(first), int(nb), wa, 0.18402,
                                         nm._ptr(out), nm._stream()))
    torch.cuda.synchronize()
    return _np(out).reshape(1, ny, nx)


@pytest.mark.gpu
@pytest.mark.parametrize("name,call,kernel", [pytest.param(n, c, k, id=n) for n, c, k in GRID_ROUTES])
def test_default_grid_values(wn, tiles, name, call, kernel):
    """Every channel of the default tier within G of WN_GRID_EXACT and of the float64 reference on the whole lattice."""
    objs, coefs = tiles
    fast = _np(run_call(wn, objs, call)).astype(np.float64)
    exact = _np(run_call(wn, objs, call, exact=True)).astype(np.float64)
    assert np.isfinite(fast).all()
    ref = ref64_call(coefs[call[1]], call) if call[1] != "empty" else np.zeros_like(fast)
    tol = call_tol(call)
    assert fast.shape == exact.shape == ref.shape
    for ch in range(4):
        e_fe = float(np.abs(fast[ch] - exact[ch]).max())
        e_fr = float(np.abs(fast[ch] - ref[ch]).max())
        e_er = float(np.abs(exact[ch] - ref[ch]).max())
        assert max(e_fe, e_fr, e_er) <= tol, (name, kernel, ch, e_fe, e_fr, e_er, tol)


@pytest.mark.gpu
def test_headline_lattice(wn, tiles):
    """512^3, tile 128, octave 4 (step 1/4): the whole volume within G of WN_GRID_EXACT, three whole z-planes within G of
    the float64 reference, channel 0 within 1e-5 of the value grid's default tier."""
    import torch
    objs, coefs = tiles
    fast = wn.wavelet_gradient_volume(objs["t128"], 512, 512, 512, 0, 512, 4)
    exact = wn.wavelet_gradient_volume(objs["t128"], 512, 512, 512, 0, 512, 4, exact=True)
    tol = _ref64_grad.tolerance(INV)
    e_fe = [float((fast[ch] - exact[ch]).abs().max()) for ch in range(4)]
    assert max(e_fe) <= tol, e_fe
    e_val = float((fast[0] - wn.wavelet_volume(objs["t128"], 512, 512, 512, 0, 512, 4)).abs().max())
    assert e_val <= 1e-5, e_val
    zs = (0, 255, 511)
    ref = ref64_call(coefs["t128"], ("g", "t128", 512, 512, 512, 0, 512, 4), zs)
    got = _np(fast[:, list(zs)]).astype(np.float64)
    e_fr = np.abs(got - ref).reshape(4, -1).max(1)
    assert (e_fr <= tol).all(), e_fr
    del fast, exact
    torch.cuda.empty_cache()


SLAB_CALLS = [("g", "t128", 512, 512, 16, 0, 64, 4), ("g", "t6", 300, 260, 9, -5, 30, 3),
              ("m", "t128", 512, 300, 9, 0, 40, -16.0, 0, 5, W8[:5])]


@pytest.mark.gpu
@pytest.mark.parametrize("call", SLAB_CALLS, ids=["single", "tile6", "multiband"])
def test_slabs_have_the_whole_volumes_bits(wn, tiles, call):
    objs, _ = tiles
    z0, z1 = call[5], call[6]
    whole = _np(run_call(wn, objs, call))
    cut = z0 + 11
    parts = [_np(run_call(wn, objs, call[:5] + (a, b) + call[7:])) for a, b in ((z0, cut), (cut, z1))]
    assert (bits(np.concatenate(parts, axis=1)) == bits(whole)).all()


@pytest.mark.gpu
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
    want = [k for _, _, k in ROUTES]
    assert len(got) == len(want), (len(got), len(want), got)
    wrong = [(name, k, g) for (name, _, k), g in zip(ROUTES, got) if k != g]
    assert not wrong, "calls served by another kernel than the table names (case, expected, ran): " + repr(wrong)


@pytest.mark.gpu
def test_host_classes_match_the_c_abi(tmp_path):
    exe = tmp_path / "grad_api_check"
    src = os.path.join(HERE, "host_src", "grad_api_check.cpp")
    build = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                            "-I" + os.path.join(PKG, "host"), src, "-o", str(exe), "-L" + PKG, "-lwnoise_host",
                            "-lwnoise_hip", "-Wl,-rpath," + PKG], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run(["timeout", "-k", "10", "300", str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "mismatches 0" in run.stdout, run.stdout


if __name__ == "__main__" and "--child" in sys.argv:
    _child()
