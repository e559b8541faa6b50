"""GPU: WMultibandNoise with a footprint per point (include/wnoise_footprint.h, csrc/wn_wavelet_footprint.hip).

 1. short lists (n = 4099): the five entry points have the bits of the host evaluator (wnhost_multiband3d_footprint,
    wnhost_wavelet_multiband_texture_value) per point and channel; value and gradient lie within the tolerance of
    tests/test_footprint_host.py of the float64 reference (tests/_ref64_footprint.py);
 2. agreement with the uniform ABI: the points that share a footprint s, sent to wn_multiband3d_points and its twins with
    that s, give the same bits -- every point without fade, and with it the points whose active bands all have f_b == 1
    (integer-valued s among them);
 3. list independence: a list of 16 * 4096 + 4096 + 1000 points (where the point kernels of wn_wavelet_points.hip change
    to their chunked routes; this feature has one kernel for every length) has the bits of the same points sent in shorter
    slices, for four orders of s, also under a mask of ~40 % active points;
 4. output frame (tests/_frame.py): from float-aligned, not 16-byte-aligned xyz, s and out exactly the n (or the active)
    records are written; a misaligned out4 is refused;
 5. argument checks;
 6. host classes (tests/host_src/footprint_api_check.cpp) and the Python classes against the C ABI.
"""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _frame  # noqa: E402
import _ref64  # noqa: E402
import _ref64_footprint as F  # noqa: E402

PKG = os.path.join(ROOT, "wavelet-noise-in-ray-tracing_amd")
pytestmark = pytest.mark.gpu

VAR, VAR_PROJ = 0.18402, 0.296
KINDS = ("value", "proj", "grad", "proj_grad", "tex")
CHANNELS = {"value": 1, "proj": 1, "grad": 4, "proj_grad": 4, "tex": 1}
SCALE = 0.37                      # the texture's scale
SORT_MIN = 16 * 4096              # where the uniform point entry points change to their chunked kernels (kSortMinPoints)
N_SHORT = 4099
N_LONG = SORT_MIN + 4096 + 1000   # one chunk longer than that, and a ragged tail


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def wn():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU (the product has no CPU path)"
    return importlib.import_module("wavelet-noise-in-ray-tracing_amd")


@pytest.fixture(scope="module")
def nm(wn):
    return importlib.import_module("wavelet-noise-in-ray-tracing_amd.noise")


@pytest.fixture(scope="module")
def tiles(wn):
    """The tiles of tests/test_footprint_host.py (128 and 6, filtered in float64 from Gaussian fields) and the empty one."""
    coefs = {f"t{n}": _ref64.tile(_ref64.tile_fields(n, 3, 12345)["gauss"], n, 3).astype(np.float32) for n in (128, 6)}
    objs = {k: wn.WaveletNoise.from_coefficients(c, 3) for k, c in coefs.items()}
    objs["empty"], coefs["empty"] = wn.WaveletNoise(128, 1), None
    return objs, coefs


@pytest.fixture(scope="module")
def host():
    return F.bind_host(C.CDLL(os.path.join(PKG, "libwnoise_host.so")))


def _p(x):
    if x is None or isinstance(x, C.c_void_p):
        return x
    return C.c_void_p(x.data_ptr())


def abi(nm, kind, handle, xyz, nrm, one, s, active, n, first, nb, w, fade, out, var=None):
    """One call of the entry point of `kind`; pointers are tensors, c_void_p or None.  Returns the status."""
    lib = nm._lib
    wa = (C.c_float * max(1, len(w)))(*[float(x) for x in w]) if w is not None else None   # (nb may be out of range)
    st = nm._stream()
    if kind == "tex":
        return lib.wn_wavelet_multiband_texture_points(handle, SCALE, first, nb, wa, VAR if var is None else var, fade,
                                                       _p(xyz), _p(s), _p(active), n, _p(out), st)
    if kind in ("value", "grad"):
        fn = lib.wn_multiband3d_footprint_points if kind == "value" else lib.wn_multiband3d_footprint_grad_points
        return fn(handle, _p(xyz), _p(s), n, first, nb, wa, VAR if var is None else var, fade, _p(out), st)
    fn = (lib.wn_multiband3d_projected_footprint_points if kind == "proj"
          else lib.wn_multiband3d_projected_footprint_grad_points)
    return fn(handle, _p(xyz), _p(nrm), one, _p(s), n, first, nb, wa, VAR_PROJ if var is None else var, fade, _p(out), st)


def run(nm, kind, tile, pts, nrs, s, first, nb, w, fade, one=0, active=None, fill=None):
    """The entry point of `kind` on host arrays: (n, channels) float32.  `fill`: the value the output holds before."""
    import torch
    n = len(pts)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    out = torch.full((n, CHANNELS[kind]), float("nan") if fill is None else fill, dtype=torch.float32, device="cuda")
    rc = abi(nm, kind, tile._handle(3), d(pts), d(nrs) if kind.startswith("proj") else None, one, d(s),
             d(active) if active is not None else None, n, first, nb, w, fade, out)
    assert rc == 0, nm._lib.wn_last_error()
    return out.cpu().numpy()


def host_records(host, coef, pts, nrs, s, first, nb, w, fade):
    """What the host evaluator gives for every kind: {kind: (n, channels) float32} (each evaluator runs once)."""
    rec, val = F.host_footprint(host, coef, pts, None, s, first, nb, w, VAR, fade)
    prec, pval = F.host_footprint(host, coef, pts, nrs, s, first, nb, w, VAR_PROJ, fade)
    tex = F.host_texture(host, coef, SCALE, pts, s, first, nb, w, VAR, fade)
    return {"value": val[:, None], "grad": rec, "proj": pval[:, None], "proj_grad": prec, "tex": tex[:, None]}


# ---- 1. short lists ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb,first,fade", F.CASES, ids=F.CASE_IDS)
def test_short_lists_have_the_host_evaluators_bits(nm, tiles, host, nb, first, fade):
    objs, coefs = tiles
    tile = "t6" if (nb + first + fade) % 2 else "t128"
    w = F.weights(nb, first)
    pts = F.points(first, nb, N_SHORT, 40 + nb + first)
    s = F.footprints(first, nb, N_SHORT, 50 + nb + first)
    nrs = F.normals(N_SHORT, 80 + nb)
    got = {k: run(nm, k, objs[tile], pts, nrs, s, first, nb, w, fade) for k in KINDS}
    want = host_records(host, coefs[tile], pts, nrs, s, first, nb, w, fade)
    for k in KINDS:
        same = bits(got[k]) == bits(want[k])
        assert same.all(), (k, int((~same).sum()), np.flatnonzero(~same.all(1))[:5])
    assert (bits(got["grad"][:, 0]) == bits(got["value"][:, 0])).all()
    assert (bits(got["proj_grad"][:, 0]) == bits(got["proj"][:, 0])).all()
    # the float64 reference: every point of the evaluate3D kinds, a sample of the projected ones
    want, _ = F.multiband_footprint_points(coefs[tile], pts, None, s, first, nb, w, VAR, fade)
    tol = F.tolerance(s, first, nb, w, VAR)
    err = np.abs(got["grad"].astype(np.float64) - want)
    assert (err <= tol[:, None]).all(), (err.max(0), tol.max())
    sub = slice(0, 256)
    want, bound = F.multiband_footprint_points(coefs[tile], pts[sub], nrs[sub], s[sub], first, nb, w, VAR_PROJ, fade)
    err = np.abs(got["proj_grad"][sub].astype(np.float64) - want)
    assert (err <= bound).all(), (err / bound).max(0)
    none = F.active_count(s, first, nb) == 0
    assert none.any()
    for k in KINDS:
        assert (got[k][none] == (0.5 if k == "tex" else 0.0)).all(), k


@pytest.mark.parametrize("fade", [0, 1])
def test_short_list_masked_texture(nm, tiles, host, fade):
    objs, coefs = tiles
    first, nb = 0, 5
    w = F.weights(nb, first)
    pts = F.points(first, nb, N_SHORT, 9)
    s = F.footprints(first, nb, N_SHORT, 10)
    active = (np.random.default_rng(11).random(N_SHORT) < 0.4).astype(np.uint8)
    got = run(nm, "tex", objs["t128"], pts, None, s, first, nb, w, fade, active=active, fill=-7.0)[:, 0]
    on = active != 0
    want = F.host_texture(host, coefs["t128"], SCALE, pts[on], s[on], first, nb, w, VAR, fade)
    assert (bits(got[on]) == bits(want)).all()
    assert (got[~on] == -7.0).all()


# ---- 2. agreement with the uniform ABI -----------------------------------------------------------------------------------
def few_footprints(first, nb, count, seed, distinct=64):
    """F.footprints with at most `distinct` + 1 different values (NaN is one of them), so that one uniform call per
    value stays cheap: the first `distinct` different values, and the rest replaced by draws among them."""
    s = F.footprints(first, nb, count, seed)
    keep = []
    for v in s:
        if not np.isnan(v) and not any(bits(np.float32(v))[0] == bits(np.float32(k))[0] for k in keep):
            keep.append(v)
        if len(keep) == distinct:
            break
    keep = np.array(keep, np.float32)
    known = np.isin(bits(s), bits(keep)) | np.isnan(s)
    return np.where(known, s, np.random.default_rng(seed).choice(keep, count)).astype(np.float32)


def uniform_call(nm, kind, tile, pts, nrs, one, sval, first, nb, w):
    """wn_multiband3d_points / _projected_points / _grad_points / _projected_grad_points at the one footprint sval."""
    import torch
    lib, n = nm._lib, len(pts)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    out = torch.full((n, CHANNELS[kind]), float("nan"), dtype=torch.float32, device="cuda")
    wa = (C.c_float * max(1, nb))(*[float(x) for x in w[:nb]])
    h, st, x = tile._handle(3), nm._stream(), d(pts)
    if kind in ("value", "grad"):
        fn = lib.wn_multiband3d_points if kind == "value" else lib.wn_multiband3d_grad_points
        rc = fn(h, _p(x), n, float(sval), first, nb, wa, VAR, _p(out), st)
    else:
        fn = lib.wn_multiband3d_projected_points if kind == "proj" else lib.wn_multiband3d_projected_grad_points
        rc = fn(h, _p(x), _p(d(nrs)), one, n, float(sval), first, nb, wa, VAR_PROJ, _p(out), st)
    assert rc == 0, lib.wn_last_error()
    return out.cpu().numpy()


@pytest.mark.parametrize("one", [0, 1], ids=["normal_per_point", "one_normal"])
@pytest.mark.parametrize("fade", [0, 1], ids=["hard", "fade"])
@pytest.mark.parametrize("nb,first", [(5, 0), (8, -2), (1, 3)])
def test_points_that_share_a_footprint_have_the_uniform_calls_bits(nm, tiles, nb, first, fade, one):
    objs, _ = tiles
    tile = objs["t128"]
    w = F.weights(nb, first)
    n = 2048 + 3
    pts = F.points(first, nb, n, 21 + nb)
    s = few_footprints(first, nb, n, 22 + nb)
    nrs = F.normals(1 if one else n, 23)
    kinds = KINDS[:4] if not one else ("proj", "proj_grad")       # one_normal only exists on the projected entry points
    got = {k: run(nm, k, tile, pts, nrs, s, first, nb, w, fade, one=one) for k in kinds}
    active, f = F.band_factors(s, first, nb, fade)
    unfaded = np.where(active, f == 1.0, True).all(1)            # every band that runs has f_b == 1
    integer = np.isfinite(s) & (s == np.round(s))
    assert (unfaded[integer]).all() and integer.sum() > n // 8
    if not fade:
        assert unfaded.all()
    checked = 0
    sb = bits(s)
    for word in np.unique(sb):
        idx = np.flatnonzero((sb == word) & unfaded)
        if idx.size == 0:
            continue
        sval = s[idx[0]]
        for k in kinds:
            want = uniform_call(nm, k, tile, pts[idx], nrs if one else nrs[idx], one, sval, first, nb, w)
            assert (bits(got[k][idx]) == bits(want)).all(), (k, float(sval))
        checked += idx.size
    assert checked == unfaded.sum() and checked >= (n if not fade else n // 8)


# ---- 3. list independence --------------------------------------------------------------------------------------------------
def ordered_footprints(order, first, nb, count, seed):
    s = F.footprints(first, nb, count, seed)
    if order == "ascending":
        return np.sort(s)                                        # NaN last
    if order == "all_equal":
        return np.full(count, -first - 2.5, np.float32)
    if order == "one_chunk_without_a_band":
        s[3 * 4096:4 * 4096] = np.float32(np.inf)
        s[4 * 4096:4 * 4096 + 7] = np.float32(np.nan)
    return s


@pytest.mark.parametrize("order", ["random", "ascending", "all_equal", "one_chunk_without_a_band"])
@pytest.mark.parametrize("kind", KINDS)
def test_long_lists_have_the_bits_of_their_slices(nm, tiles, kind, order):
    objs, _ = tiles
    first, nb, fade = 0, 5, 1
    w = F.weights(nb, first)
    pts = F.points(first, nb, N_LONG, 31)
    s = ordered_footprints(order, first, nb, N_LONG, 32)
    nrs = F.normals(N_LONG, 33)
    masks = [None] + ([(np.random.default_rng(34).random(N_LONG) < 0.4).astype(np.uint8)] if kind == "tex" else [])
    step = SORT_MIN // 2 + 5                                     # shorter slices, not chunk-aligned
    assert step < SORT_MIN <= N_LONG - 4096
    for active in masks:
        long_ = run(nm, kind, objs["t128"], pts, nrs, s, first, nb, w, fade, active=active, fill=-7.0)
        short = np.concatenate([run(nm, kind, objs["t128"], pts[a:a + step], nrs[a:a + step], s[a:a + step], first, nb, w,
                                    fade, active=None if active is None else active[a:a + step], fill=-7.0)
                                for a in range(0, N_LONG, step)])
        assert (bits(long_) == bits(short)).all(), int((bits(long_) != bits(short)).sum())
        if active is not None:
            assert (long_[active == 0] == -7.0).all() and (long_[active != 0] != -7.0).all()
        else:
            assert (long_ != -7.0).all()


@pytest.mark.parametrize("kind", ["value", "grad"])
def test_long_list_hard_cut_on_a_tile_that_is_no_power_of_two(nm, tiles, kind):
    objs, _ = tiles
    first, nb, fade = -2, 8, 0
    w = F.weights(nb, first)
    pts = F.points(first, nb, N_LONG, 35)
    s = F.footprints(first, nb, N_LONG, 36)
    long_ = run(nm, kind, objs["t6"], pts, None, s, first, nb, w, fade)
    step = SORT_MIN - 1
    short = np.concatenate([run(nm, kind, objs["t6"], pts[a:a + step], None, s[a:a + step], first, nb, w, fade)
                            for a in range(0, N_LONG, step)])
    assert (bits(long_) == bits(short)).all()


# ---- 4. output frame -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [N_SHORT, SORT_MIN + 1000], ids=["short", "long"])
@pytest.mark.parametrize("kind", KINDS)
def test_exactly_the_output_is_written_from_float_aligned_pointers(nm, tiles, kind, n):
    objs, _ = tiles
    first, nb, fade = 0, 5, 1
    w = F.weights(nb, first)
    pts = F.points(first, nb, n, 41)
    s = F.footprints(first, nb, n, 42)
    nrs = F.normals(n, 43)
    ch = CHANNELS[kind]
    x, sf, nf = _frame.Frame.holding(pts, 1), _frame.Frame.holding(s, 3), _frame.Frame.holding(nrs, 1)
    assert x.ptr.value % 16 and sf.ptr.value % 16
    want = run(nm, kind, objs["t128"], pts, nrs, s, first, nb, w, fade)
    out = _frame.Frame(n * ch, 0 if ch == 4 else 1)              # float4 records need 16 bytes; floats only their own 4
    rc = abi(nm, kind, objs["t128"]._handle(3), x.ptr, nf.ptr, 0, sf.ptr, None, n, first, nb, w, fade, out.ptr)
    assert rc == 0, nm._lib.wn_last_error()
    got = out.result(what=kind).reshape(n, ch)
    assert (bits(got) == bits(want)).all()
    for f in (x, sf, nf):                                         # the inputs and their guards are untouched
        f.result(what="input")
    if ch == 4:
        bad = _frame.Frame(n * ch, 1)
        rc = abi(nm, kind, objs["t128"]._handle(3), x.ptr, nf.ptr, 0, sf.ptr, None, n, first, nb, w, fade, bad.ptr)
        assert rc == nm._capi.WN_ERR_INVALID
        bad.result(written=np.zeros(n * ch, bool), what="refused call")
    if kind == "tex":
        active = (np.random.default_rng(44).random(n) < 0.4).astype(np.uint8)
        import torch
        act = torch.from_numpy(active).cuda()
        masked = _frame.Frame(n, 1)
        rc = abi(nm, kind, objs["t128"]._handle(3), x.ptr, None, 0, sf.ptr, act, n, first, nb, w, fade, masked.ptr)
        assert rc == 0, nm._lib.wn_last_error()
        res = masked.result(written=active != 0, what="masked texture")
        assert (bits(res[active != 0]) == bits(want[active != 0, 0])).all()


# ---- 5. argument checks ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_argument_checks(wn, nm, tiles, kind):
    import torch
    objs, _ = tiles
    INVALID = nm._capi.WN_ERR_INVALID
    first, nb, fade, n = 0, 5, 1, 300
    w = F.weights(nb, first)
    pts, s, nrs = F.points(first, nb, n, 51), F.footprints(first, nb, n, 52), F.normals(n, 53)
    # an empty tile: 0 in every channel (the texture: 0.5), short and long lists
    for count in (n, SORT_MIN + 5):
        big = np.resize(pts, (count, 3)), np.resize(nrs, (count, 3)), np.resize(s, count)
        got = run(nm, kind, objs["empty"], big[0], big[1], big[2], first, nb, w, fade)
        assert (got == (0.5 if kind == "tex" else 0.0)).all()
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    x, nr, sd = d(pts), d(nrs), d(s)
    out = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    h = objs["t128"]._handle(3)
    call = lambda **kw: abi(nm, kind, kw.get("h", h), kw.get("x", x), kw.get("nr", nr), 0, kw.get("s", sd), None,  # noqa: E731
                            kw.get("n", n), first, kw.get("nb", nb), kw.get("w", w), fade, kw.get("out", out))
    assert call() == 0
    assert call(n=0, x=None, s=None, out=None, nr=None) == 0      # n == 0: nothing is read
    assert call(h=None) == INVALID
    assert call(x=None) == INVALID and call(s=None) == INVALID and call(out=None) == INVALID
    if kind.startswith("proj"):
        assert call(nr=None) == INVALID
    assert call(nb=9) == INVALID and call(nb=-1) == INVALID
    assert call(nb=9, n=0) == INVALID                             # the bands are checked before the list's length
    assert call(w=None) == INVALID and call(w=None, nb=0) == 0
    t2 = wn.WaveletNoise(16, 3)
    t2.generateNoiseTile2D()
    assert call(h=t2._handle(2)) == INVALID and b"3-D tile" in nm._lib.wn_last_error()


def test_a_tile_is_used_on_its_own_device(nm, tiles):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs a second GPU to be the wrong device")
    objs, _ = tiles
    h = objs["t128"]._handle(3)
    with torch.cuda.device(1):
        x = torch.zeros((4, 3), dtype=torch.float32, device="cuda")
        s = torch.zeros(4, dtype=torch.float32, device="cuda")
        out = torch.empty((4, 4), dtype=torch.float32, device="cuda")
        for kind in KINDS:
            assert abi(nm, kind, h, x, x, 0, s, None, 4, 0, 2, [1.0, 0.5], 0, out) == nm._capi.WN_ERR_INVALID
            assert b"device" in nm._lib.wn_last_error()


# ---- 6. host and Python classes ------------------------------------------------------------------------------------------------
def test_host_classes_match_the_c_abi(tmp_path):
    exe = tmp_path / "footprint_api_check"
    src = os.path.join(HERE, "host_src", "footprint_api_check.cpp")
    build = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                            "-I" + os.path.join(PKG, "host"), src, "-o", str(exe), "-L" + PKG, "-lwnoise_host",
                            "-lwnoise_hip", "-Wl,-rpath," + PKG], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run_ = subprocess.run(["timeout", "-k", "10", "300", str(exe)], capture_output=True, text=True)
    assert run_.returncode == 0, run_.stdout + run_.stderr
    assert "mismatches 0" in run_.stdout, run_.stdout


@pytest.mark.parametrize("fade", [False, True])
def test_python_classes_match_the_c_abi(wn, nm, tiles, fade):
    import torch
    objs, _ = tiles
    first, nb, n = 0, 5, 1500
    w = F.weights(nb, first)
    pts, s, nrs = F.points(first, nb, n, 61), F.footprints(first, nb, n, 62), F.normals(n, 63)
    t = objs["t128"]
    td, sd = torch.from_numpy(pts).cuda(), torch.from_numpy(s).cuda()
    for normal, kinds in ((None, ("value", "grad")), (nrs, ("proj", "proj_grad")), (nrs[:1], ("proj", "proj_grad"))):
        one = int(normal is not None and len(normal) == 1)
        v = t.WMultibandNoise(td, sd, first, nb, w, normal=normal, fade=fade).cpu().numpy()
        g = t.WMultibandNoiseGradient(pts, s, first, nb, w, normal=normal, fade=fade).cpu().numpy()
        nr_all = nrs if normal is None or not one else normal
        assert (bits(v) == bits(run(nm, kinds[0], t, pts, nr_all, s, first, nb, w, int(fade), one=one)[:, 0])).all()
        assert (bits(g) == bits(run(nm, kinds[1], t, pts, nr_all, s, first, nb, w, int(fade), one=one))).all()
    # a scalar s keeps the uniform path and its bits
    v = t.WMultibandNoise(td, -2.5, first, nb, w).cpu().numpy()
    assert (bits(v) == bits(uniform_call(nm, "value", t, pts, None, 0, -2.5, first, nb, w)[:, 0])).all()
    with pytest.raises(ValueError):
        t.WMultibandNoise(td, sd[:-1], first, nb, w)
    # the texture class (its own tile: 128, seed 12345, generated on the device)
    tex = wn.wavelet_multiband_texture(SCALE, first, nb, w, fade=fade)
    assert tex.default_footprint == -np.inf
    active = (np.random.default_rng(64).random(n) < 0.4).astype(np.uint8)
    want = run(nm, "tex", tex.noise_3d, pts, None, s, first, nb, w, int(fade))[:, 0]
    assert (bits(tex.grey(pts, s).cpu().numpy()) == bits(want)).all()
    got = tex.grey(td, sd, active=active, out=torch.full((n,), -7.0, device="cuda")).cpu().numpy()
    assert (bits(got[active != 0]) == bits(want[active != 0])).all() and (got[active == 0] == -7.0).all()
    allb = run(nm, "tex", tex.noise_3d, pts, None, np.full(n, -np.inf, np.float32), first, nb, w, int(fade))[:, 0]
    assert (bits(tex.value(0, 0, pts).cpu().numpy()[:, 0]) == bits(allb)).all()
    assert tex.value(0, 0, pts[0]) == (float(allb[0]),) * 3
