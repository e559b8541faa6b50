"""GPU parity: the HIP path (through the C ABI) against the oracle and the committed goldens.

Bars (BASELINE.json north_star / SURVEY 8(c)):
  * Perlin: integer hash AND fp64 value bit-exact.
  * wavelet point lists, textures, WN_GRID_EXACT grids, tile generation: bit-exact.
  * default (separable brick) dense wavelet grids: |gpu - oracle| <= 1e-5 absolute.
"""
import hashlib
import importlib
import json
import os

import numpy as np
import pytest

from conftest import GOLD, bits, raw

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL = 1e-5  # north_star: "within 1e-5 abs of the reference float WNoise"


@pytest.fixture(scope="module")
def wn():
    assert torch.cuda.is_available(), "GPU tests need a GPU (the product has no CPU path)"
    return importlib.import_module("wavelet-noise-in-ray-tracing_amd")


@pytest.fixture(scope="module")
def noise3(wn):
    n = wn.WaveletNoise(128, 12345)
    n.generateNoiseTile3D()
    return n


@pytest.fixture(scope="module")
def noise2(wn):
    n = wn.WaveletNoise(128, 12345)
    n.generateNoiseTile2D()
    return n


def host(t):
    return t.detach().cpu().numpy()


# ---- tile generation (device filter passes) -------------------------------------------------------
def test_tile_generation_bit_exact(wn, noise2, noise3, tile2d_128, tile3d_128, artefacts):
    assert (bits(noise2.getNoiseCoefficients()) == bits(tile2d_128)).all()
    c3 = noise3.getNoiseCoefficients()
    assert (bits(c3) == bits(tile3d_128)).all()
    assert hashlib.sha256(c3.tobytes()).hexdigest() == artefacts["tile3d_128_12345"]["sha256"]


def test_tile_generation_small_odd_and_repeated(wn, gold, ora, ref_checks):
    for n, seed, dims, key in ((8, 7, 3, "tile3d_8_7"), (16, 12345, 3, "tile3d_16_12345"),
                               (16, 99, 2, "tile2d_16_99"), (7, 3, 2, "tile2d_7odd_3"),
                               (5, 11, 3, "tile3d_5odd_11")):
        w = wn.WaveletNoise(n, seed)
        (w.generateNoiseTile2D if dims == 2 else w.generateNoiseTile3D)()
        assert (bits(w.getNoiseCoefficients()) == bits(gold[key])).all(), key
        assert w.getTileSize() == n + (n % 2)
    # the rng is a member: a second generate continues the stream (WaveletNoise.h:47); the reference live when it was
    # built, its stored answer otherwise
    want = ref_checks["tile3d_16_5_after_2d"]
    R = ora.ref()
    if R is not None:
        h = R.ref_wn_new(16, 5)
        R.ref_wn_generate2d(h)
        R.ref_wn_generate3d(h)
        want = np.zeros(R.ref_wn_coeff_count(h), np.float32)
        R.ref_wn_coeffs(h, want)
        R.ref_wn_delete(h)
    w = wn.WaveletNoise(16, 5)
    w.generateNoiseTile2D()
    w.generateNoiseTile3D()
    assert (bits(w.getNoiseCoefficients()) == bits(want)).all()


# ---- point lists --------------------------------------------------------------------------------------
def test_points_bit_exact_vs_reference_vectors(wn, gold, noise2, noise3):
    pts = gold["probe_pts"]
    assert (bits(host(noise3.evaluate3D(pts))) == bits(gold["probe_e3d"])).all()
    assert (bits(host(noise2.evaluate2D(pts[:, :2]))) == bits(gold["probe_e2d"])).all()
    got = noise3.evaluate3DProjected(gold["probe_proj_pts"], gold["probe_proj_normals"])
    assert (bits(host(got)) == bits(gold["probe_e3dp"])).all()


def test_points_small_tiles_wrap(wn, gold):
    sp = gold["small_pts"]
    for key, dims in (("tile3d_8_7", 3), ("tile3d_16_12345", 3)):
        w = wn.WaveletNoise.from_coefficients(gold[key], dims)
        assert (bits(host(w.evaluate3D(sp))) == bits(gold[key + "_e3d"])).all()
    w = wn.WaveletNoise.from_coefficients(gold["tile2d_16_99"], 2)
    assert (bits(host(w.evaluate2D(sp[:, :2]))) == bits(gold["tile2d_16_99_e2d"])).all()
    # a non power-of-two tile (n = 6) exercises the generic modulo
    w6 = wn.WaveletNoise.from_coefficients(gold["tile3d_5odd_11"], 3)
    import oracle
    assert (bits(host(w6.evaluate3D(sp))) == bits(oracle.evaluate3d(gold["tile3d_5odd_11"], sp))).all()


def test_scalar_api_and_empty_tile(wn, noise3, ora, tile3d_128):
    p = [1.25, -3.75, 100.1]
    assert noise3.evaluate3D(p) == pytest.approx(0.355737954, abs=2e-7)
    assert np.float32(noise3.evaluate3D(p)) == ora.evaluate3d(tile3d_128, [p])[0]
    empty = wn.WaveletNoise(128, 1)  # never generated
    assert empty.evaluate3D(p) == 0.0 and empty.evaluate2D(p[:2]) == 0.0
    assert empty.evaluate3DProjected(p, [0, 0, 1]) == 0.0
    assert empty.getNoiseCoefficients().size == 0
    # zero points is a no-op
    assert noise3.evaluate3D(np.zeros((0, 3), np.float32)).numel() == 0


def test_large_random_point_list_vs_oracle(wn, noise3, ora, ref_checks, tile3d_128):
    pts = ref_checks["rng3_pts"]  # default_rng(3).uniform(-320, 320, (20000, 3)) as float32
    got = host(noise3.evaluate3D(pts))
    want = ref_checks["rng3_e3d"]  # the reference's answer, stored; live below when it was built
    R = ora.ref()
    if R is not None:
        h = R.ref_wn_new(128, 12345)
        R.ref_wn_generate3d(h)
        want = np.zeros(len(pts), np.float32)
        R.ref_wn_eval3d(h, np.ascontiguousarray(pts), len(pts), want)
        R.ref_wn_delete(h)
    assert (bits(got) == bits(want)).all()
    assert (bits(got[:4000]) == bits(ora.evaluate3d(tile3d_128, pts[:4000]))).all()


def test_long_point_lists_take_plane_ordered_chunks_bit_exact(wn, noise3, ora, tile3d_128):
    """evaluate3D / WMultibandNoise lists of >= 64 K points go through plane_sorted_points_kernel (chunks of 4,096 points
    in z-plane order, or in stream order when already coherent): same floats as the oracle and as the plain kernels
    (the same points in pieces below the threshold)."""
    rng = np.random.default_rng(11)
    n = 4096 * 20 + 777
    scattered = rng.uniform(-40, 40, (n, 3)).astype(np.float32)
    planar = scattered.copy()
    planar[:, 1] = -0.5
    coherent = np.stack([np.linspace(-40, 40, n), np.full(n, 0.25), np.repeat(rng.uniform(-40, 40, n // 256 + 1), 256)[:n]], 1).astype(np.float32)
    w = [1.0, 0.5, 2.0, 1.0, 1.0]
    for pts in (scattered, planar, coherent):
        whole = host(noise3.evaluate3D(pts))
        pieces = np.concatenate([host(noise3.evaluate3D(pts[i:i + 30000])) for i in range(0, n, 30000)])
        assert (bits(whole) == bits(pieces)).all()
        assert (bits(whole[:3000]) == bits(ora.evaluate3d(tile3d_128, pts[:3000]))).all()
        small = (pts * np.float32(0.1)).astype(np.float32)  # band scales up to 32: keep the coordinates moderate
        whole = host(noise3.WMultibandNoise(small, -16.0, 0, 5, w))
        pieces = np.concatenate([host(noise3.WMultibandNoise(small[i:i + 30000], -16.0, 0, 5, w)) for i in range(0, n, 30000)])
        assert (bits(whole) == bits(pieces)).all()
        assert (bits(whole[:2000]) == bits(ora.multiband3d(tile3d_128, small[:2000], -16.0, 0, 5, w, 0.18402))).all()


# ---- dense grids: the committed raws ---------------------------------------------------------------------
@pytest.mark.parametrize("octave", (3, 4, 5))
def test_committed_raw_grids(wn, noise2, noise3, octave):
    sha = json.load(open(os.path.join(GOLD, "artefacts.json")))["raw"]
    per = wn.PerlinNoise(12345)

    def digest(t):
        return hashlib.sha256(host(t).astype("<f4").tobytes()).hexdigest()

    # bit-exact paths: byte-identical files
    assert digest(wn.generate2DOctaveBandNoise(256, octave, None, noise2)) == sha[f"wavelet_noise_2D_octave_{octave}.raw"]
    assert digest(wn.generate3DProjectedOctaveBandNoise(256, octave, None, noise3)) == sha[f"wavelet_noise_3Dprojected_octave_{octave}.raw"]
    assert digest(wn.generatePerlinNoise2D(256, octave, None, per)) == sha[f"perlin_noise_2D_octave_{octave}.raw"]
    assert digest(wn.generatePerlinNoise3DSliced(256, octave, None, per)) == sha[f"perlin_noise_3Dsliced_octave_{octave}.raw"]
    exact = wn.generate3DSlicedOctaveBandNoise(256, octave, None, noise3, flags=wn.WN_GRID_EXACT)
    assert digest(exact) == sha[f"wavelet_noise_3Dsliced_octave_{octave}.raw"]
    # opt-in fast path (separable bricks when the lattice step allows): within tolerance
    fast = host(wn.generate3DSlicedOctaveBandNoise(256, octave, None, noise3, flags=wn.WN_GRID_DEFAULT)).ravel()
    want = raw(f"wavelet_noise_3Dsliced_octave_{octave}.raw")
    assert np.abs(fast - want).max() <= TOL


def test_raw_writer_round_trip(wn, noise2, tmp_path):
    f = tmp_path / "w2d.raw"
    wn.generate2DOctaveBandNoise(256, 4, str(f), noise2)
    assert hashlib.sha256(f.read_bytes()).hexdigest() == \
        json.load(open(os.path.join(GOLD, "artefacts.json")))["raw"]["wavelet_noise_2D_octave_4.raw"]


# ---- dense volumes (config 2 / 5 mapping) -------------------------------------------------------------------
def test_volume_goldens(wn, gold, artefacts, noise3):
    for name, den, nx, ny, z0, z1, octave in artefacts["volumes"]:
        want = gold[name]
        exact = host(wn.wavelet_volume(noise3, den, nx, ny, z0, z1, octave, exact=True))
        assert (bits(exact) == bits(want)).all(), name
        fast = host(wn.wavelet_volume(noise3, den, nx, ny, z0, z1, octave))
        assert np.abs(fast - want).max() <= TOL, name


@pytest.mark.parametrize("den,nx,ny,z0,z1,octave", [
    (512, 512, 24, 0, 8, 4),        # config-2 step .25, full-width rows (the plane pipeline takes it)
    (512, 512, 9, 505, 512, 4),     # last planes, ragged y (plane pipeline)
    (512, 300, 17, 3, 6, 4),        # nx not a multiple of 256; thin slab (BZ=4)
    (512, 131, 5, 7, 8, 4),         # nx not a multiple of 4 -> scalar stores; one plane
    (2048, 2048, 8, 1000, 1009, 4), # config-5 step 1/16, 9 planes (plane pipeline)
    (1024, 515, 20, 0, 2, 4),       # step 1/8
    (256, 256, 16, 0, 16, 3),       # step .25 at octave 3 (rows of 256: the strip kernel takes it)
    (512, 512, 8, 4096, 4104, 4),   # z beyond one tile period (weak-scaling shards) (plane pipeline)
    (768, 768, 8, 0, 8, 4),         # non power-of-two divisor, step 1/6
    (1000, 1000, 8, 0, 8, 4),       # inexact float division in the lattice coordinate (plane pipeline, partial x-brick)
    (768, 768, 9, 3, 40, 4),        # 256-wide bricks, 16 planes deep (37 planes: two full bricks and a ragged one in z)
    (1280, 640, 5, 0, 21, 4),       # step .1: 256-wide bricks with a half-empty last column, 16-plane bricks
    (512, 998, 9, 0, 20, 4),        # 512-wide bricks, 8 planes deep, ragged in x, y and z (nx % 4: not the pipeline)
    (712, 768, 5, 3, 12, 4),        # step .1798, just below the strip kernel's regime; inexact division
    (512, 928, 7, 1, 10, 4),        # the pipeline would pad its last brick by more than 10 %
])
def test_brick_path_vs_oracle(wn, ora, noise3, tile3d_128, den, nx, ny, z0, z1, octave):
    """The default path against the oracle, the exact kernel bit-exact.  Named after the brick kernel, but the plane
    pipeline and the strip kernel take the lattices marked so (the first fitting kernel serves: tests/test_gpu_dispatch.py
    pins which kernel serves each of the last three)."""
    want = ora.grid_wavelet3d_volume(tile3d_128, den, nx, ny, z0, z1, octave)
    fast = host(wn.wavelet_volume(noise3, den, nx, ny, z0, z1, octave))
    assert fast.shape == want.shape
    err = np.abs(fast - want).max()
    assert err <= TOL, err
    exact = host(wn.wavelet_volume(noise3, den, nx, ny, z0, z1, octave, exact=True))
    assert (bits(exact) == bits(want)).all()


@pytest.mark.parametrize("den,nx,ny,z0,z1,octave", [
    (512, 256, 4, 0, 300, 4),       # three z chunks of 100 planes, one column block
    (512, 512, 3, 17, 18, 4),       # a single plane (the plane pipeline takes it)
    (400, 512, 6, 0, 40, 4),        # step .32, close to the 1/3 limit of the window scheme
    (700, 768, 5, 0, 20, 4),        # step .183, just inside the regime; inexact division; 3 column blocks
    (512, 1024, 3, 100, 140, 4),    # x beyond one lattice period (plane pipeline)
    (512, 512, 2, 8190, 8200, 4),   # large z offset (plane pipeline)
    (448, 512, 6, 0, 40, 4),        # step 2/7: too coarse for the plane pipeline (K = 6), strip kernel
    (385, 256, 5, 9, 30, 4),        # step .3325, the largest step inside the regime
    (711, 768, 7, 2, 40, 4),        # step .18003, the smallest
    (512, 768, 5, 4000, 4033, 4),   # large z offset, 3 column blocks
])
def test_strip_path_vs_oracle(wn, ora, noise3, tile3d_128, den, nx, ny, z0, z1, octave):
    """Lattices in the strip-march kernel's regime (rows of k*256 samples, 0.18 <= step <= 1/3):
    chunk seams, single planes, the regime's edges.  The plane pipeline comes first and takes the lattices marked so."""
    want = ora.grid_wavelet3d_volume(tile3d_128, den, nx, ny, z0, z1, octave)
    fast = host(wn.wavelet_volume(noise3, den, nx, ny, z0, z1, octave))
    assert fast.shape == want.shape
    err = np.abs(fast - want).max()
    assert err <= TOL, err


@pytest.mark.parametrize("den,nx,ny,z0,z1", [
    (512, 512, 300, 0, 512),        # (the plane pipeline takes it)
    (512, 768, 170, 3, 260),        # ragged last chunk, 3 column blocks, odd row count
    (512, 512, 2048, 1, 255),       # (the plane pipeline takes it)
    (400, 256, 2052, 0, 301),       # step .32: 513 groups, a range of 301 planes in items of 76, 75, 75, 75
    (448, 512, 300, 0, 128),        # step 2/7 (not the pipeline's): 150 groups of 2-segment rows, 4 ranges of 32 planes
    (416, 512, 2048, 1, 255),       # step .3077: 1024 groups, one range of 254 planes walked in 3 items of 85
])
def test_strip_path_many_items_vs_exact_kernel(wn, ora, tile3d_128, noise3, den, nx, ny, z0, z1):
    """More items than resident compute waves.  Checker for the whole lattice: the exact kernel (bit-identical to the
    oracle, test_brick_path_vs_oracle); the first and last plane of every case also against the oracle ITSELF (the exact
    kernel is a HIP kernel too: round-2 VERDICT), rows y < 64 of them (the oracle's 27-tap loop on 1-2 M samples)."""
    fast = wn.wavelet_volume(noise3, den, nx, ny, z0, z1, 4)
    exact = wn.wavelet_volume(noise3, den, nx, ny, z0, z1, 4, exact=True)
    err = float((fast - exact).abs().max())
    assert err <= TOL, err
    rows = min(ny, 64)
    for z in (z0, z1 - 1):
        want = ora.grid_wavelet3d_volume(tile3d_128, den, nx, rows, z, z + 1, 4)[0]
        assert np.abs(host(fast[z - z0, :rows]) - want).max() <= TOL, z
        assert (bits(host(exact[z - z0, :rows])) == bits(want)).all(), z


def test_brick_path_small_tiles_and_wrap(wn, ora, gold):
    """Periodic wrap inside the coefficient box: tiles far smaller than a brick's footprint."""
    for key in ("tile3d_8_7", "tile3d_16_12345", "tile3d_5odd_11"):
        coef = gold[key]
        w = wn.WaveletNoise.from_coefficients(coef, 3)
        want = ora.grid_wavelet3d_volume(coef, 512, 512, 10, 0, 5, 4)
        fast = host(wn.wavelet_volume(w, 512, 512, 10, 0, 5, 4))
        assert np.abs(fast - want).max() <= TOL, key


def test_empty_grids_and_empty_tile(wn, noise3):
    assert wn.wavelet_volume(noise3, 64, 0, 8, 0, 4, 4).numel() == 0
    assert wn.wavelet_volume(noise3, 64, 8, 8, 4, 4, 4).numel() == 0
    empty = wn.WaveletNoise(128, 1)
    v = host(wn.wavelet_volume(empty, 512, 512, 8, 0, 4, 4))
    assert (v == 0).all()  # empty tile -> 0.0f * inv_stddev


# ---- multiband / turb (config 3) -------------------------------------------------------------------------------
def test_multiband_grid_and_points(wn, ora, noise3, tile3d_128):
    w = [1.0, 1.0, 1.0, 1.0, 1.0]
    want = ora.grid_multiband3d_volume(tile3d_128, 512, 512, 8, 16, 20, -16.0, 0, 5, w, 0.18402)
    fast = host(wn.multiband_volume(noise3, 512, 512, 8, 16, 20, -16.0, 0, 5, w))
    assert np.abs(fast - want).max() <= TOL
    exact = host(wn.multiband_volume(noise3, 512, 512, 8, 16, 20, -16.0, 0, 5, w, exact=True))
    assert (bits(exact) == bits(want)).all()
    # the top band of config 3 is config 2's band
    w2 = [0.5, 2.0, 1.0]
    for s, first, nb in ((-16.0, 1, 3), (-2.0, 0, 3), (0.0, 0, 3), (-16.0, -3, 3)):
        want = ora.grid_multiband3d_volume(tile3d_128, 256, 256, 8, 0, 3, s, first, nb, w2, 0.21)
        got = host(wn.multiband_volume(noise3, 256, 256, 8, 0, 3, s, first, nb, w2, variance=0.21))
        assert np.abs(got - want).max() <= TOL, (s, first, nb)
    rng = np.random.default_rng(5)
    pts = rng.uniform(-4, 4, (3000, 3)).astype(np.float32)
    got = host(noise3.WMultibandNoise(pts, -16.0, 0, 5, w))
    assert (bits(got) == bits(ora.multiband3d(tile3d_128, pts, -16.0, 0, 5, w, 0.18402))).all()


def test_perlin_points_grids_turb_fractal(wn, ora, gold):
    pts = gold["perlin_pts"]
    for seed in (12345, 5489):
        p = wn.perlin(seed)
        assert (p.p == gold["perm_tables"][list(gold["perm_seeds"]).index(seed)]).all()  # integer hash table
        assert (bits(host(p.noise(pts))) == bits(gold[f"perlin_noise_{seed}"])).all()
        f32 = pts.astype(np.float32)
        assert (bits(host(p.noise(f32))) == bits(gold[f"perlin_noise_vec3_{seed}"])).all()
        assert (bits(host(p.fractal_noise(f32))) == bits(gold[f"perlin_fractal_{seed}"])).all()
    p = wn.perlin(12345)
    perm = ora.perlin_perm(12345)
    assert p.noise(1.25, -3.75, 100.1) == -0.20131776773070792
    assert p.noise(0.5, 0.5) == ora.perlin_noise(perm, [[0.5, 0.5, 0.0]])[0]
    f32 = pts[:3000].astype(np.float32)
    assert (bits(host(p.turb(f32, 7))) == bits(ora.perlin_turb(perm, f32, 7))).all()
    got = host(wn.turb_volume(p, 512, 512, 6, 9, 12, 7))
    assert (bits(got) == bits(ora.grid_turb_volume(perm, 512, 512, 6, 9, 12, 7))).all()
    got = host(wn.perlin_volume(p, 100, 100, 7, 2, 5, 4))
    assert (bits(got) == bits(ora.grid_perlin_volume(perm, 100, 100, 7, 2, 5, 4))).all()


# ---- texture adaptor -------------------------------------------------------------------------------------------------
def test_textures_bit_exact(wn, gold, artefacts):
    tp = gold["tex_pts"]
    cache = {}
    for kind, scale, octave in artefacts["texture_cases"]:
        key = f"tex_{kind}_s{scale}_o{octave}"
        if kind == "perlin":
            tex = wn.noise_texture(scale, octave)
        else:
            k = (kind, scale, octave)
            tex = cache.get(k) or wn.wavelet_texture(scale, octave, kind == "wavelet3d")
            cache[k] = tex
        assert (bits(host(tex.grey(tp))) == bits(gold[key])).all(), key
    # scalar value(u,v,p) returns an equal-channel colour (texture.h:106)
    tex = wn.wavelet_texture(1.0, 4, True)
    c = tex.value(0.0, 0.0, tp[0])
    assert c[0] == c[1] == c[2] == float(gold["tex_wavelet3d_s1.0_o4"][0])


@pytest.mark.parametrize("frac", (0.0, 0.07, 0.59, 1.0))
def test_texture_active_mask_compaction(wn, gold, frac):
    """Ballot compaction: active hits get the texture value, the rest are left untouched."""
    rng = np.random.default_rng(int(frac * 100))
    n = 70001  # not a multiple of 64 or of the per-wave chunk
    pts = np.stack([rng.uniform(-10, 10, n), np.full(n, -0.5), rng.uniform(-10, 10, n)], 1).astype(np.float32)
    active = (rng.random(n) < frac).astype(np.uint8)
    for tex in (wn.wavelet_texture(1.0, 4, True), wn.noise_texture(1.0, 4)):
        full = host(tex.grey(pts))
        out = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
        masked = host(tex.grey(pts, active=active, out=out))
        assert (masked[active == 0] == -7.0).all()
        assert (bits(masked[active == 1]) == bits(full[active == 1])).all()


def test_texture_plane_sorted_chunks_match_stream_order(wn):
    """Lists of >= 64 K points take chunks in z-plane order when the stream is incoherent (wn_wavelet_points.hip,
    plane_sorted_points_kernel) and in stream order when it is coherent; both must give the floats of the
    unsorted kernel, which the goldens pin (here: the same points in pieces below the threshold)."""
    rng = np.random.default_rng(77)
    n = 4096 * 40 + 1234
    tex = wn.wavelet_texture(1.0, 4, True)
    scattered = np.stack([rng.uniform(-10, 10, n), np.full(n, -0.5), rng.uniform(-10, 10, n)], 1).astype(np.float32)
    sphere = rng.normal(size=(n, 3))
    sphere = (2.0 * sphere / np.linalg.norm(sphere, axis=1, keepdims=True) + [0, 2, 0]).astype(np.float32)
    coherent = np.stack([np.linspace(-10, 10, n), np.full(n, -0.5), np.repeat(rng.uniform(-10, 10, n // 512 + 1), 512)[:n]], 1).astype(np.float32)
    mixed = np.concatenate([coherent[: 4096 * 20], scattered[4096 * 20:]])  # the decision is per chunk
    for pts in (scattered, sphere, coherent, mixed):
        whole = host(tex.grey(pts))
        pieces = np.concatenate([host(tex.grey(pts[i:i + 30000])) for i in range(0, n, 30000)])
        assert (bits(whole) == bits(pieces)).all()


def test_row_slab_kernel_long_lists_bit_exact(wn, noise3, ora, tile3d_128):
    """Unmasked lists of >= 16.8 M points on the padded 128^3 tile: plane_sorted_points_kernel evaluates the chunks that are
    coherent already and leaves the others to row_slab_points_kernel (wn_wavelet_points.hip): persistent workgroups that
    keep the two y rows most of a chunk's points share in LDS (and a third for 55 planes) and take those points' row
    triples from there.  Same floats as the plain kernels (the same points in pieces below every threshold) and as the
    oracle, for streams that (a) lie mostly on one axis-aligned plane, (b) move from one plane to another and then scatter
    (the slab is replaced, then unused), (c) are coherent already, (d) carry an `active` mask (the plane-ordered kernel
    alone)."""
    rng = np.random.default_rng(5)
    n = 16 * 256 * 4096 + 3333
    tex = wn.wavelet_texture(1.0, 4, True)
    quad = np.stack([rng.uniform(-10, 10, n), np.full(n, -0.5), rng.uniform(-10, 10, n)], 1)
    sph = rng.normal(size=(n, 3))
    sph = 0.5 * sph / np.linalg.norm(sph, axis=1, keepdims=True) + [1.0, 0.0, -1.75]
    scene = np.where((rng.uniform(size=n) < 0.85)[:, None], quad, sph).astype(np.float32)  # configs[3]'s stand-in
    moving = quad.copy()
    moving[n // 3: 2 * n // 3, 1] = 1.3
    moving[2 * n // 3:, 1] = rng.uniform(-10, 10, n - 2 * n // 3)
    moving = moving.astype(np.float32)
    coherent = np.stack([np.linspace(-10, 10, n), np.full(n, -0.5), np.repeat(rng.uniform(-10, 10, n // 512 + 1), 512)[:n]], 1).astype(np.float32)
    step = 60000  # < 16 chunks: the plain kernels
    for pts in (scene, moving, coherent):
        whole = host(tex.grey(pts))
        pieces = np.concatenate([host(tex.grey(pts[i:i + step])) for i in range(0, n, step)])
        assert (bits(whole) == bits(pieces)).all()
        pick = rng.integers(0, n, 3000)
        assert (bits(whole[pick]) == bits(ora.wavelet_texture_value(tile3d_128, True, 1.0, 4, pts[pick]))).all()
    # masked: inactive points keep the caller's value
    active = (rng.uniform(size=n) < 0.6).astype(np.uint8)
    out = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
    got = host(tex.grey(scene, active, out=out))
    want = np.where(active != 0, host(tex.grey(scene)), np.float32(-7.0))
    assert (bits(got) == bits(want)).all()
    # WaveletNoise::evaluate3D lists take the same kernel (lattice coordinates: the plane y = 16.0)
    lat = (scene * np.float32(32.0)).astype(np.float32)
    whole = host(noise3.evaluate3D(lat))
    pieces = np.concatenate([host(noise3.evaluate3D(lat[i:i + step])) for i in range(0, n, step)])
    assert (bits(whole) == bits(pieces)).all()
    assert (bits(whole[:3000]) == bits(ora.evaluate3d(tile3d_128, lat[:3000]))).all()


@pytest.mark.parametrize("seed", (2024, 7, 31337))
def test_dispatcher_fuzz_default_kernels_vs_exact(wn, noise3, seed):
    """Random lattices through wn_eval3d_grid / wn_multiband3d_grid: whatever kernel the dispatcher picks (strip march,
    brick, 16-plane brick, direct gathers) must stay within 1e-5 of WN_GRID_EXACT, which is bit-identical to the
    reference (pinned by the tests above).  Shapes include rows that are / are not multiples of 256, odd sizes,
    non-power-of-two denominators, steps on both sides of every regime edge, and offsets into the lattice."""
    rng = np.random.default_rng(seed)
    worst = 0.0
    for case in range(40):
        nx = int(rng.choice([64, 100, 192, 256, 257, 320, 512, 768, 1024]))
        ny = int(rng.choice([1, 3, 8, 13, 32, 70]))
        nz = int(rng.choice([1, 2, 5, 16, 33, 140]))
        while nx * ny * nz > 6_000_000:
            nz = max(1, nz // 2)
        den = int(rng.choice([128, 200, 256, 384, 512, 640, 1024, 2048]))
        octave = int(rng.integers(0, 6))
        z0 = int(rng.choice([0, 1, 7, 100, 511]))
        fast = wn.wavelet_volume(noise3, den, nx, ny, z0, z0 + nz, octave)
        exact = wn.wavelet_volume(noise3, den, nx, ny, z0, z0 + nz, octave, exact=True)
        err = float((fast - exact).abs().max())
        assert err <= TOL, ("wavelet_volume", den, nx, ny, z0, nz, octave, err)
        worst = max(worst, err)
        if case % 2 == 0:
            nb = int(rng.integers(1, 6))
            first = int(rng.integers(-2, 3))
            w = [float(x) for x in rng.uniform(0.25, 2.0, nb)]
            fast = wn.multiband_volume(noise3, den, nx, ny, z0, z0 + nz, -16.0, first, nb, w)
            exact = wn.multiband_volume(noise3, den, nx, ny, z0, z0 + nz, -16.0, first, nb, w, exact=True)
            err = float((fast - exact).abs().max())
            assert err <= TOL, ("multiband_volume", den, nx, ny, z0, nz, first, nb, err)
            worst = max(worst, err)
    assert worst > 0.0  # the separable kernels did run (their sums are ordered differently)


def test_entry_points_capture_into_a_hip_graph(wn, noise3):
    """The batched entry points only enqueue (no allocation, synchronisation or host read in the call), so a caller can
    capture them into a hipGraph and replay it: dense grid, turb grid and a texture list in one graph."""
    N = 256
    p = wn.perlin(12345)
    tex = wn.wavelet_texture(1.0, 4, True)
    pts = torch.rand(100000, 3, device="cuda") * 8 - 4
    want = (wn.wavelet_volume(noise3, N, N, N, 0, 16, 4).clone(), wn.turb_volume(p, N, N, N, 0, 8, 7).clone(), tex.grey(pts).clone())
    outs = (torch.empty(N * N * 16, dtype=torch.float32, device="cuda"), torch.empty(N * N * 8, dtype=torch.float32, device="cuda"),
            torch.empty(100000, dtype=torch.float32, device="cuda"))
    torch.cuda.synchronize()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            wn.wavelet_volume(noise3, N, N, N, 0, 16, 4, out=outs[0])
            wn.turb_volume(p, N, N, N, 0, 8, 7, out=outs[1])
            tex.grey(pts, out=outs[2])
    for _ in range(2):
        for o in outs:
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(outs[0].view(16, N, N), want[0]) and torch.equal(outs[1].view(8, N, N), want[1]) and torch.equal(outs[2], want[2])


# ---- size-independent properties at BASELINE sizes ---------------------------------------------------------------------
def test_full_512_cubed_properties(wn, ora, noise3, tile3d_128):
    """Config 2 at full size: periodicity, slab consistency, statistics and spot checks."""
    N = 512
    vol = wn.wavelet_volume(noise3, N, N, N, 0, N, 4)  # 512 MiB on the device
    assert vol.shape == (N, N, N)
    # (1) z-slabs computed separately are bit-identical to the full call (shard-safety)
    part = wn.wavelet_volume(noise3, N, N, N, 200, 208, 4)
    assert torch.equal(part, vol[200:208])
    # (2) the lattice spans exactly one tile period: shifting by N samples reproduces the plane
    wrap = wn.wavelet_volume(noise3, N, N, N, N + 37, N + 38, 4)
    assert torch.equal(wrap[0], vol[37])
    # (3) statistics of one band at unit-ish variance (~N(0, 0.77^2), |v| < 4.5)
    assert abs(float(vol.mean())) < 5e-3
    assert 0.70 < float(vol.std()) < 0.85
    assert float(vol.abs().max()) < 4.5
    # (4) random spot checks against the oracle's scalar evaluate3D
    rng = np.random.default_rng(11)
    idx = rng.integers(0, N, (4000, 3))
    q = (idx.astype(np.float32) / np.float32(N)) * np.float32(4) * np.float32(16) * np.float32(2)
    want = ora.evaluate3d(tile3d_128, q[:, ::-1].copy()) * (np.float32(1) / np.sqrt(np.float32(0.18402)))
    got = host(vol[idx[:, 0], idx[:, 1], idx[:, 2]])
    assert np.abs(got - want).max() <= TOL
    # (5) the committed 3-D-sliced raw (octave 4) is the z = 2.0 plane: lattice index 8 at N = 512,
    #     every second sample in x and y
    plane = host(vol[8, ::2, ::2]).ravel()
    assert np.abs(plane - raw("wavelet_noise_3Dsliced_octave_4.raw")).max() <= TOL


def test_randomised_lattices_vs_oracle(wn, ora, noise3, tile3d_128, gold):
    """Seeded sweep over lattice shapes / steps / offsets / tiles: default path within 1e-5,
    WN_GRID_EXACT bit-identical, whichever kernel the dispatcher picks."""
    rng = np.random.default_rng(20251004)
    tiles = {128: (noise3, tile3d_128),
             16: (wn.WaveletNoise.from_coefficients(gold["tile3d_16_12345"], 3), gold["tile3d_16_12345"]),
             6: (wn.WaveletNoise.from_coefficients(gold["tile3d_5odd_11"], 3), gold["tile3d_5odd_11"])}
    for case in range(40):
        den = int(rng.choice([1, 3, 64, 100, 256, 512, 640, 1024, 4096]))
        nx = int(rng.choice([1, 2, 3, 5, 63, 64, 255, 256, 257, 300, 512, 515, 700]))
        ny = int(rng.integers(1, 20))
        nz = int(rng.integers(1, 12))
        z0 = int(rng.choice([0, 1, 7, 100, 511, 5000]))
        octave = int(rng.integers(0, 7))
        n = int(rng.choice([128, 128, 16, 6]))
        w, coef = tiles[n]
        want = ora.grid_wavelet3d_volume(coef, den, nx, ny, z0, z0 + nz, octave)
        tag = (case, den, nx, ny, z0, nz, octave, n)
        fast = host(wn.wavelet_volume(w, den, nx, ny, z0, z0 + nz, octave))
        assert fast.shape == want.shape, tag
        assert np.abs(fast - want).max() <= TOL, tag
        exact = host(wn.wavelet_volume(w, den, nx, ny, z0, z0 + nz, octave, exact=True))
        assert (bits(exact) == bits(want)).all(), tag


def test_randomised_strip_regime_vs_exact_kernel(wn, noise3, gold):
    """Seeded sweep inside the strip-march kernel's regime (rows of k*256 samples, 0.18 <= step <= 1/3): steps,
    row counts not divisible by 4, plane ranges that end inside an item, offsets beyond the tile period, a small
    tile.  Checker: the exact kernel on the same lattice (bit-identical to the oracle in the tests above)."""
    rng = np.random.default_rng(4099)
    small = wn.WaveletNoise.from_coefficients(gold["tile3d_16_12345"], 3)
    for case in range(24):
        octave = int(rng.integers(2, 6))
        step = float(rng.uniform(0.181, 0.332))
        den = max(1, int(round(8.0 * 2.0 ** octave / step)))
        nx = int(rng.choice([256, 512, 768, 1024]))
        ny = int(rng.integers(1, 38))
        nz = int(rng.choice([1, 2, 3, 31, 64, 127, 129, 200, 333]))
        z0 = int(rng.choice([0, 5, 511, 4097, 100000]))
        w = small if case % 4 == 3 else noise3
        tag = (case, den, nx, ny, z0, nz, octave)
        fast = wn.wavelet_volume(w, den, nx, ny, z0, z0 + nz, octave)
        exact = wn.wavelet_volume(w, den, nx, ny, z0, z0 + nz, octave, exact=True)
        err = float((fast - exact).abs().max())
        assert err <= TOL, (tag, err)


def test_generic_grid_descriptor_negative_and_constant_axes(wn, ora, noise3, tile3d_128):
    """Unusual descriptors: negative range and steps > 1/3 cell go to the direct kernel
    (bit-identical); a zero step (all samples on one point) stays within tolerance."""
    import ctypes as C
    from importlib import import_module
    noise_mod = import_module("wavelet-noise-in-ray-tracing_amd.noise")
    for base_range, oscale in ((-4.0, 16.0), (0.0, 16.0), (4.0, 0.0), (4.0, 1024.0)):
        g = wn.GridSpec(64, 40, 6, 2, 5, base_range=base_range, octave_scale=oscale, post_scale=2.0, out_scale=1.0)
        out = g.empty()
        gc = g.c()
        noise_mod.check(noise_mod._lib.wn_eval3d_grid(noise3._handle(3), C.byref(gc), noise_mod._ptr(out), noise_mod._stream()))
        got = host(out).reshape(3, 6, 40)
        idx = np.arange(40, dtype=np.float32)
        def coord(i):
            c = (np.float32(i) / np.float32(64)) * np.float32(base_range)
            return np.float32(np.float32(c * np.float32(oscale)) * np.float32(2.0))
        pts = np.array([[coord(x), coord(y), coord(z)] for z in range(2, 5) for y in range(6) for x in range(40)], np.float32)
        want = ora.evaluate3d(tile3d_128, pts).reshape(3, 6, 40)
        assert np.abs(got - want).max() <= TOL, (base_range, oscale)
        if base_range < 0 or oscale > 100:  # outside the brick kernel's regime -> direct kernel, bit-identical
            assert (bits(got) == bits(want)).all(), (base_range, oscale)


def test_grid_launches_are_stream_ordered_and_graph_capturable(wn, noise3):
    """The compute entry points only enqueue on the caller's stream (no allocation, no sync), so
    they can run on a side stream and be captured into a hipGraph and replayed."""
    ref = wn.wavelet_volume(noise3, 512, 512, 32, 0, 8, 4).clone()
    out = torch.zeros_like(ref).view(-1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        wn.wavelet_volume(noise3, 512, 512, 32, 0, 8, 4, out=out)  # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(out.view_as(ref), ref)
    out.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for z in range(0, 8, 2):  # four launches writing four sub-slabs
            wn.wavelet_volume(noise3, 512, 512, 32, z, z + 2, 4, out=out[z * 32 * 512:(z + 2) * 32 * 512])
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0  # capture records, it does not run
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view_as(ref), ref)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view_as(ref), ref)


def test_texture_without_tile_gives_half_grey(wn):
    """texture.h:100-104: neither noise object present -> noise_val = 0 -> 0.5*(1+clamp(0)) = 0.5."""
    import ctypes as C
    from importlib import import_module
    nm = import_module("wavelet-noise-in-ray-tracing_amd.noise")
    pts = torch.rand((1000, 3), device="cuda") * 20 - 10
    out = torch.full((1000,), -1.0, device="cuda")
    for use_3d in (1, 0):
        nm.check(nm._lib.wn_wavelet_texture_points(None, use_3d, 1.0, 4, nm._ptr(pts), None, 1000, nm._ptr(out), nm._stream()))
        assert bool((out == 0.5).all())
    empty = wn.WaveletNoise(128, 1)
    nm.check(nm._lib.wn_wavelet_texture_points(empty._handle(3), 1, 1.0, 4, nm._ptr(pts), None, 1000, nm._ptr(out), nm._stream()))
    assert bool((out == 0.5).all())


def test_multiband_constant_z_default_and_exact_agree_with_the_oracle(wn, ora, noise3, tile3d_128):
    """with z_mode == WN_Z_CONST band b sits at 2*z_const*2^(first_band+b); the default
    path must give the same values as WN_GRID_EXACT and as the composition of oracle evaluate3D calls."""
    import ctypes as C
    from importlib import import_module
    nm = import_module("wavelet-noise-in-ray-tracing_amd.noise")
    w = np.array([1.0, 0.5, 2.0, 1.0, 1.0], np.float32)
    den, nx, ny, zc = 512, 512, 24, 0.37
    i = np.arange(nx, dtype=np.float32)
    cx = (i / np.float32(den)) * np.float32(4.0)           # octave_scale = post_scale = 1
    cy = cx[:ny]
    pts = np.stack([np.broadcast_to(cx[None, :], (ny, nx)), np.broadcast_to(cy[:, None], (ny, nx)),
                    np.full((ny, nx), np.float32(zc), np.float32)], axis=-1).reshape(-1, 3)
    want = ora.multiband3d(tile3d_128, pts, -16.0, 0, 5, w, 0.18402).reshape(ny, nx)
    wa = (C.c_float * 5)(*[float(x) for x in w])
    got = {}
    for name, flags in (("default", nm.WN_GRID_DEFAULT), ("exact", nm.WN_GRID_EXACT)):
        g = wn.GridSpec(den, nx, ny, z_mode=nm.WN_Z_CONST, z_const=zc, flags=flags)
        out = g.empty()
        gc = g.c()
        nm.check(nm._lib.wn_multiband3d_grid(noise3._handle(3), C.byref(gc), -16.0, 0, 5, wa, 0.18402,
                                             nm._ptr(out), nm._stream()))
        got[name] = host(out).reshape(ny, nx)
    assert (bits(got["exact"]) == bits(want)).all()
    assert np.abs(got["default"] - want).max() <= TOL


def test_negative_plane_indices_go_to_the_exact_kernel(wn, ora, noise3, tile3d_128):
    """z0 < 0 is accepted (check_grid); the fast kernels' bounds assume indices >= 0, so such slabs are served
    by the direct kernel, bit-identical to evaluate3D."""
    got = host(wn.wavelet_volume(noise3, 512, 512, 8, -3, 2, 4))
    want = ora.grid_wavelet3d_volume(tile3d_128, 512, 512, 8, -3, 2, 4)
    assert (bits(got) == bits(want)).all()


def test_reference_named_generators_are_byte_identical_by_default(wn, noise3):
    """generate3DSlicedOctaveBandNoise keeps the reference's name, so its default output is the reference's
    file; the fast path is opt-in."""
    for octave in (3, 4, 5):
        got = host(wn.generate3DSlicedOctaveBandNoise(256, octave, None, noise3)).ravel()
        assert (bits(got) == bits(raw(f"wavelet_noise_3Dsliced_octave_{octave}.raw"))).all(), octave


def test_multiband_with_a_normal_points(wn, ora, noise3, tile3d_128):
    """WMultibandNoise(p, s, normal, ...) (paper App. 2, normal != NULL): bands are evaluate3DProjected; bit-exact
    against the oracle composition, with one normal for all points and with one normal per point."""
    rng = np.random.default_rng(11)
    pts = rng.uniform(-3, 3, (400, 3)).astype(np.float32)
    w = [1.0, 0.5, 2.0]
    one = np.array([[0.0, 0.0, 1.0]], np.float32)
    got = host(noise3.WMultibandNoise(pts, -16.0, 0, 3, w, normal=one))
    want = ora.multiband3d_projected(tile3d_128, pts, one, -16.0, 0, 3, w, 0.296)
    assert (bits(got) == bits(want)).all()
    nr = rng.normal(size=(400, 3)).astype(np.float32)
    nr /= np.linalg.norm(nr, axis=1, keepdims=True).astype(np.float32)
    got = host(noise3.WMultibandNoise(pts, -1.0, 0, 3, w, variance=0.25, normal=nr))
    want = ora.multiband3d_projected(tile3d_128, pts, nr, -1.0, 0, 3, w, 0.25)
    assert (bits(got) == bits(want)).all()
    # scalar call shape
    v = noise3.WMultibandNoise(pts[0], -16.0, 0, 3, w, normal=one)
    assert np.float32(v) == ora.multiband3d_projected(tile3d_128, pts[:1], one, -16.0, 0, 3, w, 0.296)[0]


def test_entry_points_from_several_host_threads_and_rand_is_preserved(wn, ora, noise3, tile3d_128):
    """per-device facts sit in mutex-protected tables and the rand() park/restore is depth-counted,
    so several host threads may be inside the library at once.  Four threads run different entry points (dense grid,
    Perlin grid, point list, scalar mailbox calls) concurrently, each on its own stream; every result must equal the
    single-threaded one, and the process's rand() stream must be the one it would be without the library."""
    import ctypes
    import threading
    libc = ctypes.CDLL(None)
    libc.srand(4242)
    expected_rand = [libc.rand() for _ in range(8)]
    libc.srand(4242)
    first_half = [libc.rand() for _ in range(4)]

    per = wn.perlin(12345)
    rng = np.random.default_rng(3)
    pts = rng.uniform(-20, 20, (5000, 3)).astype(np.float32)
    want_vol = host(wn.wavelet_volume(noise3, 512, 512, 16, 0, 4, 4))
    want_per = host(wn.perlin_volume(per, 256, 256, 16, 0, 4, 4))
    want_pts = host(noise3.evaluate3D(pts))
    want_scalar = [noise3.evaluate3D(pts[i]) for i in range(50)]
    torch.cuda.synchronize()
    errors = []

    def run(kind):
        try:
            stream = torch.cuda.Stream()
            with torch.cuda.stream(stream):
                for _ in range(6):
                    if kind == 0:
                        got = host(wn.wavelet_volume(noise3, 512, 512, 16, 0, 4, 4))
                        assert (bits(got) == bits(want_vol)).all()
                    elif kind == 1:
                        got = host(wn.perlin_volume(per, 256, 256, 16, 0, 4, 4))
                        assert (bits(got) == bits(want_per)).all()
                    elif kind == 2:
                        got = host(noise3.evaluate3D(pts))
                        assert (bits(got) == bits(want_pts)).all()
                    else:
                        got = [noise3.evaluate3D(pts[i]) for i in range(50)]
                        assert got == want_scalar
        except Exception as e:  # noqa: BLE001
            errors.append((kind, repr(e)))

    threads = [threading.Thread(target=run, args=(k,)) for k in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    second_half = [libc.rand() for _ in range(4)]
    assert first_half + second_half == expected_rand  # dozens of launches later the caller's stream is untouched


def test_perlin_run_kernel_odd_shapes_steps_and_descriptors(wn, ora):
    """The cell-sharing Perlin kernel (rows of >= 128 samples) on shapes and lattices that are not the benchmark's:
    rows that are no multiple of 8 / 512, bricks cut by ny / nz, steps from 1/128 to > 1 (several cells per run:
    the per-lane segment loops), a negative range, a constant z, a non-power-of-two divisor, an unaligned output --
    noise, turb and fractal_noise, every value bit for bit against the oracle's scalar noise()."""
    import ctypes as C
    from importlib import import_module
    nm = import_module("wavelet-noise-in-ray-tracing_amd.noise")
    p = wn.perlin(5489)
    perm = ora.perlin_perm(5489)

    def coords(n, den, base_range, oscale):
        i = np.arange(n, dtype=np.float32)
        return ((i / np.float32(den)) * np.float32(base_range)) * np.float32(oscale)

    cases = [  # den, nx, ny, z0, z1, base_range, octave_scale, z_const or None
        (512, 512, 9, 3, 12, 4.0, 16.0, None),      # bricks cut in y and z
        (131, 131, 5, 0, 3, 4.0, 16.0, None),       # ragged row, non-power-of-two divisor
        (300, 643, 3, 7, 9, 4.0, 1.0, None),        # two x segments, the second ragged; step 1/75
        (256, 256, 4, 0, 2, 4.0, 77.0, None),       # step 1.2: a new cell every sample
        (256, 200, 4, 1, 2, 4.0, 19.2, None),       # step 0.3: cells change inside runs at lane-dependent places
        (256, 256, 3, 0, 2, -4.0, 8.0, None),       # negative coordinates, descending
        (256, 256, 6, 0, 1, 4.0, 32.0, 0.37),       # constant z (the "sliced" generators)
    ]
    for den, nx, ny, z0, z1, base_range, oscale, zc in cases:
        cx, cy = coords(nx, den, base_range, oscale), coords(ny, den, base_range, oscale)
        cz = np.full(1, np.float32(zc), np.float32) if zc is not None else coords(z1, den, base_range, oscale)[z0:z1]
        nz = len(cz)
        pts = np.stack(np.broadcast_arrays(cx[None, None, :], cy[None, :, None], cz[:, None, None]), axis=-1).reshape(-1, 3)
        g = wn.GridSpec(den, nx, ny, z0, z1, base_range=base_range, octave_scale=oscale,
                        z_mode=nm.WN_Z_CONST if zc is not None else nm.WN_Z_LATTICE, z_const=zc or 0.0)
        buf = torch.empty(nz * ny * nx + 1, dtype=torch.float32, device="cuda")
        for shift in (0, 1):  # shift 1: the output rows are not 16-byte aligned (scalar stores)
            out = buf[shift:shift + nz * ny * nx]
            gc = g.c()
            nm.check(nm._lib.wn_perlin_grid(p._h, C.byref(gc), nm._ptr(out), nm._stream()))
            want = ora.perlin_noise(perm, pts.astype(np.float64)).astype(np.float32)
            assert (bits(host(out)) == bits(want)).all(), ("noise", den, nx, ny, oscale, shift)
        nm.check(nm._lib.wn_perlin_turb_grid(p._h, C.byref(gc), 5, nm._ptr(out), nm._stream()))
        want = ora.perlin_turb(perm, pts, 5).astype(np.float32)
        assert (bits(host(out)) == bits(want)).all(), ("turb", den, nx, ny, oscale)
        nm.check(nm._lib.wn_perlin_fractal_grid(p._h, C.byref(gc), nm._ptr(out), nm._stream()))
        want = ora.perlin_fractal(perm, pts).astype(np.float32)
        assert (bits(host(out)) == bits(want)).all(), ("fractal", den, nx, ny, oscale)


def test_scalar_entry_points_conventions_and_errors(wn, ora, noise3, noise2, tile3d_128):
    """wn_scalar_*: the reference's value-level conventions (empty tile -> 0.0f, no-tile texture -> 0.5), argument
    errors reported like every other entry point, restart after the resident kernel's idle exit, and agreement with
    the batched kernels for every op."""
    import ctypes as C
    import time
    from importlib import import_module
    nm = import_module("wavelet-noise-in-ray-tracing_amd.noise")
    lib = nm._lib
    f3 = (C.c_float * 3)(1.25, -3.75, 100.1)
    out = C.c_float(-1)
    empty = wn.WaveletNoise(128, 1)
    assert lib.wn_scalar_eval3d(empty._handle(3), f3, C.byref(out)) == 0 and out.value == 0.0
    assert lib.wn_scalar_wavelet_texture(None, 1, 1.0, 4, f3, C.byref(out)) == 0 and out.value == 0.5
    assert lib.wn_scalar_eval3d(None, f3, C.byref(out)) == nm._capi.WN_ERR_INVALID
    assert lib.wn_scalar_eval3d(noise2._handle(2), f3, C.byref(out)) == nm._capi.WN_ERR_INVALID  # 2-D tile
    assert b"3-D tile" in lib.wn_last_error()
    # every op against its batched twin
    rng = np.random.default_rng(9)
    pts = rng.uniform(-30, 30, (64, 3)).astype(np.float32)
    nrm = np.array([0.0, 0.6, 0.8], np.float32)
    per = wn.perlin(12345)
    wt, pt = wn.wavelet_texture(1.0, 4, True), wn.noise_texture(1.0, 4)
    b3, b2 = host(noise3.evaluate3D(pts)), host(noise2.evaluate2D(pts[:, :2]))
    bp = host(noise3.evaluate3DProjected(pts, nrm))
    bn, bt, bf = host(per.noise(pts)), host(per.turb(pts, 4)), host(per.fractal_noise(pts))
    bw, bq = host(wt.grey(pts)), host(pt.grey(pts))
    for i in (0, 1, 2, 33, 63):
        if i == 33:
            time.sleep(0.02)  # the resident kernel has ended by now (2 ms idle): the next call restarts it
        assert np.float32(noise3.evaluate3D(pts[i])) == b3[i]
        assert np.float32(noise2.evaluate2D(pts[i, :2])) == b2[i]
        assert np.float32(noise3.evaluate3DProjected(pts[i], nrm)) == bp[i]
        assert per.noise(pts[i]) == bn[i] and per.turb(pts[i], 4) == bt[i] and per.fractal_noise(pts[i]) == bf[i]
        assert per.noise(float(pts[i, 0]), float(pts[i, 1]), float(pts[i, 2])) == bn[i]
        assert np.float32(wt.value(0, 0, pts[i])[0]) == bw[i] and np.float32(pt.value(0, 0, pts[i])[0]) == bq[i]
    calls, launches = C.c_ulonglong(0), C.c_ulonglong(0)
    assert lib.wn_scalar_stats(C.byref(calls), C.byref(launches)) == 0
    assert calls.value >= 45 and 1 <= launches.value <= calls.value


def test_full_512_cubed_perlin_and_turb_planes_and_properties(wn, ora):
    """BASELINE sizes for the Perlin grids: the whole 512^3 noise and turb(7) volumes are produced by the run kernel;
    sampled planes are compared bit for bit with the oracle, and the whole volumes through size-independent
    properties: turb >= 0 everywhere, |noise| below the gradient set's bound (~1.036), noise vanishes on integer lattice points (every 8th sample on
    every axis at this lattice), and the volume is the same when produced in two z-slabs."""
    per = wn.perlin(12345)
    perm = ora.perlin_perm(12345)
    vol = wn.perlin_volume(per, 512, 512, 512, 0, 512, 4)
    for z in (0, 77, 511):
        want = ora.grid_perlin_volume(perm, 512, 512, 512, z, z + 1, 4)[0]
        assert (bits(host(vol[z])) == bits(want)).all(), z
    assert float(vol.abs().max()) <= 1.04  # improved noise with these 12 gradients peaks at ~1.036, not 1
    assert float(vol[::8, ::8, ::8].abs().max()) == 0.0  # gradient noise is zero at lattice points
    halves = torch.cat([wn.perlin_volume(per, 512, 512, 512, 0, 200, 4), wn.perlin_volume(per, 512, 512, 512, 200, 512, 4)])
    assert torch.equal(halves, vol)
    del halves
    tv = wn.turb_volume(per, 512, 512, 512, 0, 512, 7)
    for z in (3, 300):
        want = ora.grid_turb_volume(perm, 512, 512, 512, z, z + 1, 7)[0]
        assert (bits(host(tv[z])) == bits(want)).all(), z
    assert float(tv.min()) >= 0.0 and bool(torch.isfinite(tv).all())


# ---- WMultibandNoise on dense lattices: the plane-pipeline kernel (wn_wavelet_multiband.hip) ------------------------------
def test_multiband_plane_pipeline_shapes_vs_exact_kernel_and_oracle(wn, ora, noise3, tile3d_128):
    """Wide lattices of 2..5 bands go to grid3d_mbp_kernel (16-wave workgroups: window, collapse and store waves around
    one barrier per plane) -- except those whose last 512-wide brick would be more than 10 % padding (516, 1028, 768
    below), which the brick kernel serves (tests/test_gpu_dispatch.py pins both).  Edge bricks in x / y / z, slabs that do not start at plane 0, band counts, weights, first bands
    and `s` cut-offs: every case against the bit-exact kernel (itself bit-identical to the oracle composition, checked
    in test_multiband_grid_and_points) on the whole lattice, and two planes per case against the oracle itself."""
    cases = [  # den, nx, ny, z0, z1, s, first, nbands, w
        (512, 512, 24, 3, 14, -16.0, 0, 5, [1.0, 1.0, 1.0, 1.0, 1.0]),
        (512, 516, 13, 0, 11, -16.0, 0, 5, [1.0, 0.5, 2.0, 1.0, 0.25]),     # ragged in x, y and z: brick kernel <5, 1>
        (1024, 1024, 9, 5, 22, -16.0, 0, 5, [1.0, 1.0, 1.0, 1.0, 1.0]),    # two bricks in x, finer steps (K = 4 passes)
        (512, 512, 17, 100, 109, -16.0, 0, 4, [0.5, 2.0, 1.0, 1.0]),
        (512, 1028, 8, 0, 8, -16.0, 1, 3, [1.0, 0.5, 2.0]),                 # 1028 wide: brick kernel <3, 1> (256-wide bricks)
        (512, 512, 8, 7, 9, -16.0, 2, 2, [1.0, 3.0]),
        (512, 512, 10, 0, 9, -3.0, 0, 5, [1.0, 1.0, 1.0, 1.0, 1.0]),        # s + b < 0 stops after 3 bands, variance over 5
        (1000, 1000, 11, 3, 14, -16.0, -1, 5, [1.0, 0.5, 2.0, 1.0, 0.25]),  # partial x-brick (488 of 512) in the pipeline
        (960, 960, 9, 9, 18, -4.0, -1, 6, [2.0, 1.0, 0.5, 1.0, 1.0, 1.0]),   # s stops after 5 of 6 bands, partial x-brick
        (768, 768, 16, 60, 70, -16.0, 0, 5, [1.0, 1.0, 1.0, 1.0, 1.0]),     # den not a power of two: brick kernel <5, 1>
    ]
    for den, nx, ny, z0, z1, s, first, nb, w in cases:
        fast = wn.multiband_volume(noise3, den, nx, ny, z0, z1, s, first, nb, w)
        exact = wn.multiband_volume(noise3, den, nx, ny, z0, z1, s, first, nb, w, exact=True)
        err = float((fast - exact).abs().max())
        assert err <= TOL, (den, nx, ny, z0, z1, s, first, nb, err)
        assert bool(torch.isfinite(fast).all())
        for z in (z0, z1 - 1):
            want = ora.grid_multiband3d_volume(tile3d_128, den, nx, ny, z, z + 1, s, first, nb, w, 0.18402)[0]
            assert np.abs(host(fast[z - z0]) - want).max() <= TOL, (den, nx, ny, z)
    # many bricks per workgroup, every workgroup busy: 512 x 512 x 40 planes = 1280 bricks on 256 CUs
    fast = wn.multiband_volume(noise3, 512, 512, 512, 8, 48)
    exact = wn.multiband_volume(noise3, 512, 512, 512, 8, 48, exact=True)
    assert float((fast - exact).abs().max()) <= TOL
    # output buffers handed in by the caller are written in place and nowhere else
    buf = torch.full((512 * 512 * 10 + 64,), 7.0, dtype=torch.float32, device="cuda")
    got = wn.multiband_volume(noise3, 512, 512, 512, 0, 10, out=buf)
    assert torch.equal(got, wn.multiband_volume(noise3, 512, 512, 512, 0, 10))
    assert bool((buf[512 * 512 * 10:] == 7.0).all())


def test_full_512_cubed_multiband_volume_planes_and_properties(wn, ora, noise3, tile3d_128):
    """BASELINE configs[2](A) at full size: the 512^3 x 5-band WMultibandNoise volume.  Three sampled planes against the
    oracle's composition of evaluate3D calls (<= 1e-5), z-slabs computed separately bit-identical to the full call
    (shard-safety), finite, mean ~ 0 and a standard deviation of ~ 0.77 (five independent bands of variance ~ 0.18402,
    divided by sqrt(5 * 0.18402))."""
    N = 512
    vol = wn.multiband_volume(noise3, N, N, N, 0, N)
    assert vol.shape == (N, N, N)
    for z in (0, 301, 511):
        want = ora.grid_multiband3d_volume(tile3d_128, N, N, N, z, z + 1, -16.0, 0, 5, [1.0] * 5, 0.18402)[0]
        err = float(np.abs(host(vol[z]) - want).max())
        assert err <= TOL, (z, err)
    for z0, z1 in ((200, 208), (3, 30), (505, 512)):
        part = wn.multiband_volume(noise3, N, N, N, z0, z1)
        assert torch.equal(part, vol[z0:z1]), (z0, z1)
    assert bool(torch.isfinite(vol).all())
    assert abs(float(vol.double().mean())) < 2e-2
    assert 0.6 < float(vol.std()) < 0.95
    assert float(vol.abs().max()) < 5.0


def test_device_wide_sync_from_another_thread_is_not_held_up_by_a_burst_of_scalar_calls(wn, ora, noise3, tile3d_128):
    """Round-2 ADVICE: the resident scalar kernel used to restart its idle timer with every request, so a thread that kept
    calling wn_scalar_* held every other thread's device-wide synchronise (torch.cuda.synchronize, the hipFree inside
    wn_dev_free) for the length of its burst.  An instance now ends 20 ms after its start however busy it is: while thread
    A makes scalar calls for about a second, thread B's synchronises and frees each return within a fraction of that
    (bound: 0.5 s, two orders above the 20 ms), and A's values stay those of the oracle."""
    import ctypes as C
    import threading
    import time
    from importlib import import_module
    nm = import_module("wavelet-noise-in-ray-tracing_amd.noise")
    lib = nm._lib
    rng = np.random.default_rng(21)
    pts = rng.uniform(-50, 50, (4000, 3)).astype(np.float32)
    want = ora.evaluate3d(tile3d_128, pts)
    handle = noise3._handle(3)
    stop = threading.Event()
    got = np.zeros(len(pts), np.float32)
    calls = [0]
    errors = []

    def burst():
        try:
            out = C.c_float(0)
            arr = (C.c_float * 3)()
            t_end = time.perf_counter() + 1.2
            while time.perf_counter() < t_end and not stop.is_set():
                i = calls[0] % len(pts)
                arr[0], arr[1], arr[2] = float(pts[i, 0]), float(pts[i, 1]), float(pts[i, 2])
                nm.check(lib.wn_scalar_eval3d(handle, arr, C.byref(out)))
                got[i] = out.value
                calls[0] += 1
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    th = threading.Thread(target=burst)
    th.start()
    time.sleep(0.15)
    waits = []
    for _ in range(5):
        t0 = time.perf_counter()
        torch.cuda.synchronize()
        waits.append(time.perf_counter() - t0)
        p = C.c_void_p()
        t0 = time.perf_counter()
        nm.check(lib.wn_dev_alloc(C.byref(p), 1 << 20))
        nm.check(lib.wn_dev_free(p))
        waits.append(time.perf_counter() - t0)
        time.sleep(0.05)
    stop.set()
    th.join()
    assert not errors, errors
    assert calls[0] > 2000, calls[0]           # the burst really ran beside the synchronises
    assert max(waits) < 0.5, waits             # none of them waited for the burst to end
    n = min(calls[0], len(pts))
    assert (bits(got[:n]) == bits(want[:n])).all()
    cs, ls = C.c_ulonglong(0), C.c_ulonglong(0)
    nm.check(lib.wn_scalar_stats(C.byref(cs), C.byref(ls)))
    assert ls.value >= 2  # instances ended and were restarted during the burst
