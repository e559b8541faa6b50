"""HIP-event timing (wn_timer) of the bounded curl brick-list kernels (csrc/wn_wavelet_bounded_bricks.hip,
include/wnoise_bounded_bricks.h) on one MI355X, in the manner of profiles/brick_fields_timing.py: the headline lattice (den
512, tile 128, octave 4; five bands: WMultibandNoise from band 0), the default offsets, and the lists of
profiles/bricks_timing.py -- all 262,144 bricks in raster order, a uniform random 10 % in random order, the bricks cut by
the sphere of radius 200 samples about the centre.

Every figure is a comparison of two calls timed ALTERNATELY in the same process: per round a burst of the one between two
events, then a burst of the other, bursts of about 0.1 s (at least 3 launches); the medians over the rounds are compared and
the rounds' extreme ratios are the spread.

    bar (a)   wn_*_curl_bounded_bricks against wn_*_curl_bounded_points on exactly the same samples (512 float coordinates per
              brick), with the scene of tests/test_gpu_bounded_bricks.py scaled to the volume, on every list, in both tiers:
              the brick call takes no more than 1.0 x the point call.
    bar (b)   nobs == 0 against wn_*_curl_bricks (default tier): the same kernel, so within the spread.
    no bar    against the unbounded default-tier curl bricks: a scene in which every sample is near (one container whose ramp
              covers the volume: the value sums and the combination everywhere); scenes in which every sample is far, with
              1, 3 and 16 obstacles (the ramp's cost per obstacle); and the scaled scene on a list of bricks that lie wholly
              inside its sphere (no fill, no band loop).

    python profiles/bounded_bricks_timing.py [--quick] [--out profiles/bounded_bricks_kernels.txt]

The driver runs every step as a child process under its own `timeout`, stops at the first step that fails, and writes the
steps' JSON lines to --out."""
import ctypes as C
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import bricks_timing as bt  # noqa: E402

STEPS = {"one_band": 400, "five_bands": 400}   # seconds allowed
QUICK = "--quick" in sys.argv
N = bt.N
K = N / 40.0                                    # the tests' scene lives on 40 samples


def scene(h, k=K):
    c = (19.5 * k * h, 11.5 * k * h, 19.5 * k * h)
    return [("sphere", c, 7.0 * k * h, 5.0 * k * h), ("halfspace", (0.0, 1.0, 0.0), 2.5 * k * h, 3.0 * k * h),
            ("container", c, 28.0 * k * h, 5.0 * k * h)]


def near_scene(h):
    """One container about the centre whose ramp covers the whole volume: 0 < d < d0 at every sample but the centre."""
    return [("container", (0.5 * N * h,) * 3, 500.0 * h, 500.0 * h)]


def far_scene(h, count):
    """`count` spheres far outside the volume: every sample is far from all of them, and every distance is evaluated."""
    return [("sphere", ((2000.0 + 100.0 * j) * h, -1500.0 * h, 3000.0 * h), 10.0 * h, 20.0 * h) for j in range(count)]


def inside_list(np):
    """The bricks that lie wholly inside the scaled scene's sphere, in raster order."""
    full = bt.brick_lists(np)["full_raster"].astype(np.float64)
    c, r = np.array([19.5, 11.5, 19.5]) * K, 7.0 * K
    lo, hi = full * 8.0 - c, full * 8.0 + 7.0 - c
    far = np.maximum(np.abs(lo), np.abs(hi))
    keep = np.sqrt((far ** 2).sum(1)) < r
    return np.ascontiguousarray(full[keep].astype(np.int32))


def alternate(wn, np, torch, launch_a, launch_b, rounds=5, burst_s=0.1):
    """Medians (us per launch) of a and b over `rounds` alternating bursts, and the rounds' smallest and largest a / b."""
    for _ in range(3):
        launch_a()
        launch_b()
    torch.cuda.synchronize()
    t = wn.HipTimer()

    def burst(launch, k):
        t.start()
        for _ in range(k):
            launch()
        t.stop()
        return t.elapsed_ms() * 1e3 / k

    ka = max(3, int(burst_s * 1e6 / max(burst(launch_a, 3), 1.0)))
    kb = max(3, int(burst_s * 1e6 / max(burst(launch_b, 3), 1.0)))
    if QUICK:
        ka, kb, rounds = min(ka, 3), min(kb, 3), 2
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(burst(launch_a, ka))
        tb.append(burst(launch_b, kb))
    ratios = [a / b for a, b in zip(ta, tb)]
    return float(np.median(ta)), float(np.median(tb)), min(ratios), max(ratios), rounds


def step(name):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    wn = importlib.import_module("wavelet-noise-in-ray-tracing_amd")
    nm = importlib.import_module("wavelet-noise-in-ray-tracing_amd.noise")
    torch.cuda.set_device(0)
    lib, st = nm._lib, nm._stream()
    bands = {"one": 1, "five": 5}[name.split("_")[0]]

    noise = wn.WaveletNoise(128, 12345)
    noise.generateNoiseTile3D()
    h = noise._handle(3)
    off = noise._curl_offsets(None)
    w5 = (C.c_float * 5)(*[1.0] * 5)
    if bands == 1:
        os_, post, scale = nm._octave_scale(4), 2.0, nm._inv_stddev(0.18402)
    else:
        os_, post, scale = 1.0, 1.0, 1.0
    mb = () if bands == 1 else (-16.0, 0, 5, w5, 0.18402)
    stem = "wn_eval3d" if bands == 1 else "wn_multiband3d"
    f_points, f_bricks, f_free = (getattr(lib, f"{stem}_curl_{what}") for what in ("bounded_points", "bounded_bricks", "bricks"))
    step_h = ((1.0 / N) * 4.0) * os_ * post          # the lattice's step in the obstacles' coordinate

    def grid(flags):
        return wn.GridSpec(N, N, N, 0, N, octave_scale=os_, post_scale=post, out_scale=scale, flags=flags).c()

    def compare(label, launch_a, launch_b, what, **extra):
        a, b, lo, hi, rounds = alternate(wn, np, torch, launch_a, launch_b)
        line = {"name": label, "us": round(a, 2), f"{what}_us": round(b, 2), "ratio": round(a / b, 4), "ratio_min": round(lo, 4),
                "ratio_max": round(hi, 4), "rounds": rounds, **extra}
        print(json.dumps(line), flush=True)
        return line

    tiers = ((nm.WN_GRID_DEFAULT, "default"), (nm.WN_GRID_EXACT, "exact"))
    local = torch.arange(512, device="cuda")
    offs = torch.stack([local & 7, (local >> 3) & 7, local >> 6], -1)                   # (512, 3): lx, ly, lz
    lists = dict(bt.brick_lists(np))
    lists["inside_the_sphere"] = inside_list(np)
    so, sn = noise._obstacles(scene(step_h))
    for lname, host_list in lists.items():
        n = len(host_list)
        bricks = torch.from_numpy(host_list).cuda()
        out = torch.empty(3 * n * 512, dtype=torch.float32, device="cuda")
        gd = grid(nm.WN_GRID_DEFAULT)

        def bounded(gc, obs, nobs):
            return lambda: nm.check(f_bricks(h, C.byref(gc), nm._ptr(bricks), n, off, *mb, obs, nobs, nm._ptr(out), st))

        def free(gc=gd):
            nm.check(f_free(h, C.byref(gc), nm._ptr(bricks), n, off, *mb, nm._ptr(out), st))

        if lname == "inside_the_sphere":
            compare(f"bounded_{lname}_{name}_default_over_unbounded", bounded(gd, so, sn), free, "unbounded", bricks=n, samples=n * 512)
            del out, bricks
            continue
        # bar (a): the same samples as a point list, c = (((float)i / den) * 4) * octave_scale * post_scale per axis
        idx = (bricks[:, None, :] * 8 + offs[None, :, :]).to(torch.float32).reshape(-1, 3)
        pts = ((((idx / float(N)) * 4.0) * os_) * post).contiguous()
        del idx

        def points():
            nm.check(f_points(h, nm._ptr(pts), n * 512, off, *mb, so, sn, nm._ptr(out), st))
        for flags, tier in tiers:
            line = compare(f"bounded_{lname}_{name}_{tier}_over_points", bounded(grid(flags), so, sn), points, "points", bricks=n,
                           samples=n * 512)
            print(json.dumps({"name": f"bounded_{lname}_{name}_{tier}_bar_a", "bricks_over_points": line["ratio"],
                              "bar_1.0_met": line["ratio"] <= 1.0, "G_samples_per_s": round(n * 512 / line["us"] * 1e-3, 2)}), flush=True)
        del pts
        # bar (b): no obstacle is the unbounded call
        none, zero = noise._obstacles([])
        line = compare(f"bounded_{lname}_{name}_default_nobs0_over_unbounded", bounded(gd, none, zero), free, "unbounded", bricks=n)
        print(json.dumps({"name": f"bounded_{lname}_{name}_bar_b", "nobs0_over_unbounded": line["ratio"],
                          "within_the_spread": line["ratio_min"] <= 1.0 <= line["ratio_max"] or abs(line["ratio"] - 1.0) <= 0.02}), flush=True)
        # no bar: the scene, every sample near, every sample far from 1, 3, 16 obstacles -- against the unbounded curl bricks
        for sname, obstacles in (("scene", scene(step_h)), ("all_near", near_scene(step_h)), ("all_far_1", far_scene(step_h, 1)),
                                 ("all_far_3", far_scene(step_h, 3)), ("all_far_16", far_scene(step_h, 16))):
            obs, nobs = noise._obstacles(obstacles)
            compare(f"bounded_{lname}_{name}_default_{sname}_over_unbounded", bounded(gd, obs, nobs), free, "unbounded", bricks=n, nobs=nobs)
        del out, bricks
    torch.cuda.synchronize()
    print(json.dumps({"name": "device", **wn.device_info(), "time": time.strftime("%Y-%m-%d")}), flush=True)


def main():
    out = os.path.join(ROOT, "profiles", "bounded_bricks_kernels.txt")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    text = ["Bounded curl brick-list kernels (csrc/wn_wavelet_bounded_bricks.hip) on one MI355X: python profiles/bounded_bricks_timing.py"
            + (" --quick" if QUICK else ""),
            "(HIP events on the launch stream; microseconds per launch; den 512, tile 128, octave 4; every line compares two calls",
            " timed alternately in one process: `us` over `points_us` / `unbounded_us`, medians of `rounds` bursts of about 0.1 s;",
            " ratio_min .. ratio_max are the rounds' extremes.  One run of the script.)", ""]
    rc = 0
    for name, limit in STEPS.items():
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name] + (["--quick"] if QUICK else [])
        res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
        print(res.stdout, end="", flush=True)
        text += [f"[{name}]"] + res.stdout.splitlines() + [""]
        if res.returncode != 0:   # nothing more runs on the device after a failed step
            print(res.stderr[-3000:], file=sys.stderr)
            text += [f"step {name} failed with exit status {res.returncode}; later steps were not run"]
            rc = 1
            break
    with open(out, "w") as f:
        f.write("\n".join(text) + "\n")
    return rc


if __name__ == "__main__":
    if "--step" in sys.argv:
        step(sys.argv[sys.argv.index("--step") + 1])
    else:
        sys.exit(main())
