"""HIP-event timing of the surface gradient kernels (csrc/wn_wavelet_grad_surface.hip) on one MI355X, each beside the
value kernel of the same call:

  * 16,777,216 random points in [-300, 300]^3, tile 128, one random unit normal per point: wn_eval3d_projected_points
    and wn_eval3d_projected_grad_points;
  * the 512 x 512 x 64 lattice of wavelet_volume at octave 4 with normals (0, 0, 1) and (1, 1, 1)/sqrt(3):
    wn_eval3d_projected_grid and wn_eval3d_projected_grad_grid;
  * the 4096^2 image of generate2DOctaveBandNoise at octave 4 (2-D tile 128): wn_eval2d_grid and wn_eval2d_grad_grid;
  * 16,777,216 random points in [-300, 300]^2: wn_eval2d_points and wn_eval2d_grad_points.

One JSON line per measurement, then one per case with the ratio gradient / value of the sustained times.

    python profiles/grad_surface_timing.py [--quick]

Per-launch time: the mean of `launches` single launches, each between its own two events.  Sustained: back-to-back
launches for about one second between two events, divided by their number."""
import ctypes as C
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

wn = importlib.import_module("wavelet-noise-in-ray-tracing_amd")
nm = importlib.import_module("wavelet-noise-in-ray-tracing_amd.noise")
QUICK = "--quick" in sys.argv


def measure(launch, launches=20, sustain_s=1.0):
    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    t = wn.HipTimer()
    per = []
    for _ in range(launches):
        t.start()
        launch()
        t.stop()
        per.append(t.elapsed_ms() * 1e3)
    k = max(1, int(sustain_s * 1e6 / max(np.median(per), 1.0)))
    if QUICK:
        k = min(k, 20)
    t.start()
    for _ in range(k):
        launch()
    t.stop()
    return float(np.mean(per)), float(np.min(per)), t.elapsed_ms() * 1e3 / k, k


def report(name, launch, work, unit, **extra):
    mean, best, sustained, k = measure(launch)
    line = {"name": name, "launch_us_mean": round(mean, 2), "launch_us_min": round(best, 2),
            "sustained_us": round(sustained, 2), "sustained_launches": k,
            f"{unit}_per_s_sustained": work / (sustained * 1e-6), **extra}
    print(json.dumps(line), flush=True)
    return line


def pair(case, value_launch, grad_launch, work, unit, target):
    v = report(f"{case}_value", value_launch, work, unit)
    g = report(f"{case}_gradient", grad_launch, work, unit)
    ratio = g["sustained_us"] / v["sustained_us"]
    print(json.dumps({"name": f"{case}_ratio", "gradient_over_value": round(ratio, 3), "target_at_most": target,
                      "met": ratio <= target}), flush=True)


def checked(fn, *args):
    def launch():
        rc = fn(*args)
        if rc:
            nm.check(rc)
    launch.keep = args
    return launch


def main():
    torch.cuda.set_device(0)
    st = nm._stream()
    noise3 = wn.WaveletNoise(128, 12345)
    noise3.generateNoiseTile3D()
    noise2 = wn.WaveletNoise(128, 12345)
    noise2.generateNoiseTile2D()
    h3, h2 = noise3._handle(3), noise2._handle(2)
    npts = 1 << 24
    rng = np.random.default_rng(1)

    # projected points: one random unit normal per point
    pts = torch.from_numpy(rng.uniform(-300.0, 300.0, (npts, 3)).astype(np.float32)).cuda()
    nr = torch.from_numpy(rng.normal(size=(npts, 3)).astype(np.float32)).cuda()
    nr = (nr / nr.norm(dim=1, keepdim=True)).contiguous()
    o1 = torch.empty(npts, dtype=torch.float32, device="cuda")
    o4 = torch.empty((npts, 4), dtype=torch.float32, device="cuda")
    pair("projected_points_16M_random", checked(nm._lib.wn_eval3d_projected_points, h3, nm._ptr(pts), nm._ptr(nr), npts,
                                                nm._ptr(o1), st),
         checked(nm._lib.wn_eval3d_projected_grad_points, h3, nm._ptr(pts), nm._ptr(nr), npts, nm._ptr(o4), st),
         npts, "points", 2.5)
    del pts, nr, o4
    torch.cuda.empty_cache()

    # projected grid: 512 x 512 x 64 at octave 4
    s3 = float(np.float32(1.0 / np.sqrt(3.0)))
    g = wn.GridSpec(512, 512, 512, 0, 64, octave_scale=nm._octave_scale(4), post_scale=2.0,
                    out_scale=nm._inv_stddev(0.296))
    gc = g.c()
    vol = g.nz * g.ny * g.nx
    out4 = torch.empty(4 * vol, dtype=torch.float32, device="cuda")
    for tag, normal in (("n001", (0.0, 0.0, 1.0)), ("n111", (s3, s3, s3))):
        na = (C.c_float * 3)(*normal)
        pair(f"projected_grid_512x512x64_{tag}",
             checked(nm._lib.wn_eval3d_projected_grid, h3, C.byref(gc), na, nm._ptr(out4), st),
             checked(nm._lib.wn_eval3d_projected_grad_grid, h3, C.byref(gc), na, nm._ptr(out4), st), vol, "samples", 2.5)
    del out4
    torch.cuda.empty_cache()

    # 2-D image: generate2DOctaveBandNoise's lattice at 4096^2, octave 4
    g2 = wn.GridSpec(4096, 4096, 4096, octave_scale=nm._octave_scale(4), post_scale=2.0, out_scale=nm._inv_stddev(0.19686))
    gc2 = g2.c()
    out3 = torch.empty(3 * 4096 * 4096, dtype=torch.float32, device="cuda")
    pair("image2d_4096^2", checked(nm._lib.wn_eval2d_grid, h2, C.byref(gc2), nm._ptr(out3), st),
         checked(nm._lib.wn_eval2d_grad_grid, h2, C.byref(gc2), nm._ptr(out3), st), 4096 * 4096, "samples", 2.0)
    del out3

    # 2-D points
    pts2 = torch.from_numpy(rng.uniform(-300.0, 300.0, (npts, 2)).astype(np.float32)).cuda()
    o3 = torch.empty((npts, 3), dtype=torch.float32, device="cuda")
    pair("points2d_16M_random", checked(nm._lib.wn_eval2d_points, h2, nm._ptr(pts2), npts, nm._ptr(o1), st),
         checked(nm._lib.wn_eval2d_grad_points, h2, nm._ptr(pts2), npts, nm._ptr(o3), st), npts, "points", 2.0)
    torch.cuda.synchronize()
    print(json.dumps({"name": "device", **wn.device_info(), "time": time.strftime("%Y-%m-%d")}), flush=True)


if __name__ == "__main__":
    main()
