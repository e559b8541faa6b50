"""HIP-event timing of the Perlin gradient kernels (csrc/wn_perlin_grad.hip) on one MI355X, each beside the value kernel
of the same call (csrc/wn_perlin.hip) in the same run:

  * the 512^3 lattice of perlin_volume at octave 4: wn_perlin_grid and wn_perlin_grad_grid;
  * the 512^3 lattice of turb_volume at depth 7: wn_perlin_turb_grid and wn_perlin_turb_grad_grid (the run form), and the
    generic gradient kernel on a 120 x 2048 x 546 lattice of the same step and (within 0.03 %) the same sample count,
    which is what the 512-wide lattice would get if turb were routed to it;
  * 16,777,216 random points in [-300, 300]^3: wn_perlin_points_vec3 / wn_perlin_grad_points_vec3 and
    wn_perlin_turb_points / wn_perlin_turb_grad_points at depth 7.

One JSON line per measurement, then one per case with the ratio gradient / value of the sustained times.  The bar: a
caller without the gradient entry points takes the value and three one-sided differences, four value launches, so
every ratio must stay below 4.

    python profiles/perlin_grad_timing.py [--quick]

Warm-up: back-to-back launches for at least 0.1 s.  Per-launch time: the mean of `launches` single launches, each between
its own two events.  Sustained: back-to-back launches for about one second between two events, divided by their number."""
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


def measure(launch, launches=20, sustain_s=1.0, warm_s=0.1):
    t0 = time.perf_counter()
    while True:
        for _ in range(3):
            launch()
        torch.cuda.synchronize()
        if QUICK or time.perf_counter() - t0 >= warm_s:
            break
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


def pair(case, value_launch, grad_launch, work, unit):
    v = report(f"{case}_value", value_launch, work, unit)
    g = report(f"{case}_gradient", grad_launch, work, unit)
    ratio = g["sustained_us"] / v["sustained_us"]
    print(json.dumps({"name": f"{case}_ratio", "gradient_over_value": round(ratio, 3), "bar_below": 4.0,
                      "met": ratio < 4.0}), flush=True)
    return v, g


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
    lib = nm._lib
    p = wn.perlin(12345)
    n = 512
    vol = n * n * n
    gvol = 120 * 2048 * 546
    out4 = torch.empty(4 * max(vol, gvol), dtype=torch.float32, device="cuda")

    gn = wn.GridSpec(n, n, n, 0, n, octave_scale=nm._octave_scale(4)).c()
    pair("perlin_grid_512^3_octave4", checked(lib.wn_perlin_grid, p._h, C.byref(gn), nm._ptr(out4), st),
         checked(lib.wn_perlin_grad_grid, p._h, C.byref(gn), nm._ptr(out4), st), vol, "samples")

    gt = wn.GridSpec(n, n, n, 0, n).c()
    _, run = pair("turb7_grid_512^3", checked(lib.wn_perlin_turb_grid, p._h, C.byref(gt), 7, nm._ptr(out4), st),
                  checked(lib.wn_perlin_turb_grad_grid, p._h, C.byref(gt), 7, nm._ptr(out4), st), vol, "samples")
    # the generic gradient kernel at the same step (den 512) on rows too narrow for the run form
    gg = wn.GridSpec(n, 120, 2048, 0, 546).c()
    gen = report("turb7_grid_120x2048x546_generic_gradient",
                 checked(lib.wn_perlin_turb_grad_grid, p._h, C.byref(gg), 7, nm._ptr(out4), st), gvol, "samples")
    print(json.dumps({"name": "turb7_run_form_over_generic_per_sample",
                      "ratio": round((run["sustained_us"] / vol) / (gen["sustained_us"] / gvol), 3)}), flush=True)
    del out4
    torch.cuda.empty_cache()

    npts = 1 << 24
    rng = np.random.default_rng(1)
    pts = torch.from_numpy(rng.uniform(-300.0, 300.0, (npts, 3)).astype(np.float32)).cuda()
    o1 = torch.empty(npts, dtype=torch.float64, device="cuda")
    o4 = torch.empty((npts, 4), dtype=torch.float64, device="cuda")
    pair("perlin_points_16M_random", checked(lib.wn_perlin_points_vec3, p._h, nm._ptr(pts), npts, nm._ptr(o1), st),
         checked(lib.wn_perlin_grad_points_vec3, p._h, nm._ptr(pts), npts, nm._ptr(o4), st), npts, "points")
    pair("turb7_points_16M_random", checked(lib.wn_perlin_turb_points, p._h, nm._ptr(pts), npts, 7, nm._ptr(o1), st),
         checked(lib.wn_perlin_turb_grad_points, p._h, nm._ptr(pts), npts, 7, nm._ptr(o4), st), npts, "points")
    torch.cuda.synchronize()
    print(json.dumps({"name": "device", **wn.device_info(), "time": time.strftime("%Y-%m-%d")}), flush=True)


if __name__ == "__main__":
    main()
