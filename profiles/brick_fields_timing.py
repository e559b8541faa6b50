"""HIP-event timing (wn_timer) of the gradient and curl brick-list kernels (csrc/wn_wavelet_brick_fields.hip,
include/wnoise_brick_fields.h) on one MI355X, in the manner of profiles/bricks_timing.py: the headline lattice (den 512,
tile 128, octave 4; five bands: WMultibandNoise from band 0), each call beside the two yardsticks it stands between, timed
alone in the same run:

    points   wn_eval3d_grad_points / wn_eval3d_curl_points (or their multiband forms) on exactly the same samples (512 float
             coordinates per brick): the call a sparse-volume holder makes without the brick entry points.  BAR: the brick
             call takes no more than 1.0 x this, on every list and in both tiers.
    dense    wn_eval3d_grad_grid / wn_eval3d_curl_grid (or their multiband forms) on the whole 512^3 box, in the same tier:
             the ratio -- the break-even fill fraction -- is reported, no bar.

The lists are those of profiles/bricks_timing.py: all 262,144 bricks in raster order; a uniform random 10 % in random order;
the bricks cut by the surface of the sphere of radius 200 samples about the centre.  The curl uses the default offsets.

    python profiles/brick_fields_timing.py [--quick] [--out profiles/brick_fields_kernels.txt]

The driver runs every step as a child process under its own `timeout`, stops at the first step that fails, and writes the
steps' JSON lines to --out.  Per-launch time: 20 single calls after 3 warm-up launches, each between its own two events;
sustained: back-to-back calls for about 0.4 s between two events, divided by their number; the ratios use it."""
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

STEPS = {"grad_one_band": 300, "grad_five_bands": 300, "curl_one_band": 300, "curl_five_bands": 300}   # seconds allowed
QUICK = "--quick" in sys.argv
N = bt.N


def step(name):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    wn = importlib.import_module("wavelet-noise-in-ray-tracing_amd")
    nm = importlib.import_module("wavelet-noise-in-ray-tracing_amd.noise")
    torch.cuda.set_device(0)
    lib, st = nm._lib, nm._stream()
    kind, bands = name.split("_")[0], {"one": 1, "five": 5}[name.split("_")[1]]
    ch = 4 if kind == "grad" else 3
    bt.QUICK = QUICK

    def report(label, launch, **extra):
        mean, best, worst, sustained, k = bt.measure(wn, np, torch, launch)
        line = {"name": label, "launch_us_mean": round(mean, 2), "launch_us_min": round(best, 2), "launch_us_max": round(worst, 2),
                "sustained_us": round(sustained, 2), "sustained_launches": k, **extra}
        print(json.dumps(line), flush=True)
        return line

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
    lead = (off,) if kind == "curl" else ()
    stem = "wn_eval3d" if bands == 1 else "wn_multiband3d"
    f_grid, f_points, f_bricks = (getattr(lib, f"{stem}_{kind}_{what}") for what in ("grid", "points", "bricks"))

    def grid(flags):
        return wn.GridSpec(N, N, N, 0, N, octave_scale=os_, post_scale=post, out_scale=scale, flags=flags).c()

    tiers = ((nm.WN_GRID_DEFAULT, "default"), (nm.WN_GRID_EXACT, "exact"))
    dense_out = torch.empty(ch * N ** 3, dtype=torch.float32, device="cuda")
    dense = {}
    for flags, tier in tiers:
        gc = grid(flags)

        def launch_dense(gc=gc):
            nm.check(f_grid(h, C.byref(gc), *lead, *mb, nm._ptr(dense_out), st))
        dense[tier] = report(f"dense_512^3_{name}_{tier}", launch_dense, samples=N ** 3)
    del dense_out

    local = torch.arange(512, device="cuda")
    offs = torch.stack([local & 7, (local >> 3) & 7, local >> 6], -1)                   # (512, 3): lx, ly, lz
    for lname, host_list in bt.brick_lists(np).items():
        n = len(host_list)
        bricks = torch.from_numpy(host_list).cuda()
        out = torch.empty(ch * n * 512, dtype=torch.float32, device="cuda")
        # the same samples as a point list: c = (((float)i / den) * 4) * octave_scale * post_scale per axis
        idx = (bricks[:, None, :] * 8 + offs[None, :, :]).to(torch.float32).reshape(-1, 3)
        pts = (((idx / float(N)) * 4.0) * os_) * post
        del idx
        pts = pts.contiguous()

        def launch_points():
            nm.check(f_points(h, nm._ptr(pts), n * 512, *lead, *mb, nm._ptr(out), st))
        points = report(f"points_{lname}_{name}", launch_points, bricks=n, samples=n * 512)
        for flags, tier in tiers:
            gc = grid(flags)

            def launch_bricks(gc=gc):
                nm.check(f_bricks(h, C.byref(gc), nm._ptr(bricks), n, *lead, *mb, nm._ptr(out), st))
            line = report(f"bricks_{lname}_{name}_{tier}", launch_bricks, bricks=n, samples=n * 512)
            ratio = line["sustained_us"] / points["sustained_us"]
            print(json.dumps({"name": f"bricks_{lname}_{name}_{tier}_ratios",
                              "bricks_over_points": round(ratio, 4), "bar_1.0_met": ratio <= 1.0,
                              "bricks_over_dense_512^3": round(line["sustained_us"] / dense[tier]["sustained_us"], 4),
                              "G_samples_per_s": round(n * 512 / line["sustained_us"] * 1e-3, 2)}), flush=True)
        del pts, out, bricks
    torch.cuda.synchronize()
    print(json.dumps({"name": "device", **wn.device_info(), "time": time.strftime("%Y-%m-%d")}), flush=True)


def main():
    out = os.path.join(ROOT, "profiles", "brick_fields_kernels.txt")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    text = ["Gradient and curl brick-list kernels (csrc/wn_wavelet_brick_fields.hip) on one MI355X: python profiles/brick_fields_timing.py"
            + (" --quick" if QUICK else ""),
            "(HIP events on the launch stream; microseconds; den 512, tile 128, octave 4; `points_*` is the point-list call on the",
            " same samples, `dense_*` the dense derivative grid of the whole 512^3 box; ratios are of sustained times)", ""]
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
