"""HIP-event timing (wn_timer) of the Perlin brick-list kernels (csrc/wn_perlin_bricks.hip, include/wnoise_perlin_bricks.h) on
one MI355X, in the manner of profiles/bricks_timing.py: the 512^3 lattice at den 512 -- noise at octave 4 (step 1/8 cell),
turb(7) and fractal_noise at octave 0 (step 1/128; the octaves reach 1/2 and 1/4) -- each of the seven calls beside its two
yardsticks:

    points   the matching point entry (wn_perlin_points_vec3, _turb_points, _fractal_points, their _grad_ forms,
             wn_perlin_curl_points_vec3) on exactly the same samples (512 float coordinates per brick): the call a
             sparse-volume holder makes without the brick entry points.  BAR: the brick call takes no more than 1.0 x this, on
             every list.
    dense    the matching dense grid entry point on the whole 512^3 box: the ratio -- the break-even fill fraction -- and
             the per-sample time on the full list against it are reported, no bar.

The lists are those of profiles/bricks_timing.py: all 262,144 bricks in raster order; a uniform random 10 % in random order;
the bricks cut by the surface of the sphere of radius 200 samples about the centre.  The curl uses the default offsets and
turb(7) potentials.

    python profiles/perlin_bricks_timing.py [--quick] [--out profiles/perlin_bricks_kernels.txt]

The driver runs every step as a child process under its own `timeout`, stops at the first step that fails, and writes the
steps' JSON lines to --out.  Per-launch time: 20 single calls after 3 warm-up launches, each between its own two events;
sustained: back-to-back calls for about 0.4 s between two events, divided by their number.  The brick call and the point
entry are timed alternately, ROUNDS times each in the same process; the ratio is reported per round, with its spread."""
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

# step: (field, kind, depth, octave, seconds allowed)
STEPS = {"noise": ("value", 0, 0, 4, 300), "turb7": ("value", 1, 7, 0, 300), "fractal": ("value", 2, 0, 0, 300),
         "noise_grad": ("grad", 0, 0, 4, 300), "turb7_grad": ("grad", 1, 7, 0, 300), "fractal_grad": ("grad", 2, 0, 0, 300),
         "turb7_curl": ("curl", 1, 7, 0, 300)}
QUICK = "--quick" in sys.argv
ROUNDS = 3
N = bt.N


def step(name):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    wn = importlib.import_module("wavelet-noise-in-ray-tracing_amd")
    nm = importlib.import_module("wavelet-noise-in-ray-tracing_amd.noise")
    torch.cuda.set_device(0)
    lib, st = nm._lib, nm._stream()
    field, kind, depth, octave, _ = STEPS[name]
    ch = {"value": 1, "grad": 4, "curl": 3}[field]
    bt.QUICK = QUICK

    def report(label, launch, **extra):
        mean, best, worst, sustained, k = bt.measure(wn, np, torch, launch)
        line = {"name": label, "launch_us_mean": round(mean, 2), "launch_us_min": round(best, 2), "launch_us_max": round(worst, 2),
                "sustained_us": round(sustained, 2), "sustained_launches": k, **extra}
        print(json.dumps(line), flush=True)
        return line

    p = wn.perlin(12345)
    off = p._curl_offsets(None)
    stem = "wn_perlin_" + ("", "turb_", "fractal_")[kind] + ("grad_" if field == "grad" else "")
    if field == "curl":
        f_grid, f_points, f_bricks = lib.wn_perlin_curl_grid, lib.wn_perlin_curl_points_vec3, lib.wn_perlin_curl_bricks
        g_mid = p_mid = (kind, depth, off)
    else:
        f_grid, f_bricks = getattr(lib, stem + "grid"), getattr(lib, stem + "bricks")
        f_points = getattr(lib, stem + ("points_vec3" if kind == 0 else "points"))
        g_mid = p_mid = (depth,) if kind == 1 else ()
    gc = wn.GridSpec(N, N, N, 0, N, octave_scale=nm._octave_scale(octave)).c()

    dense_out = torch.empty(ch * N ** 3, dtype=torch.float32, device="cuda")

    def launch_dense():
        nm.check(f_grid(p._h, C.byref(gc), *g_mid, nm._ptr(dense_out), st))
    dense = report(f"dense_512^3_{name}", launch_dense, samples=N ** 3)
    del dense_out

    local = torch.arange(512, device="cuda")
    offs = torch.stack([local & 7, (local >> 3) & 7, local >> 6], -1)                   # (512, 3): lx, ly, lz
    for lname, host_list in bt.brick_lists(np).items():
        n = len(host_list)
        bricks = torch.from_numpy(host_list).cuda()
        out = torch.empty(ch * n * 512, dtype=torch.float32, device="cuda")
        out64 = torch.empty(ch * n * 512, dtype=torch.float64, device="cuda")
        # the same samples as a point list: c = (((float)i / den) * 4) * octave_scale per axis
        idx = (bricks[:, None, :] * 8 + offs[None, :, :]).to(torch.float32).reshape(-1, 3)
        pts = (((idx / float(N)) * 4.0) * float(nm._octave_scale(octave))).contiguous()
        del idx

        def launch_points():
            nm.check(f_points(p._h, nm._ptr(pts), n * 512, *p_mid, nm._ptr(out64), st))

        def launch_bricks():
            nm.check(f_bricks(p._h, C.byref(gc), *g_mid, nm._ptr(bricks), n, nm._ptr(out), st))
        ratios, last = [], None
        for r in range(1 if QUICK else ROUNDS):               # alternately: points, bricks, points, bricks, ...
            points = report(f"points_{lname}_{name}_round{r}", launch_points, bricks=n, samples=n * 512)
            last = report(f"bricks_{lname}_{name}_round{r}", launch_bricks, bricks=n, samples=n * 512)
            ratios.append(last["sustained_us"] / points["sustained_us"])
        worst = max(ratios)
        print(json.dumps({"name": f"bricks_{lname}_{name}_ratios",
                          "bricks_over_points_per_round": [round(v, 4) for v in ratios],
                          "bricks_over_points_min": round(min(ratios), 4), "bricks_over_points_max": round(worst, 4),
                          "bar_1.0": "met" if worst <= 1.0 else "MISSED",
                          "bricks_over_dense_512^3": round(last["sustained_us"] / dense["sustained_us"], 4),
                          "ps_per_sample_bricks": round(last["sustained_us"] * 1e6 / (n * 512), 3),
                          "ps_per_sample_dense": round(dense["sustained_us"] * 1e6 / N ** 3, 3)}), flush=True)
        del pts, out, out64, bricks
    torch.cuda.synchronize()
    print(json.dumps({"name": "device", **wn.device_info(), "time": time.strftime("%Y-%m-%d")}), flush=True)


def main():
    out = os.path.join(ROOT, "profiles", "perlin_bricks_kernels.txt")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    text = ["Perlin brick-list kernels (csrc/wn_perlin_bricks.hip) on one MI355X: python profiles/perlin_bricks_timing.py"
            + (" --quick" if QUICK else ""),
            "(HIP events on the launch stream; microseconds; den 512; noise at octave 4, turb(7) and fractal_noise at octave 0;",
            " `points_*` is the point entry on the same samples, `dense_*` the dense grid of the whole 512^3 box; ratios are of",
            " sustained times, points and bricks timed alternately)", ""]
    rc = 0
    for name, spec in STEPS.items():
        cmd = ["timeout", "-k", "10", str(spec[-1]), sys.executable, os.path.abspath(__file__), "--step", name] + (["--quick"] if QUICK else [])
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
