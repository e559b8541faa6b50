"""HIP-event timing (wn_timer) of WMultibandNoise with a footprint per point (csrc/wn_wavelet_footprint.hip) on one MI355X.

Workload: 16 M points uniform in [-10, 10]^3 (the box of bench.py's texture stand-in), tile 128 (seed 12345), five unit
weights, first_band 0, footprints s uniform on [-5.5, 0.5): the band counts 0 .. 5 are about evenly mixed.

    (a) footprint          wn_multiband3d_footprint_points (hard cut), the list as drawn
    (b) uniform_5_bands    wn_multiband3d_points at s = -16 (all five bands) on the same points -- what a caller pays who
                           does not limit the bands at all; timed in this tree and, with --parent DIR, in a built checkout
                           of the parent commit (the yardstick: this change does not touch that entry point)
    (d) footprint_sorted_s (a) with s sorted ascending: every wave's lanes run the same number of bands

    python profiles/footprint_timing.py [--parent DIR] [--rounds 2] [--quick] [--out profiles/footprint_kernels.txt]

The driver runs every measurement as a child process under its own `timeout`, `--rounds` times in alternation (this tree,
parent, this tree, ...), stops at the first child that fails, and writes the children's JSON lines and a summary
to --out.  Per-launch time: the mean of 10 single calls, each between its own two events.  Sustained: back-to-back calls for
at least 0.3 s between two events, divided by their number.  The summary takes each measurement's median over the rounds and
reports the spread (max - min) beside it:
    bar                 (a) <= (b) at the parent commit: limiting the bands must cost no more than not limiting them
    distance_from_ideal (a) / ((b) * mean active bands / 5)
    divergence_cost     (a) / (d): what lanes of unequal band counts in one wave cost"""
import ctypes as C
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUICK = "--quick" in sys.argv
NPTS = 1 << 24
LIMIT = 300   # seconds allowed per child


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def measure(wn, np, torch, launch, launches=10, sustain_s=0.35):
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
    k = max(1, int(sustain_s * 1e6 / max(np.median(per), 1.0)) + 1)
    if QUICK:
        k = min(k, 5)
    t.start()
    for _ in range(k):
        launch()
    t.stop()
    total_us = t.elapsed_ms() * 1e3
    return float(np.mean(per)), float(np.min(per)), total_us / k, k, total_us * 1e-6


def child(root, which):
    """Time the measurements `which` (a comma list of a, b, d) with the package of the tree at `root`."""
    sys.path.insert(0, root)
    import numpy as np
    import torch
    wn = importlib.import_module("wavelet-noise-in-ray-tracing_amd")
    nm = importlib.import_module("wavelet-noise-in-ray-tracing_amd.noise")
    torch.cuda.set_device(0)
    lib, st = nm._lib, nm._stream()
    npts = NPTS >> 6 if QUICK else NPTS
    rng = np.random.default_rng(1)
    pts = torch.from_numpy(rng.uniform(-10.0, 10.0, (npts, 3)).astype(np.float32)).cuda()
    s_host = rng.uniform(-5.5, 0.5, npts).astype(np.float32)
    bands = sum(((s_host + np.float32(0)) + np.float32(b) < 0).astype(np.int64) for b in range(5))
    mean_bands = float(bands.mean())
    noise = wn.WaveletNoise(128, 12345)
    noise.generateNoiseTile3D()
    h = noise._handle(3)
    out = torch.empty(npts, dtype=torch.float32, device="cuda")
    w5 = (C.c_float * 5)(*[1.0] * 5)

    def footprint(s):
        def launch():
            nm.check(lib.wn_multiband3d_footprint_points(h, nm._ptr(pts), nm._ptr(s), npts, 0, 5, w5, 0.18402, 0, nm._ptr(out), st))
        return launch

    def uniform():
        nm.check(lib.wn_multiband3d_points(h, nm._ptr(pts), npts, -16.0, 0, 5, w5, 0.18402, nm._ptr(out), st))

    for key in which.split(","):
        if key == "b":
            label, launch = "uniform_5_bands", uniform
        elif key == "d":
            label, launch = "footprint_sorted_s", footprint(torch.from_numpy(np.sort(s_host)).cuda())
        else:
            label, launch = "footprint", footprint(torch.from_numpy(s_host).cuda())
        mean, best, sustained, k, window = measure(wn, np, torch, launch)
        print(json.dumps({"name": label, "tree": os.path.relpath(root, ROOT), "points": npts, "mean_active_bands": round(mean_bands, 4),
                          "launch_us_mean": round(mean, 1), "launch_us_min": round(best, 1), "sustained_us": round(sustained, 1),
                          "sustained_launches": k, "sustained_window_s": round(window, 3),
                          "G_points_per_s": round(npts / sustained / 1e3, 3)}), flush=True)
    torch.cuda.synchronize()
    print(json.dumps({"name": "device", **wn.device_info(), "time": time.strftime("%Y-%m-%d")}), flush=True)


def main():
    out = arg("--out", os.path.join(ROOT, "profiles", "footprint_kernels.txt"))
    parent, rounds = arg("--parent"), int(arg("--rounds", "2"))
    plan = [(ROOT, "a,b,d", "")]
    if parent:
        plan.append((os.path.abspath(parent), "b", "_parent"))
    text = ["WMultibandNoise with a footprint per point (csrc/wn_wavelet_footprint.hip) on one MI355X: "
            "python profiles/footprint_timing.py" + (" --quick" if QUICK else ""),
            "(HIP events on the launch stream; microseconds per call of 16 M points; see the script's docstring)", ""]
    seen, rc = {}, 0
    for r in range(rounds):
        for root, which, suffix in plan:
            cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--child", root, which]
            res = subprocess.run(cmd + (["--quick"] if QUICK else []), cwd=ROOT, capture_output=True, text=True)
            print(res.stdout, end="", flush=True)
            text += [f"[round {r}: {os.path.relpath(root, ROOT)} {which}]"] + res.stdout.splitlines() + [""]
            if res.returncode != 0:   # nothing more runs on the device after a failed child
                print(res.stderr[-3000:], file=sys.stderr)
                text += [f"the child failed with exit status {res.returncode}; nothing more was run"]
                rc = 1
                break
            for ln in res.stdout.splitlines():
                d = json.loads(ln)
                if "sustained_us" in d:
                    seen.setdefault(d["name"] + suffix, []).append(d["sustained_us"])
                    seen["mean_active_bands"] = d["mean_active_bands"]
        if rc:
            break
    if not rc:
        med = {k: sorted(v)[len(v) // 2] for k, v in seen.items() if isinstance(v, list)}
        summary = {"name": "summary", "median_sustained_us": med,
                   "spread_us": {k: round(max(v) - min(v), 1) for k, v in seen.items() if isinstance(v, list)},
                   "mean_active_bands": seen.get("mean_active_bands")}
        a, b_here, b = med.get("footprint"), med.get("uniform_5_bands"), med.get("uniform_5_bands_parent")
        yard = b if b is not None else b_here
        summary["yardstick"] = "uniform_5_bands at the parent commit" if b is not None else "uniform_5_bands in this tree (no --parent)"
        summary["bar_a_le_b"] = bool(a <= yard)
        summary["a_over_b"] = round(a / yard, 4)
        summary["distance_from_ideal"] = round(a / (yard * seen["mean_active_bands"] / 5.0), 4)
        summary["divergence_cost_a_over_d"] = round(a / med["footprint_sorted_s"], 4)
        print(json.dumps(summary), flush=True)
        text += ["[summary]", json.dumps(summary), ""]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(text) + "\n")
    return rc


if __name__ == "__main__":
    if "--child" in sys.argv:
        i = sys.argv.index("--child")
        child(sys.argv[i + 1], sys.argv[i + 2])
    else:
        sys.exit(main())
