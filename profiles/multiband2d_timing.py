"""HIP-event timing (wn_timer) of WMultibandNoise on a 2-D tile (csrc/wn_wavelet_multiband2d.hip) on one MI355X.

Workloads: tile 128 (seed 12345), unit weights, first_band 0, s = -16 (every band runs).
    grid_1 / grid_5 / grad_grid_1 / grad_grid_5   wn_multiband2d_grid / _grad_grid on the 4096 x 4096 lattice p = (i/4096)*4
                                                  with 1 and 5 bands
    points_5 / grad_points_5                      wn_multiband2d_points / _grad_points, 16 M points uniform in [-10, 10]^2
    footprint_points_5                            wn_multiband2d_footprint_points, s uniform on [-5.5, 0.5) (information)
    sweep_2^e                                     points_5 on the first 2^e points, e = 12 .. 24
    fill_1 / fill_3                               torch's zero_ of 4096^2 floats (x 3): the store floor, at the fill rate
                                                  bench.py reports
    unfused_*                                     the yardstick: what a caller pays without these entry points -- the nbands
                                                  launches of wn_eval2d_grid / wn_eval2d_grad_grid / wn_eval2d_points /
                                                  wn_eval2d_grad_points on the bands' lattices (octave_scale 2^b, post_scale
                                                  2), back to back, their accumulation passes NOT counted; timed in this
                                                  tree and, with --parent DIR, in a built checkout of the parent commit
    --gather DIR                                  a build of this tree with -DWN_MB2D_LDS_TILE_MAX_BYTES=0: no tile is staged
                                                  in LDS, the global-gather form serves grids and point lists
    --wg512 DIR                                   a build with -DWN_MB2D_WORKGROUP=512: the alternative workgroup size
    --points-lds DIR                              a build with -DWN_MB2D_POINTS_LDS_MIN_POINTS=0: every point list stages the
                                                  tile in LDS (the sweep, for the crossover against --gather)

    python profiles/multiband2d_timing.py [--parent DIR] [--gather DIR] [--wg512 DIR] [--points-lds DIR] [--rounds 2] [--quick]
                                          [--out profiles/multiband2d_kernels.txt]
    (a variant build: make -C <copy of the package> EXTRA_HIPFLAGS=-DWN_MB2D_WORKGROUP=512)

The driver runs every tree's measurements as a child process under its own `timeout`, `--rounds` times in alternation,
stops at the first child that fails, and writes the children's JSON lines and a summary to --out.  Per-launch time: the
mean of 10 single calls, each between its own two events.  Sustained: back-to-back calls for at least 0.35 s between two
events, divided by their number.  The summary takes each measurement's median over the rounds and reports the spread
(max - min) beside it:
    bar_*               fused <= 1.0 x unfused_* at the parent commit: fusing must not cost more than not fusing
    lds_gain_us_*       gather build - this build; ship_lds_*: the gain exceeds the sum of the two spreads
    wg512_over_wg1024_* the alternative workgroup size against the shipped one
    over_store_floor_*  fused / fill_1 (gradients: fill_3)
    points_crossover    the smallest swept length from which on the --points-lds build is faster than the --gather build"""
import ctypes as C
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUICK = "--quick" in sys.argv
SIDE = 4096
NPTS = 1 << 24
LIMIT = 300   # seconds allowed per child
FUSED = "g1,g5,gg1,gg5,p5,pg5"


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
    while True:   # back-to-back launches are shorter than single ones: repeat with more until the window is reached
        t.start()
        for _ in range(k):
            launch()
        t.stop()
        total_us = t.elapsed_ms() * 1e3
        if QUICK or total_us >= sustain_s * 1e6:
            break
        k = int(k * sustain_s * 1e6 / max(total_us, 1.0) * 1.05) + 1
    return float(np.mean(per)), float(np.min(per)), total_us / k, k, total_us * 1e-6


def child(root, which):
    """Time the measurements `which` (a comma list of the keys below) with the package of the tree at `root`."""
    sys.path.insert(0, root)
    import numpy as np
    import torch
    wn = importlib.import_module("wavelet-noise-in-ray-tracing_amd")
    nm = importlib.import_module("wavelet-noise-in-ray-tracing_amd.noise")
    torch.cuda.set_device(0)
    lib, st = nm._lib, nm._stream()
    side = SIDE >> 3 if QUICK else SIDE
    npts = NPTS >> 6 if QUICK else NPTS
    noise = wn.WaveletNoise(128, 12345)
    noise.generateNoiseTile2D()
    h = noise._handle(2)
    rng = np.random.default_rng(1)
    pts = torch.from_numpy(rng.uniform(-10.0, 10.0, (npts, 2)).astype(np.float32)).cuda()
    s_mixed = torch.from_numpy(rng.uniform(-5.5, 0.5, npts).astype(np.float32)).cuda()
    out = torch.empty(3 * max(side * side, npts), dtype=torch.float32, device="cuda")
    ones = (C.c_float * 8)(*([1.0] * 8))
    check, ptr = nm.check, nm._ptr

    def fused_grid(name, nb):
        fn, gc = getattr(lib, name), nm.GridSpec(side, side, side).c()
        return lambda: check(fn(h, C.byref(gc), -16.0, 0, nb, ones, 0.19686, ptr(out), st))

    def unfused_grid(name, nb):
        fn = getattr(lib, name)
        gcs = [nm.GridSpec(side, side, side, octave_scale=float(2.0 ** b), post_scale=2.0).c() for b in range(nb)]

        def launch():
            for gc in gcs:
                check(fn(h, C.byref(gc), ptr(out), st))
        return launch

    def fused_points(name, n):
        fn = getattr(lib, name)
        return lambda: check(fn(h, ptr(pts), n, -16.0, 0, 5, ones, 0.19686, ptr(out), st))

    def footprint_points():
        fn = lib.wn_multiband2d_footprint_points
        return lambda: check(fn(h, ptr(pts), ptr(s_mixed), npts, 0, 5, ones, 0.19686, 0, ptr(out), st))

    def unfused_points(name):
        fn = getattr(lib, name)

        def launch():   # the five launches a caller makes (on the same list: scaling it per band is not counted either)
            for _ in range(5):
                check(fn(h, ptr(pts), npts, ptr(out), st))
        return launch

    def fill(planes):
        view = out[:planes * side * side]
        return lambda: view.zero_()

    table = {
        "g1": ("grid_1", lambda: fused_grid("wn_multiband2d_grid", 1)), "g5": ("grid_5", lambda: fused_grid("wn_multiband2d_grid", 5)),
        "gg1": ("grad_grid_1", lambda: fused_grid("wn_multiband2d_grad_grid", 1)),
        "gg5": ("grad_grid_5", lambda: fused_grid("wn_multiband2d_grad_grid", 5)),
        "p5": ("points_5", lambda: fused_points("wn_multiband2d_points", npts)),
        "pg5": ("grad_points_5", lambda: fused_points("wn_multiband2d_grad_points", npts)),
        "fp5": ("footprint_points_5", footprint_points),
        "f1": ("fill_1", lambda: fill(1)), "f3": ("fill_3", lambda: fill(3)),
        "u1": ("unfused_grid_1", lambda: unfused_grid("wn_eval2d_grid", 1)), "u5": ("unfused_grid_5", lambda: unfused_grid("wn_eval2d_grid", 5)),
        "ug1": ("unfused_grad_grid_1", lambda: unfused_grid("wn_eval2d_grad_grid", 1)),
        "ug5": ("unfused_grad_grid_5", lambda: unfused_grid("wn_eval2d_grad_grid", 5)),
        "up5": ("unfused_points_5", lambda: unfused_points("wn_eval2d_points")),
        "upg5": ("unfused_grad_points_5", lambda: unfused_points("wn_eval2d_grad_points")),
    }
    jobs = []
    for key in which.split(","):
        if key == "sweep":
            for e in range(12, 25):
                n = min(1 << e, npts)
                jobs.append((f"sweep_2^{e}", n, fused_points("wn_multiband2d_points", n)))
        else:
            label, make = table[key]
            jobs.append((label, npts if "points" in label else side * side, make()))
    for label, n, launch in jobs:
        mean, best, sustained, k, window = measure(wn, np, torch, launch)
        print(json.dumps({"name": label, "tree": os.path.relpath(root, ROOT), "samples": n, "launch_us_mean": round(mean, 1),
                          "launch_us_min": round(best, 1), "sustained_us": round(sustained, 1), "sustained_launches": k,
                          "sustained_window_s": round(window, 3)}), flush=True)
    torch.cuda.synchronize()
    print(json.dumps({"name": "device", **wn.device_info(), "time": time.strftime("%Y-%m-%d")}), flush=True)


def main():
    out = arg("--out", os.path.join(ROOT, "profiles", "multiband2d_kernels.txt"))
    rounds = int(arg("--rounds", "2"))
    yard = "u1,u5,ug1,ug5,up5,upg5"
    plan = [(ROOT, FUSED + ",fp5,f1,f3,sweep," + yard, "")]
    for flag, which, suffix in (("--parent", yard, "_parent"), ("--gather", FUSED + ",sweep", "_gather"), ("--wg512", FUSED, "_wg512"),
                                ("--points-lds", "sweep", "_plds")):
        if arg(flag):
            plan.append((os.path.abspath(arg(flag)), which, suffix))
    text = ["WMultibandNoise on a 2-D tile (csrc/wn_wavelet_multiband2d.hip) on one MI355X: "
            "python profiles/multiband2d_timing.py" + (" --quick" if QUICK else ""),
            "(HIP events on the launch stream; microseconds per call; see the script's docstring)", ""]
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
        if rc:
            break
    if not rc:
        med = {k: sorted(v)[len(v) // 2] for k, v in seen.items()}
        spread = {k: round(max(v) - min(v), 1) for k, v in seen.items()}
        summary = {"name": "summary", "median_sustained_us": med, "spread_us": spread,
                   "yardstick": "the parent commit" if "unfused_grid_5_parent" in med else "this tree (no --parent)"}
        for name in ("grid_1", "grid_5", "grad_grid_1", "grad_grid_5", "points_5", "grad_points_5"):
            yardstick = med.get(f"unfused_{name}_parent", med[f"unfused_{name}"])
            summary[f"fused_over_unfused_{name}"] = round(med[name] / yardstick, 4)
            summary[f"bar_{name}"] = bool(med[name] <= 1.0 * yardstick)
            if "grid" in name:
                summary[f"over_store_floor_{name}"] = round(med[name] / med["fill_3" if "grad" in name else "fill_1"], 3)
            if f"{name}_gather" in med:
                gain = med[f"{name}_gather"] - med[name]
                summary[f"lds_gain_us_{name}"] = round(gain, 1)
                summary[f"ship_lds_{name}"] = bool(gain > spread[name] + spread[f"{name}_gather"])
            if f"{name}_wg512" in med:
                summary[f"wg512_over_wg1024_{name}"] = round(med[f"{name}_wg512"] / med[name], 4)
        summary["fill_GBps"] = round(SIDE * SIDE * 4 / med["fill_1"] / 1e3, 1) if not QUICK else None
        sizes = [e for e in range(12, 25) if f"sweep_2^{e}_plds" in med and f"sweep_2^{e}_gather" in med]
        if sizes:
            wins = [med[f"sweep_2^{e}_plds"] < med[f"sweep_2^{e}_gather"] for e in sizes]
            first = next((e for i, e in enumerate(sizes) if all(wins[i:])), None)
            summary["points_crossover"] = f"2^{first}" if first is not None else "none: the gather build wins at the longest list"
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
