"""HIP-event timing (wn_timer) of curl noise on a 2-D tile and of fused particle advection through it
(csrc/wn_wavelet_curl2d.hip) on one MI355X.

Workloads: tile 128 (seed 12345), unit weights, first_band 0, s = -16 (every band runs), 1 and 5 bands.
    advect_<method>_<nb>[_sorted]   wn_multiband2d_curl_advect_points, 16 M particles uniform in a 128-cell box, 16 steps of
                                    h = 0.001, out of place (every call starts from the same list); _sorted: the same list
                                    sorted by cell, to show whether the order still matters
    unfused_<method>_<nb>[_sorted]  the yardstick: the 16 * stages wn_multiband2d_grad_points launches the call replaces
                                    (64 for RK4, 32 for midpoint, 16 for Euler) on that list, back to back; the float32
                                    passes between them are NOT counted
    launch_<method>_<nb>            one launch: wn_advect2d_launch_steps(method, nb) steps on the uniform list
    curl_points_<nb> / grad_points_<nb>   wn_multiband2d_curl_points against wn_multiband2d_grad_points on that list
    curl_grid_<nb> / grad_grid_<nb>       wn_multiband2d_curl_grid against wn_multiband2d_grad_grid on 4096 x 4096, p = (i/4096)*4
    sweep_points_2^e / sweep_advect_2^e   curl_points_5 / wn_advect2d_launch_steps(RK4, 5) RK4 steps through five bands in the
                                          default build (3: 60 band evaluations) on the first 2^e points, e = 0, 4, 8, 10,
                                          12 .. 24
    --gather DIR    a build with both point thresholds past every list: the global-gather form serves every point list
    --lds DIR       a build with -DWN_CURL2D_POINTS_LDS_MIN_POINTS=0 -DWN_ADVECT2D_LDS_MIN_POINTS=0: every list stages the tile
    --wg1 DIR       a build with -DWN_CURL2D_WORKGROUPS_PER_CU=1: one workgroup of 1024 lanes per CU, 128 VGPRs a lane
    --wg512 DIR     a build with -DWN_CURL2D_WORKGROUP=512: two workgroups of 512 lanes per CU
    --caps DIR,...  builds with -DWN_ADVECT2D_LAUNCH_EVALS=<n>, in directories named evals<n>: their launch_* rows only

    python profiles/curl2d_timing.py [--gather DIR] [--lds DIR] [--wg1 DIR] [--wg512 DIR] [--caps DIR,...] [--rounds 2] [--quick]
                                     [--out profiles/curl2d_kernels.txt]
    (a variant build: make -C <copy of the package> EXTRA_HIPFLAGS=-DWN_CURL2D_WORKGROUPS_PER_CU=1)

The driver runs every tree's measurements as a child process under its own `timeout`, `--rounds` times in alternation,
stops at the first child that fails, and writes the children's JSON lines and a summary to --out.  Per-launch time: the
mean of 10 single calls, each between its own two events.  Sustained: back-to-back calls for at least 0.35 s between two
events, divided by their number.  The summary takes each measurement's median over the rounds and reports the spread
(max - min) beside it:
    bar_*                   fused <= 1.0 x its yardstick, both timed in this tree in the same run
    sorted_over_uniform_*   the cell-sorted list against the uniform one
    wg1_over_shipped_* / wg512_over_shipped_*   the alternative workgroup shapes against the shipped one
    crossover_points / crossover_advect   the smallest swept length from which on the --lds build beats the --gather build
    longest_launch_us       the largest launch_* (mean of single calls), of this tree and of every --caps build"""
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
STEPS = 16
LIMIT = 420   # seconds allowed per child
SWEEP = (0, 4, 8, 10) + tuple(range(12, 25))
METHODS = {"euler": (0, 1), "midpoint": (1, 2), "rk4": (2, 4)}   # name -> (WN_ADVECT_*, stages)
ADVECT = "a_rk4_1,a_rk4_5,a_midpoint_5,a_euler_5,as_rk4_1,as_rk4_5"
SHAPE = ADVECT + ",cp1,cp5,cg1,cg5"
YARD = "u_rk4_1,u_rk4_5,u_midpoint_5,u_euler_5,us_rk4_1,us_rk4_5,gp1,gp5,gg1,gg5"
LAUNCH = ",".join(f"l_{m}_{nb}" for m in METHODS for nb in (1, 5))


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
    uniform = torch.rand((npts, 2), dtype=torch.float32, device="cuda", generator=torch.Generator("cuda").manual_seed(1)) * 128.0
    cell = torch.floor(uniform[:, 1]).to(torch.int64) * 128 + torch.floor(uniform[:, 0]).to(torch.int64)
    by_cell = uniform[torch.argsort(cell)].contiguous()
    out = torch.empty(3 * max(side * side, npts), dtype=torch.float32, device="cuda")
    ones = (C.c_float * 8)(*([1.0] * 8))
    check, ptr = nm.check, nm._ptr

    def advect(pts, method, nb, n=npts, steps=STEPS):
        a = nm._capi.wn_advect2d(METHODS[method][0], steps, 0.001, 1.0, (C.c_float * 2)(0.0, 0.0), 0)
        fn = lib.wn_multiband2d_curl_advect_points
        return lambda: check(fn(h, ptr(pts), n, -16.0, 0, nb, ones, 0.19686, C.byref(a), ptr(out), None, st))

    def unfused(pts, method, nb):
        fn, count = lib.wn_multiband2d_grad_points, STEPS * METHODS[method][1]

        def launch():
            for _ in range(count):
                check(fn(h, ptr(pts), npts, -16.0, 0, nb, ones, 0.19686, ptr(out), st))
        return launch

    def points(name, nb, n=npts):
        fn = getattr(lib, name)
        return lambda: check(fn(h, ptr(uniform), n, -16.0, 0, nb, ones, 0.19686, ptr(out), st))

    def grid(name, nb):
        fn, gc = getattr(lib, name), nm.GridSpec(side, side, side).c()
        return lambda: check(fn(h, C.byref(gc), -16.0, 0, nb, ones, 0.19686, ptr(out), st))

    def make(key):
        kind, *rest = key.split("_")
        if kind in ("a", "as", "u", "us"):
            method, nb = rest[0], int(rest[1])
            pts = by_cell if kind.endswith("s") else uniform
            label = ("advect_" if kind[0] == "a" else "unfused_") + f"{method}_{nb}" + ("_sorted" if kind.endswith("s") else "")
            return label, npts, (advect if kind[0] == "a" else unfused)(pts, method, nb)
        if kind == "l":
            method, nb = rest[0], int(rest[1])
            steps = lib.wn_advect2d_launch_steps(METHODS[method][0], nb)
            return f"launch_{method}_{nb}", npts, advect(uniform, method, nb, steps=steps)
        nb = int(key[2:])
        name = {"cp": "wn_multiband2d_curl_points", "gp": "wn_multiband2d_grad_points", "cg": "wn_multiband2d_curl_grid",
                "gg": "wn_multiband2d_grad_grid"}[key[:2]]
        label = name[len("wn_multiband2d_"):] + f"_{nb}"
        return (label, side * side, grid(name, nb)) if "grid" in name else (label, npts, points(name, nb))

    jobs = []
    for key in which.split(","):
        if key == "sweep":
            steps = 3   # one launch of the default build; a build with a larger cap runs the same steps in one launch too
            for e in SWEEP:
                n = min(1 << e, npts)
                jobs.append((f"sweep_points_2^{e}", n, points("wn_multiband2d_curl_points", 5, n)))
                jobs.append((f"sweep_advect_2^{e}", n, advect(uniform, "rk4", 5, n, steps)))
        else:
            jobs.append(make(key))
    for label, n, launch in jobs:
        mean, best, sustained, k, window = measure(wn, np, torch, launch)
        print(json.dumps({"name": label, "tree": os.path.relpath(root, ROOT), "samples": n, "launch_us_mean": round(mean, 1),
                          "launch_us_min": round(best, 1), "sustained_us": round(sustained, 1), "sustained_launches": k,
                          "sustained_window_s": round(window, 3)}), flush=True)
    torch.cuda.synchronize()
    print(json.dumps({"name": "device", **wn.device_info(), "time": time.strftime("%Y-%m-%d"),
                      "launch_steps_rk4_5": lib.wn_advect2d_launch_steps(2, 5)}), flush=True)


def main():
    out = arg("--out", os.path.join(ROOT, "profiles", "curl2d_kernels.txt"))
    rounds = int(arg("--rounds", "2"))
    plan = [(ROOT, SHAPE + "," + YARD + "," + LAUNCH + ",sweep", "")]
    for flag, which, suffix in (("--gather", "sweep", "_gather"), ("--lds", "sweep", "_lds"), ("--wg1", SHAPE + ",l_rk4_5", "_wg1"),
                                ("--wg512", SHAPE + ",l_rk4_5", "_wg512")):
        if arg(flag):
            plan.append((os.path.abspath(arg(flag)), which, suffix))
    for d in filter(None, arg("--caps", "").split(",")):
        plan.append((os.path.abspath(d), LAUNCH, "_" + os.path.basename(os.path.normpath(d))))
    text = ["Curl noise on a 2-D tile and fused advection (csrc/wn_wavelet_curl2d.hip) on one MI355X: "
            "python profiles/curl2d_timing.py" + (" --quick" if QUICK else ""),
            "(HIP events on the launch stream; microseconds per call; see the script's docstring)", ""]
    seen, single, rc = {}, {}, 0
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
                    single.setdefault(d["name"] + suffix, []).append(d["launch_us_mean"])
        if rc:
            break
    if not rc:
        med = {k: sorted(v)[len(v) // 2] for k, v in seen.items()}
        spread = {k: round(max(v) - min(v), 1) for k, v in seen.items()}
        summary = {"name": "summary", "median_sustained_us": med, "spread_us": spread}
        for name in [k for k in med if k.startswith("advect_") and "_wg" not in k]:
            yard = "unfused_" + name[len("advect_"):]
            if yard in med:
                summary[f"fused_over_unfused_{name}"] = round(med[name] / med[yard], 4)
                summary[f"bar_{name}"] = bool(med[name] <= 1.0 * med[yard])
                summary[f"Gsteps_per_s_{name}"] = round(NPTS * STEPS / med[name] / 1e3, 2) if not QUICK else None
            if name.endswith("_sorted"):
                summary[f"sorted_over_uniform_{name[:-7]}"] = round(med[name] / med[name[:-7]], 4)
        for kind in ("points", "grid"):
            for nb in (1, 5):
                summary[f"curl_over_grad_{kind}_{nb}"] = round(med[f"curl_{kind}_{nb}"] / med[f"grad_{kind}_{nb}"], 4)
                summary[f"bar_curl_{kind}_{nb}"] = bool(med[f"curl_{kind}_{nb}"] <= 1.0 * med[f"grad_{kind}_{nb}"])
        for suffix in ("_wg1", "_wg512"):
            for k in [k for k in med if k.endswith(suffix)]:
                summary[f"{suffix[1:]}_over_shipped_{k[:-len(suffix)]}"] = round(med[k] / med[k[:-len(suffix)]], 4)
        launches = {k: sorted(v)[len(v) // 2] for k, v in single.items() if k.startswith("launch_") and "_wg" not in k}
        summary["single_launch_us_mean"] = launches
        summary["longest_launch_us"] = max(v for k, v in launches.items() if "_evals" not in k)
        for cap in sorted({k[k.index("_evals") + 1:] for k in launches if "_evals" in k}):
            summary[f"longest_launch_us_{cap}"] = max(v for k, v in launches.items() if k.endswith("_" + cap))
        for kind in ("points", "advect"):
            sizes = [e for e in SWEEP if f"sweep_{kind}_2^{e}_lds" in med and f"sweep_{kind}_2^{e}_gather" in med]
            if sizes:
                wins = [med[f"sweep_{kind}_2^{e}_lds"] < med[f"sweep_{kind}_2^{e}_gather"] for e in sizes]
                first = next((e for i, e in enumerate(sizes) if all(wins[i:])), None)
                summary[f"crossover_{kind}"] = f"2^{first}" if first is not None else "none: the gather build wins at the longest list"
                summary[f"lds_over_gather_{kind}"] = {f"2^{e}": round(med[f"sweep_{kind}_2^{e}_lds"] / med[f"sweep_{kind}_2^{e}_gather"], 3)
                                                      for e in sizes}
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
