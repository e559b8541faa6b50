"""HIP-event timing (wn_timer) of Perlin curl noise with solid boundaries (csrc/wn_perlin_bounded.hip) on one MI355X.

    16 M particles uniform in a 128-cell box, RK4, 16 steps, the default offsets; noise, turb(7), fractal_noise
    bar (a)   every particle NEAR (one container around the box, its ramp as wide as its radius):
              wn_perlin_curl_bounded_advect_points_f64 | the 64 wn_perlin_curl_points(_vec3) launches plus the 64
              wn_perlin_curl_potential_points_f64 / _f32 launches a caller's own loop needs for the same trace, timed ALONE (no
              ramp, no stage arithmetic, which favours the loop); bar: <= 1.0 x.  Also against the 64 curl launches alone:
              what the boundary itself costs.
    bar (b)   nobs == 0 | wn_perlin_curl_advect_points: inside the run-to-run spread (the same kernel through another door)
    no bar    every particle FAR from 1, 3 and 16 obstacles (spheres outside the box); the tests' scene scaled to the box;
              the bounded and potential point entries against wn_perlin_curl_points(_vec3)
    kappa     the cost of one obstacle's ramp in octave evaluations, for kRampKappa: (far from 16 - far from 1) / 15 per
              stage, over the time of one octave evaluation (the unbounded call's time / (16 steps x 4 stages x octaves));
              and the longest launch of each chain

    python profiles/perlin_bounded_timing.py [--quick] [--out profiles/perlin_bounded_kernels.txt]

Every timing alternates with its yardstick: one warm-up call of each, then REPS rounds of (yardstick, call), each between two
events on the launch stream; the mean and the minimum of the rounds.  The driver runs every kind as a child process under
its own `timeout`, stops at the first one that fails, and writes the JSON lines to --out (--quick: 1 M particles)."""
import ctypes as C
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = {"noise": 240, "turb7": 500, "fractal": 500}   # seconds allowed
QUICK = "--quick" in sys.argv
NPTS = 1 << (20 if QUICK else 24)
TRACE_STEPS, STAGES = 16, 4
REPS = 3
BOX = 128.0
LAUNCH_MS_LIMIT = 50.0   # a launch over 16 M particles stays at or below this


def scenes():
    """name -> obstacle tuples, in the coordinates of the box (0, 128)^3."""
    mid, s = BOX / 2, BOX / 600.0      # the tests' scene lives in (-300, 300)^3
    centre = (mid, mid, mid)
    far = [("sphere", (1000.0 + 100.0 * j, -500.0, 0.0), 10.0, 10.0) for j in range(16)]
    return {
        "near": [("container", centre, 200.0, 200.0)],     # the box's corners lie 110.9 from its centre: 89 < d < 200 = d0
        "far1": far[:1], "far3": far[:3], "far16": far,
        "scene": [("sphere", centre, 120.0 * s, 80.0 * s), ("halfspace", (0.0, 1.0, 0.0), mid - 250.0 * s, 100.0 * s),
                  ("container", centre, 500.0 * s, 150.0 * s)],
    }


def step(name):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    wn = importlib.import_module("wavelet-noise-in-ray-tracing_amd")
    nm = importlib.import_module("wavelet-noise-in-ray-tracing_amd.noise")
    capi = nm._capi
    torch.cuda.set_device(0)
    lib = nm._lib
    per = wn.perlin(12345)
    kind, depth, octaves = {"noise": (capi.WN_PERLIN_CURL_NOISE, 0, 1), "turb7": (capi.WN_PERLIN_CURL_TURB, 7, 7),
                            "fractal": (capi.WN_PERLIN_CURL_FRACTAL, 0, 6)}[name]
    h, off, st = per._h, per._curl_offsets(None), nm._stream()
    timer = wn.HipTimer()

    def once(call):
        timer.start()
        call()
        timer.stop()
        return timer.elapsed_ms()

    def alternate(yardstick, call):
        """(mean, min) of the yardstick and of the call, measured in turns."""
        yardstick()
        call()
        torch.cuda.synchronize()
        ys, cs = [], []
        for _ in range(REPS):
            ys.append(once(yardstick))
            cs.append(once(call))
        return (float(np.mean(ys)), float(np.min(ys))), (float(np.mean(cs)), float(np.min(cs)))

    pts = torch.from_numpy(np.random.default_rng(1).uniform(0.0, BOX, (NPTS, 3))).cuda()
    pts32 = pts.to(torch.float32)
    out = torch.empty((NPTS, 3), dtype=torch.float64, device="cuda")
    vel = torch.empty((NPTS, 3), dtype=torch.float64, device="cuda")
    adv = capi.wn_advect(capi.WN_ADVECT_RK4, TRACE_STEPS, 0.05, 1.0, (C.c_float * 3)(0.0, 0.0, 0.0), 0)
    obstacle_lists = {k: nm.WaveletNoise._obstacles(v) for k, v in scenes().items()}
    obstacle_lists["none"] = nm.WaveletNoise._obstacles([])

    def unbounded():
        nm.check(lib.wn_perlin_curl_advect_points(h, nm._ptr(pts), NPTS, kind, depth, off, C.byref(adv), nm._ptr(out), None, st))

    def bounded(scene):
        obs, nobs = obstacle_lists[scene]
        return lambda: nm.check(lib.wn_perlin_curl_bounded_advect_points_f64(h, nm._ptr(pts), NPTS, kind, depth, off, obs, nobs,
                                                                            C.byref(adv), nm._ptr(out), None, st))

    def curl_point():
        if name == "noise":
            nm.check(lib.wn_perlin_curl_points(h, nm._ptr(pts), NPTS, off, nm._ptr(vel), st))
        else:
            nm.check(lib.wn_perlin_curl_points_vec3(h, nm._ptr(pts32), NPTS, kind, depth, off, nm._ptr(vel), st))

    def potential_point():
        if name == "noise":
            nm.check(lib.wn_perlin_curl_potential_points_f64(h, nm._ptr(pts), NPTS, off, nm._ptr(vel), st))
        else:
            nm.check(lib.wn_perlin_curl_potential_points_f32(h, nm._ptr(pts32), NPTS, kind, depth, off, nm._ptr(vel), st))

    def bounded_point(scene):
        obs, nobs = obstacle_lists[scene]
        if name == "noise":
            return lambda: nm.check(lib.wn_perlin_curl_bounded_points_f64(h, nm._ptr(pts), NPTS, off, obs, nobs, nm._ptr(vel), st))
        return lambda: nm.check(lib.wn_perlin_curl_bounded_points_f32(h, nm._ptr(pts32), NPTS, kind, depth, off, obs, nobs,
                                                                      nm._ptr(vel), st))
    count = STAGES * TRACE_STEPS

    def launches(*calls):
        def run():
            for _ in range(count):
                for call in calls:
                    call()
        return run

    def emit(**row):
        print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items()}), flush=True)

    # bar (a)
    (both, both_min), (near, near_min) = alternate(launches(curl_point, potential_point), bounded("near"))
    (curl, curl_min), (near2, _) = alternate(launches(curl_point), bounded("near"))
    emit(name=f"{name}_bar_a_every_particle_near", ms_bounded_advect=near, ms_bounded_advect_min=near_min,
         ms_64_curl_plus_64_potential_launches=both, ms_launches_min=both_min, bounded_over_curl_plus_potential=near / both,
         bar_1_0_met=bool(near <= both), ms_bounded_advect_second_run=near2, ms_64_curl_launches=curl, ms_64_curl_launches_min=curl_min,
         bounded_over_curl_launches_alone=near2 / curl, points=NPTS)
    # bar (b)
    (free, free_min), (none, none_min) = alternate(unbounded, bounded("none"))
    emit(name=f"{name}_bar_b_nobs_0", ms_unbounded_advect=free, ms_unbounded_min=free_min, ms_bounded_nobs_0=none,
         ms_bounded_nobs_0_min=none_min, nobs_0_over_unbounded=none / free,
         unbounded_spread=(free - free_min) / free, points=NPTS)
    per_octave = free / (TRACE_STEPS * STAGES * octaves)
    # far and the scene, each against the unbounded call
    far = {}
    for scene in ("far1", "far3", "far16", "scene", "near"):
        nobs = obstacle_lists[scene][1]
        per_launch = lib.wn_perlin_bounded_advect_launch_steps(kind, depth, capi.WN_ADVECT_RK4, nobs)
        (yard, _), (ms, ms_min) = alternate(unbounded, bounded(scene))
        far[scene] = ms
        emit(name=f"{name}_{scene}", nobs=nobs, ms_bounded_advect=ms, ms_bounded_advect_min=ms_min, ms_unbounded_advect=yard,
             bounded_over_unbounded=ms / yard, launch_steps=per_launch, launches=-(-TRACE_STEPS // per_launch),
             ms_longest_launch=ms / TRACE_STEPS * min(per_launch, TRACE_STEPS),
             under_50_ms=bool(ms / TRACE_STEPS * min(per_launch, TRACE_STEPS) <= LAUNCH_MS_LIMIT))
    ramp_ms = (far["far16"] - far["far1"]) / 15.0 / (TRACE_STEPS * STAGES)
    emit(name=f"{name}_kappa", ms_per_octave_evaluation=per_octave, ms_per_obstacle_ramp=ramp_ms, kappa=ramp_ms / per_octave)
    # the point entries against their unbounded twin
    for label, call in (("potential_points", potential_point), ("bounded_points_near", bounded_point("near")),
                        ("bounded_points_scene", bounded_point("scene")), ("bounded_points_far16", bounded_point("far16"))):
        (yard, _), (ms, ms_min) = alternate(curl_point, call)
        emit(name=f"{name}_{label}", ms=ms, ms_min=ms_min, ms_curl_points=yard, over_curl_points=ms / yard)
    torch.cuda.synchronize()
    print(json.dumps({"name": "device", **wn.device_info(), "time": time.strftime("%Y-%m-%d")}), flush=True)


def main():
    out = os.path.join(ROOT, "profiles", "perlin_bounded_kernels.txt")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    text = ["Perlin bounded kernels (csrc/wn_perlin_bounded.hip) on one MI355X: python profiles/perlin_bounded_timing.py" + (" --quick" if QUICK else ""),
            "(HIP events on the launch stream; milliseconds per call of 16 RK4 steps, or per point launch; every call alternates",
            "with its yardstick)", ""]
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
