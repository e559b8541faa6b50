"""HIP-event timing (wn_timer) of fused particle advection with solid boundaries (csrc/wn_wavelet_bounded.hip) on one MI355X,
on the workload of profiles/advect_timing.py: 16 M particles uniform in a 128-cell box, tile 128, RK4, 16 steps.

    single    wn_eval3d_curl_bounded_advect_points        (offsets: the tile's default)
    bands     wn_multiband3d_curl_bounded_advect_points   (5 bands from first band -2, w = 1)
    each with three obstacle lists:
      far     a container, a ground plane and a sphere that every particle is far from (d >= d0 for all three)
      near    one container with d0 = r around the box: every particle is near
      scene   the reference scene's ground plane, textured sphere and light sphere, 16 cells per world unit
    bar (a)   near: the fused call against the launches it replaces, timed ALONE without the loop's arithmetic:
              64 x wn_eval3d_curl_points + 3 x 64 x wn_eval3d_points on the rolled tiles (bands: the multiband forms)
    bar (b)   far: the fused call against the unbounded wn_eval3d_curl_advect_points, the two alternating, five calls
              each; the spread is (max - min) / mean of the unbounded call's five times

    python profiles/bounded_timing.py [--quick] [--out profiles/bounded_kernels.txt]

The driver runs every step as a child process under its own `timeout`, stops at the first step that fails, and writes the
steps' JSON lines to --out.  A call is timed between two events on the launch stream; one warm-up call, then the mean and
the minimum of 3 (--quick: 1 M particles)."""
import ctypes as C
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = {"single": 150, "bands": 300}   # seconds allowed
QUICK = "--quick" in sys.argv
NPTS = 1 << (20 if QUICK else 24)
TRACE_STEPS = 16
REPS = 3
ALTERNATIONS = 5

FAR = [("container", (64.0, 64.0, 64.0), 1000.0, 100.0), ("halfspace", (0.0, 1.0, 0.0), -1000.0, 100.0),
       ("sphere", (500.0, 500.0, 500.0), 50.0, 50.0)]
NEAR = [("container", (64.0, 64.0, 64.0), 128.0, 128.0)]
# main.cpp's world times 16 plus (64, 24, 64): the ground y = -0.5, the sphere (1, 0, -1.75) r 0.5, the light (-5, 5, 0) r 0.8
SCENE = [("halfspace", (0.0, 1.0, 0.0), 16.0, 12.0), ("sphere", (80.0, 24.0, 36.0), 8.0, 12.0),
         ("sphere", (-16.0, 104.0, 64.0), 12.8, 12.0)]


def step(name):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    wn = importlib.import_module("wavelet-noise-in-ray-tracing_amd")
    nm = importlib.import_module("wavelet-noise-in-ray-tracing_amd.noise")
    capi = nm._capi
    torch.cuda.set_device(0)
    lib = nm._lib
    noise = wn.WaveletNoise(128, 12345)
    noise.generateNoiseTile3D()
    h, off, st = noise._handle(3), noise._curl_offsets(None), nm._stream()
    coef = noise.getNoiseCoefficients().reshape(128, 128, 128)
    rolled = [wn.WaveletNoise.from_coefficients(np.roll(coef, shift=(-o, -o, -o), axis=(0, 1, 2)), 3)
              for o in (0, 128 // 3, 2 * 128 // 3)]          # the default offsets' tiles T_k
    w5 = (C.c_float * 5)(*[1.0] * 5)
    timer = wn.HipTimer()

    def once(call):
        timer.start()
        call()
        timer.stop()
        return timer.elapsed_ms()

    def timed(call):
        call()
        torch.cuda.synchronize()
        per = [once(call) for _ in range(REPS)]
        return float(np.mean(per)), float(np.min(per))

    pts = torch.from_numpy(np.random.default_rng(1).uniform(0.0, 128.0, (NPTS, 3)).astype(np.float32)).cuda()
    out = torch.empty((NPTS, 3), dtype=torch.float32, device="cuda")
    vel = torch.empty((NPTS, 3), dtype=torch.float32, device="cuda")
    val = torch.empty(NPTS, dtype=torch.float32, device="cuda")
    step_h = 0.05 if name == "single" else 0.005
    a = capi.wn_advect(capi.WN_ADVECT_RK4, TRACE_STEPS, step_h, 1.0, (C.c_float * 3)(0.0, 0.0, 0.0), 0)

    if name == "single":
        def bounded(obs, nobs):
            nm.check(lib.wn_eval3d_curl_bounded_advect_points(h, nm._ptr(pts), NPTS, off, obs, nobs, C.byref(a), nm._ptr(out), None, st))

        def unbounded():
            nm.check(lib.wn_eval3d_curl_advect_points(h, nm._ptr(pts), NPTS, off, C.byref(a), nm._ptr(out), None, st))

        def curl_launches():
            for _ in range(4 * TRACE_STEPS):
                nm.check(lib.wn_eval3d_curl_points(h, nm._ptr(pts), NPTS, off, nm._ptr(vel), st))

        def value_launches():
            for _ in range(4 * TRACE_STEPS):
                for t in rolled:
                    nm.check(lib.wn_eval3d_points(t._handle(3), nm._ptr(pts), NPTS, nm._ptr(val), st))
    elif name == "bands":
        def bounded(obs, nobs):
            nm.check(lib.wn_multiband3d_curl_bounded_advect_points(h, nm._ptr(pts), NPTS, off, -16.0, -2, 5, w5, 0.18402, obs, nobs,
                                                                   C.byref(a), nm._ptr(out), None, st))

        def unbounded():
            nm.check(lib.wn_multiband3d_curl_advect_points(h, nm._ptr(pts), NPTS, off, -16.0, -2, 5, w5, 0.18402, C.byref(a),
                                                           nm._ptr(out), None, st))

        def curl_launches():
            for _ in range(4 * TRACE_STEPS):
                nm.check(lib.wn_multiband3d_curl_points(h, nm._ptr(pts), NPTS, off, -16.0, -2, 5, w5, 0.18402, nm._ptr(vel), st))

        def value_launches():
            for _ in range(4 * TRACE_STEPS):
                for t in rolled:
                    nm.check(lib.wn_multiband3d_points(t._handle(3), nm._ptr(pts), NPTS, -16.0, -2, 5, w5, 0.18402, nm._ptr(val), st))
    else:
        raise SystemExit(f"unknown step {name}")

    def emit(**line):
        print(json.dumps(line), flush=True)

    # where the particles are at the start (they move about 0.1 cell per step)
    for label, obstacles in (("far", FAR), ("near", NEAR), ("scene", SCENE)):
        v = noise.evaluate3DCurlBounded(pts[:1 << 20], obstacles)
        free = noise.evaluate3DCurl(pts[:1 << 20])
        same = (v == free).all(1)
        emit(name=f"{label}_classes_of_the_first_1M", unbounded_bits=round(float(same.float().mean()), 4),
             zero=round(float(((v == 0).all(1) & ~same).float().mean()), 4))

    # bar (b): every particle far, against the unbounded call, alternating
    far_obs, far_n = noise._obstacles(FAR)
    unbounded()
    bounded(far_obs, far_n)
    torch.cuda.synchronize()
    tu, tb = [], []
    for _ in range(ALTERNATIONS):
        tu.append(once(unbounded))
        tb.append(once(lambda: bounded(far_obs, far_n)))
    spread = (max(tu) - min(tu)) / float(np.mean(tu))
    ratio = float(np.mean(tb)) / float(np.mean(tu))
    emit(name=f"{name}_unbounded_rk4_{TRACE_STEPS}_steps_fused", ms_mean=round(float(np.mean(tu)), 3), ms_min=round(min(tu), 3),
         ms_max=round(max(tu), 3), spread=round(spread, 5), points=NPTS)
    emit(name=f"{name}_far_rk4_{TRACE_STEPS}_steps_fused", ms_mean=round(float(np.mean(tb)), 3), ms_min=round(min(tb), 3),
         ms_max=round(max(tb), 3), bounded_over_unbounded=round(ratio, 5), bar_b_within_spread_met=bool(ratio <= 1.0 + spread))

    # bar (a): every particle near, against the launches it replaces
    curl_mean, curl_min = timed(curl_launches)
    value_mean, value_min = timed(value_launches)
    emit(name=f"{name}_{4 * TRACE_STEPS}_curl_point_launches", ms_mean=round(curl_mean, 3), ms_min=round(curl_min, 3))
    emit(name=f"{name}_{3 * 4 * TRACE_STEPS}_value_point_launches", ms_mean=round(value_mean, 3), ms_min=round(value_min, 3))
    replaced = curl_mean + value_mean
    for label, obstacles in (("near", NEAR), ("scene", SCENE)):
        obs, nobs = noise._obstacles(obstacles)
        mean, best = timed(lambda: bounded(obs, nobs))
        line = dict(name=f"{name}_{label}_rk4_{TRACE_STEPS}_steps_fused", ms_mean=round(mean, 3), ms_min=round(best, 3),
                    ms_per_step=round(mean / TRACE_STEPS, 3), launches=-(-TRACE_STEPS // lib.wn_advect_launch_steps()))
        if label == "near":
            line.update(fused_over_replaced_launches=round(mean / replaced, 4), bar_a_1_0_met=bool(mean <= replaced))
        emit(**line)
    torch.cuda.synchronize()
    emit(**{"name": "device", **wn.device_info(), "launch_steps": lib.wn_advect_launch_steps(), "time": time.strftime("%Y-%m-%d")})


def main():
    out = os.path.join(ROOT, "profiles", "bounded_kernels.txt")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    text = ["Boundary kernels (csrc/wn_wavelet_bounded.hip) on one MI355X: python profiles/bounded_timing.py" + (" --quick" if QUICK else ""),
            "(HIP events on the launch stream; milliseconds per call; the replaced launches are the 64 curl and 192 value launches",
            "of a caller's own 16-step RK4 loop through the bounded field, without its ramp and stage arithmetic)", ""]
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
