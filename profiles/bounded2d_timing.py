"""HIP-event timing (wn_timer) of 2-D curl noise with solid boundaries and a background stream
(csrc/wn_wavelet_bounded2d.hip) on one MI355X, on the workload of profiles/curl2d_timing.py: 16 M particles uniform in a
128-cell box, tile 128, RK4, 16 steps, one and five bands.

    (a) near    one container with d0 = r around the box: every particle is near.  The fused call against the 64
                wn_multiband2d_grad_points launches (each gives psi and grad psi) a caller would otherwise compose, timed
                alone without the caller's ramp and stage arithmetic.  Bar: fused <= 1.0 x.
    (b) far     1, 3 and 16 obstacles that every particle is far from, and none at all (no stream), against the unbounded
                wn_multiband2d_curl_advect_points.  No bar but for none: its ratio must lie inside the unbounded call's spread.
    (c) mixed   a half-plane, two discs and a stream; the far / near / inside shares of the particles at the start.
    (d) points  wn_multiband2d_curl_bounded_points on the 16 M list and _grid on a 4096^2 image of the mixed scene against
                wn_multiband2d_curl_points / _curl_grid; with --gather DIR the same calls of a build whose lists never
                stage the tile (EXTRA_HIPFLAGS="-DWN_BOUNDED2D_POINTS_LDS_MIN_POINTS=4294967295
                -DWN_BOUNDED2D_ADVECT_LDS_MIN_POINTS=4294967295").
    (e) shape   with --wg1 DIR the rows of (a), (b) with 3 obstacles and (c) of a build with one workgroup per CU
                (EXTRA_HIPFLAGS=-DWN_BOUNDED2D_WORKGROUPS_PER_CU=1), against this tree's.

    python profiles/bounded2d_timing.py [--wg1 DIR] [--gather DIR] [--quick] [--out profiles/bounded2d_kernels.txt]
    (a variant build: make -C <copy of the package> EXTRA_HIPFLAGS=...; DIR is the copy of the repository that holds it)

Every pair of calls that is compared is timed alternately in the same child process: after a warm-up of both, SAMPLES
samples of each in turn, a sample being back-to-back calls for at least 0.15 s between two events on the launch stream,
divided by their number.  A row gives the mean of a call's samples; `spread` is (max - min) / mean of the yardstick's samples.
The driver runs every tree as a child process under its own `timeout` and stops at the first child that fails."""
import ctypes as C
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUICK = "--quick" in sys.argv
NPTS = 1 << (18 if QUICK else 24)
SIDE = 512 if QUICK else 4096
TRACE_STEPS = 16
SAMPLES = 5
WINDOW_S = 0.02 if QUICK else 0.15
LIMIT = 420   # seconds allowed per child

NEAR = [("container", (64.0, 64.0), 128.0, 128.0)]
FAR16 = [("container", (64.0, 64.0), 1000.0, 100.0), ("halfplane", (0.0, 1.0), -1000.0, 100.0),
         ("disc", (500.0, 500.0), 50.0, 50.0)] + [("disc", (600.0 + 120.0 * k, 500.0), 50.0, 50.0) for k in range(13)]
MIXED = [("halfplane", (0.0, 1.0), 16.0, 12.0), ("disc", (80.0, 36.0), 8.0, 12.0), ("disc", (40.0, 90.0), 12.8, 12.0)]
STREAM = (1.0, 0.0)


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def child(root, which):
    """Time the sections `which` (a comma list of a, b, c, d) with the package of the tree at `root`."""
    sys.path.insert(0, root)
    import numpy as np
    import torch
    wn = importlib.import_module("wavelet-noise-in-ray-tracing_amd")
    nm = importlib.import_module("wavelet-noise-in-ray-tracing_amd.noise")
    capi = nm._capi
    torch.cuda.set_device(0)
    lib, st, check, ptr = nm._lib, nm._stream(), nm.check, nm._ptr
    noise = wn.WaveletNoise(128, 12345)
    noise.generateNoiseTile2D()
    h = noise._handle(2)
    pts = torch.rand((NPTS, 2), dtype=torch.float32, device="cuda", generator=torch.Generator("cuda").manual_seed(1)) * 128.0
    out = torch.empty(3 * max(SIDE * SIDE, NPTS), dtype=torch.float32, device="cuda")
    ones = (C.c_float * 8)(*([1.0] * 8))
    adv = capi.wn_advect2d(capi.WN_ADVECT_RK4, TRACE_STEPS, 0.001, 1.0, (C.c_float * 2)(0.0, 0.0), 0)
    timer = wn.HipTimer()
    tree = os.path.relpath(root, ROOT)

    def emit(**line):
        print(json.dumps({"tree": tree, **line}), flush=True)

    def bounded(nb, obstacles, flow):
        obs, nobs, fl = noise._bounds2d(obstacles, flow)
        return lambda: check(lib.wn_multiband2d_curl_bounded_advect_points(h, ptr(pts), NPTS, -16.0, 0, nb, ones, 0.19686, obs,
                                                                           nobs, fl, C.byref(adv), ptr(out), None, st))

    def unbounded(nb):
        return lambda: check(lib.wn_multiband2d_curl_advect_points(h, ptr(pts), NPTS, -16.0, 0, nb, ones, 0.19686, C.byref(adv),
                                                                   ptr(out), None, st))

    def grad_launches(nb):
        def launch():
            for _ in range(4 * TRACE_STEPS):
                check(lib.wn_multiband2d_grad_points(h, ptr(pts), NPTS, -16.0, 0, nb, ones, 0.19686, ptr(out), st))
        return launch

    def sample(call, k):
        timer.start()
        for _ in range(k):
            call()
        timer.stop()
        return timer.elapsed_ms() / k

    def alternately(yard, mine):
        """SAMPLES samples of each call in turn, after both are warm: (the yardstick's, the other's), milliseconds per call."""
        ks = []
        for call in (yard, mine):
            call()
            torch.cuda.synchronize()
            ks.append(max(1, int(WINDOW_S * 1e3 / max(sample(call, 1), 1e-3)) + 1))
        ty, tm = [], []
        for _ in range(SAMPLES):
            ty.append(sample(yard, ks[0]))
            tm.append(sample(mine, ks[1]))
        return ty, tm

    def row(name, yard_name, ty, tm, **more):
        mean_y, mean_m = float(np.mean(ty)), float(np.mean(tm))
        spread = (max(ty) - min(ty)) / mean_y
        emit(name=name, ms=round(mean_m, 4), ms_min=round(min(tm), 4), ms_max=round(max(tm), 4), yardstick=yard_name,
             yardstick_ms=round(mean_y, 4), yardstick_spread=round(spread, 5), ratio=round(mean_m / mean_y, 5), **more)
        return mean_m / mean_y, spread

    def classes(obstacles):
        """The far / near / inside shares of the particles at the start, from the distances in float32 on the device."""
        inside = torch.zeros(NPTS, dtype=torch.bool, device="cuda")
        near = torch.zeros(NPTS, dtype=torch.bool, device="cuda")
        for kind, c, r, d0 in obstacles:
            if kind == "halfplane":
                d = (c[0] * pts[:, 0] + c[1] * pts[:, 1]) - r
            else:
                ln = torch.sqrt((pts[:, 0] - c[0]) ** 2 + (pts[:, 1] - c[1]) ** 2)
                d = ln - r if kind == "disc" else r - ln
            inside |= d <= 0
            near |= d < d0
        ins = float(inside.float().mean())
        nr = float((near & ~inside).float().mean())
        return {"far": round(1.0 - ins - nr, 4), "near": round(nr, 4), "inside": round(ins, 4)}

    for nb in (1, 5):
        if "a" in which:
            ty, tm = alternately(grad_launches(nb), bounded(nb, NEAR, None))
            ratio, _ = row(f"a_near_rk4_nb{nb}", f"{4 * TRACE_STEPS} wn_multiband2d_grad_points launches", ty, tm,
                           shares=classes(NEAR), particle_steps_per_s=round(NPTS * TRACE_STEPS / (float(np.mean(tm)) * 1e-3), 0))
            emit(name=f"a_bar_nb{nb}", fused_over_replaced_launches=round(ratio, 5), bar_a_1_0_met=bool(ratio <= 1.0))
        if "b" in which:
            for nobs in ((0, 1, 3, 16) if which != "abc_shape" else (3,)):
                ty, tm = alternately(unbounded(nb), bounded(nb, FAR16[:nobs], None))
                ratio, spread = row(f"b_far_{nobs}_obstacles_rk4_nb{nb}", "wn_multiband2d_curl_advect_points", ty, tm,
                                    shares=classes(FAR16[:nobs]))
                if nobs == 0:
                    emit(name=f"b_none_nb{nb}", ratio=round(ratio, 5), spread=round(spread, 5),
                         inside_spread=bool(abs(ratio - 1.0) <= spread))
        if "c" in which:
            ty, tm = alternately(unbounded(nb), bounded(nb, MIXED, STREAM))
            row(f"c_mixed_rk4_nb{nb}", "wn_multiband2d_curl_advect_points", ty, tm, shares=classes(MIXED),
                particle_steps_per_s=round(NPTS * TRACE_STEPS / (float(np.mean(tm)) * 1e-3), 0))
        if "d" in which:
            obs, nobs, fl = noise._bounds2d(MIXED, STREAM)
            ty, tm = alternately(
                lambda: check(lib.wn_multiband2d_curl_points(h, ptr(pts), NPTS, -16.0, 0, nb, ones, 0.19686, ptr(out), st)),
                lambda: check(lib.wn_multiband2d_curl_bounded_points(h, ptr(pts), NPTS, -16.0, 0, nb, ones, 0.19686, obs, nobs, fl,
                                                                     ptr(out), st)))
            row(f"d_points_mixed_nb{nb}", "wn_multiband2d_curl_points", ty, tm, points=NPTS)
            # the image: p = (i / 4096) * 4 * 32 covers the 128-cell box
            gc = nm.GridSpec(SIDE, SIDE, SIDE, post_scale=32.0).c()
            ty, tm = alternately(
                lambda: check(lib.wn_multiband2d_curl_grid(h, C.byref(gc), -16.0, 0, nb, ones, 0.19686, ptr(out), st)),
                lambda: check(lib.wn_multiband2d_curl_bounded_grid(h, C.byref(gc), -16.0, 0, nb, ones, 0.19686, obs, nobs, fl,
                                                                   ptr(out), st)))
            row(f"d_image_{SIDE}_mixed_nb{nb}", "wn_multiband2d_curl_grid", ty, tm)
    torch.cuda.synchronize()
    emit(**{"name": "device", **wn.device_info(), "launch_steps_rk4_nb1": lib.wn_advect2d_launch_steps(2, 1),
            "launch_steps_rk4_nb5": lib.wn_advect2d_launch_steps(2, 5), "time": time.strftime("%Y-%m-%d")})


def main():
    out = arg("--out", os.path.join(ROOT, "profiles", "bounded2d_kernels.txt"))
    trees = [(ROOT, "abcd")]
    if arg("--wg1"):
        trees.append((os.path.abspath(arg("--wg1")), "abc_shape"))
    if arg("--gather"):
        trees.append((os.path.abspath(arg("--gather")), "cd"))
    text = ["Bounded 2-D curl kernels (csrc/wn_wavelet_bounded2d.hip) on one MI355X: python profiles/bounded2d_timing.py"
            + (" --quick" if QUICK else ""),
            "(HIP events on the launch stream; milliseconds per call; ratio = this call / its yardstick, the two timed alternately;",
            "tree '.' is the product, the others the variant builds named in the script's docstring)", ""]
    rc, rows = 0, []
    for root, which in trees:
        cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--child", root, which] \
            + (["--quick"] if QUICK else [])
        res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
        print(res.stdout, end="", flush=True)
        text += [f"[{os.path.relpath(root, ROOT)}: {which}]"] + res.stdout.splitlines() + [""]
        if res.returncode != 0:   # nothing more runs on the device after a failed child
            print(res.stderr[-3000:], file=sys.stderr)
            text += [f"the child of {root} failed with exit status {res.returncode}; later trees were not run"]
            rc = 1
            break
        rows += [json.loads(ln) for ln in res.stdout.splitlines() if ln.startswith("{")]
    if rc == 0:   # the variant trees against the product, row by row
        mine = {r["name"]: r["ms"] for r in rows if r["tree"] == "." and "ms" in r}
        summary = {f"{r['tree']}_over_product_{r['name']}": round(r["ms"] / mine[r["name"]], 4)
                   for r in rows if r["tree"] != "." and r.get("name") in mine}
        if summary:
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
