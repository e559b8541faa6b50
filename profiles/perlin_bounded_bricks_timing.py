"""HIP-event timing (wn_timer) of the bounded Perlin curl brick-list kernel (csrc/wn_perlin_bounded_bricks.hip,
include/wnoise_perlin_bounded_bricks.h) on one MI355X, in the manner of profiles/perlin_bricks_timing.py and
profiles/bounded_bricks_timing.py: the 512^3 lattice at den 512 -- noise at octave 4 (step 1/8 cell), turb(7) and fractal_noise
at octave 0 (step 1/128) -- with the scene of tests/test_gpu_perlin_bounded_bricks.py scaled to the volume (a sphere, a floor
and a container: profiles/bounded_bricks_timing.py's scene()), default offsets.

    BAR       the brick call takes no more than 1.0 x wn_perlin_curl_bounded_points_f32 on exactly the same samples (512 float
              coordinates per brick): the call a sparse-volume holder makes without the brick entry point.  On the three lists
              of profiles/bricks_timing.py -- all 262,144 bricks in raster order, a uniform random 10 % (26,214) in random
              order, the sphere shell (10,220) -- for the three kinds: 9 rows.  The two are timed alternately, ROUNDS times
              each in the same process; the ratio is reported per round, with its spread.
    no bar    against the unbounded wn_perlin_curl_bricks on the random 10 % list: the scene; a scene in which every sample is
              near (one container whose ramp covers the volume: the 9-sum walk and the composition everywhere); scenes in
              which every sample is far from 1, 3 and 16 obstacles (the ramp's cost per obstacle around the 6-sum walk); the
              scene on the bricks that lie wholly inside its sphere (no octave loop); and nobs == 0, which is the unbounded
              call: its ratio shows the run-to-run spread.

    python profiles/perlin_bounded_bricks_timing.py [--quick] [--out profiles/perlin_bounded_bricks_kernels.txt]

The driver runs every step as a child process under its own `timeout`, stops at the first step that fails, and writes the
steps' JSON lines to --out, then a [summary] made from them, then the [notes] section of the committed record as it is (the
hand-written part: causes, and register counts of forms that are not in the tree).  Per-launch and sustained times: profiles/bricks_timing.py's measure(); the no-bar ratios:
profiles/bounded_bricks_timing.py's alternate() (medians over alternating bursts)."""
import ctypes as C
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import bounded_bricks_timing as bbt  # noqa: E402
import bricks_timing as bt  # noqa: E402

# step: (kind, depth, octave, seconds allowed)
STEPS = {"noise": (0, 0, 4, 300), "turb7": (1, 7, 0, 400), "fractal": (2, 0, 0, 400)}
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
    kind, depth, octave, _ = STEPS[name]
    bt.QUICK = bbt.QUICK = QUICK

    def report(label, launch, **extra):
        mean, best, worst, sustained, k = bt.measure(wn, np, torch, launch)
        line = {"name": label, "launch_us_mean": round(mean, 2), "launch_us_min": round(best, 2), "launch_us_max": round(worst, 2),
                "sustained_us": round(sustained, 2), "sustained_launches": k, **extra}
        print(json.dumps(line), flush=True)
        return line

    p = wn.perlin(12345)
    off = p._curl_offsets(None)
    oscale = float(nm._octave_scale(octave))
    gc = wn.GridSpec(N, N, N, 0, N, octave_scale=nm._octave_scale(octave)).c()
    h = float(np.float32(np.float32(np.float32(1.0) / np.float32(N)) * np.float32(4.0)) * np.float32(oscale))
    so, sn = wn.WaveletNoise._obstacles(bbt.scene(h))

    local = torch.arange(512, device="cuda")
    offs = torch.stack([local & 7, (local >> 3) & 7, local >> 6], -1)                   # (512, 3): lx, ly, lz
    lists = bt.brick_lists(np)
    for lname, host_list in lists.items():
        n = len(host_list)
        bricks = torch.from_numpy(host_list).cuda()
        out = torch.empty(3 * n * 512, dtype=torch.float32, device="cuda")
        out64 = torch.empty(3 * n * 512, dtype=torch.float64, device="cuda")
        # the same samples as a point list: c = (((float)i / den) * 4) * octave_scale per axis
        idx = (bricks[:, None, :] * 8 + offs[None, :, :]).to(torch.float32).reshape(-1, 3)
        pts = (((idx / float(N)) * 4.0) * oscale).contiguous()
        del idx

        def launch_points():
            nm.check(lib.wn_perlin_curl_bounded_points_f32(p._h, nm._ptr(pts), n * 512, kind, depth, off, so, sn, nm._ptr(out64), st))

        def launch_bricks():
            nm.check(lib.wn_perlin_curl_bounded_bricks(p._h, C.byref(gc), kind, depth, off, so, sn, nm._ptr(bricks), n, nm._ptr(out), st))
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
                          "ps_per_sample_bricks": round(last["sustained_us"] * 1e6 / (n * 512), 3)}), flush=True)
        del pts, out, out64, bricks

    # no bar: against the unbounded curl bricks
    def against_free(label, host_list, obstacles, nobs=None):
        n = len(host_list)
        bricks = torch.from_numpy(host_list).cuda()
        out = torch.empty(3 * n * 512, dtype=torch.float32, device="cuda")
        arr, count = wn.WaveletNoise._obstacles(obstacles)
        count = count if nobs is None else nobs

        def bounded():
            nm.check(lib.wn_perlin_curl_bounded_bricks(p._h, C.byref(gc), kind, depth, off, arr, count, nm._ptr(bricks), n, nm._ptr(out), st))

        def free():
            nm.check(lib.wn_perlin_curl_bricks(p._h, C.byref(gc), kind, depth, off, nm._ptr(bricks), n, nm._ptr(out), st))
        ta, tb, lo, hi, rounds = bbt.alternate(wn, np, torch, bounded, free)
        print(json.dumps({"name": f"{label}_{name}", "bricks": n, "obstacles": count, "bounded_us": round(ta, 2), "unbounded_us": round(tb, 2),
                          "bounded_over_unbounded_min": round(lo, 4), "bounded_over_unbounded_max": round(hi, 4), "rounds": rounds}), flush=True)

    tenth = lists["random_10_percent"]
    for sname, obstacles in (("scene", bbt.scene(h)), ("all_near", bbt.near_scene(h)), ("all_far_1", bbt.far_scene(h, 1)),
                             ("all_far_3", bbt.far_scene(h, 3)), ("all_far_16", bbt.far_scene(h, 16))):
        against_free(f"vs_unbounded_{sname}_random_10_percent", tenth, obstacles)
    against_free("vs_unbounded_scene_inside_the_sphere", bbt.inside_list(np), bbt.scene(h))
    against_free("vs_unbounded_nobs_0_random_10_percent", tenth, bbt.scene(h), nobs=0)
    torch.cuda.synchronize()
    print(json.dumps({"name": "device", **wn.device_info(), "time": time.strftime("%Y-%m-%d")}), flush=True)


def summary(text):
    """The [summary] section from the steps' JSON lines: the 9 rows against the bar, and the ratios to the unbounded call."""
    rows = {}
    for line in text:
        if line.startswith("{"):
            d = json.loads(line)
            rows[d["name"]] = d
    out = ["[summary]", "Sustained microseconds of the last round, points / bricks, and bricks / points over the rounds (min..max).",
           "BAR: bricks <= 1.0 x wn_perlin_curl_bounded_points_f32 on the same samples.", "",
           "%-10s %-20s %12s %12s   %-16s %s" % ("call", "list", "points", "bricks", "bricks/points", "bar")]
    met = total = 0
    last = 0 if QUICK else ROUNDS - 1
    for name in STEPS:
        for lname in ("full_raster", "random_10_percent", "sphere_shell"):
            r = rows.get(f"bricks_{lname}_{name}_ratios")
            if r is None:
                continue
            total += 1
            met += r["bar_1.0"] == "met"
            out.append("%-10s %-20s %12.1f %12.1f   %.3f..%.3f     %s" % (
                name, lname, rows[f"points_{lname}_{name}_round{last}"]["sustained_us"],
                rows[f"bricks_{lname}_{name}_round{last}"]["sustained_us"], r["bricks_over_points_min"], r["bricks_over_points_max"], r["bar_1.0"]))
    out += ["", f"bar met on {met} of {total} rows", "", "bounded / unbounded wn_perlin_curl_bricks (min..max over the bursts):"]
    for key, d in rows.items():
        if key.startswith("vs_unbounded_"):
            out.append("%-52s %.4f..%.4f" % (key[len("vs_unbounded_"):], d["bounded_over_unbounded_min"], d["bounded_over_unbounded_max"]))
    return out


def main():
    out = os.path.join(ROOT, "profiles", "perlin_bounded_bricks_kernels.txt")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    text = ["Bounded Perlin curl brick-list kernel (csrc/wn_perlin_bounded_bricks.hip) on one MI355X: "
            "python profiles/perlin_bounded_bricks_timing.py" + (" --quick" if QUICK else ""),
            "(HIP events on the launch stream; microseconds; den 512; noise at octave 4, turb(7) and fractal_noise at octave 0; the",
            " scene of the tests scaled to the volume; `points_*` is wn_perlin_curl_bounded_points_f32 on the same samples; ratios",
            " are of sustained times, points and bricks timed alternately; `vs_unbounded_*`: against wn_perlin_curl_bricks)", ""]
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
    text += summary(text)
    # what a run cannot produce -- what is known of the causes, the register counts of forms that are not in the tree -- is
    # kept by hand under [notes] in the committed record and carried over
    record = os.path.join(ROOT, "profiles", "perlin_bounded_bricks_kernels.txt")
    if os.path.exists(record):
        kept = open(record).read()
        if "\n[notes]\n" in kept:
            text += ["", "[notes]"] + kept.split("\n[notes]\n", 1)[1].rstrip("\n").splitlines()
    with open(out, "w") as f:
        f.write("\n".join(text) + "\n")
    return rc


if __name__ == "__main__":
    if "--step" in sys.argv:
        step(sys.argv[sys.argv.index("--step") + 1])
    else:
        sys.exit(main())
