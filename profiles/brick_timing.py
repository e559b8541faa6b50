"""Sustained time of the four 512^3 brick-kernel grids (gradient and curl, one band and five) of profiles/grad_timing.py
and profiles/curl_timing.py, with the library of the tree given as argv[1] (a checkout with its libwnoise_hip.so built), so that two builds can be timed
in turn in one visit; one JSON line, labelled argv[2].

    python profiles/brick_timing.py <tree> <label>"""
import ctypes as C
import json
import os
import sys

root = os.path.abspath(sys.argv[1])
sys.path.insert(0, os.path.join(root, "profiles"))
import grad_timing as gt  # noqa: E402  (imports the package of its own tree)

wn, nm = gt.wn, gt.nm
import torch  # noqa: E402

torch.cuda.set_device(0)
noise = wn.WaveletNoise(128, 12345)
noise.generateNoiseTile3D()
n = 512
vol = n ** 3
os_, inv = nm._octave_scale(4), nm._inv_stddev(0.18402)
out = torch.empty(4 * vol, dtype=torch.float32, device="cuda")
h, st, p = noise._handle(3), nm._stream(), nm._ptr(out)
off = noise._curl_offsets(((0, 0, 0), (42, 42, 42), (85, 85, 85)))
w5 = (C.c_float * 5)(*[1.0] * 5)
g1 = wn.GridSpec(n, n, n, 0, n, octave_scale=os_, post_scale=2.0, out_scale=inv, flags=nm.WN_GRID_DEFAULT).c()
g5 = wn.GridSpec(n, n, n, 0, n, flags=nm.WN_GRID_DEFAULT).c()
lib = nm._lib
calls = {
    "grad_1": lambda: nm.check(lib.wn_eval3d_grad_grid(h, C.byref(g1), p, st)),
    "grad_5": lambda: nm.check(lib.wn_multiband3d_grad_grid(h, C.byref(g5), -16.0, 0, 5, w5, 0.18402, p, st)),
    "curl_1": lambda: nm.check(lib.wn_eval3d_curl_grid(h, C.byref(g1), off, p, st)),
    "curl_5": lambda: nm.check(lib.wn_multiband3d_curl_grid(h, C.byref(g5), off, -16.0, 0, 5, w5, 0.18402, p, st)),
}
res = {"label": sys.argv[2]}
for name, launch in calls.items():
    mean, best, sustained, k = gt.measure(launch)
    res[name] = {"sustained_us": round(sustained, 2), "launch_us_min": round(best, 2), "k": k}
torch.cuda.synchronize()
print(json.dumps(res), flush=True)
