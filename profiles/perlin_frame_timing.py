"""Sustained time and output digest of the nine 512^3 dense Perlin grids -- noise at octave 4, turb(7) and fractal_noise, each
through the value, gradient and curl entry points (csrc/wn_perlin.hip, wn_perlin_grad.hip, wn_perlin_curl.hip) -- with the
library of the tree given as argv[1] (a checkout with its libwnoise_hip.so built), so that two builds can be timed in turn
in one visit; one JSON line, labelled argv[2].  `sha256` is the digest of the call's whole output (1, 4 or 3 volumes).

    python profiles/perlin_frame_timing.py <tree> <label>"""
import ctypes as C
import hashlib
import json
import os
import sys

root = os.path.abspath(sys.argv[1])
sys.path.insert(0, os.path.join(root, "profiles"))
import perlin_grad_timing as pt  # noqa: E402  (imports the package of its own tree)

wn, nm = pt.wn, pt.nm
import torch  # noqa: E402

NOISE, TURB, FRACTAL = 0, 1, 2
torch.cuda.set_device(0)
st, lib = nm._stream(), nm._lib
p = wn.perlin(12345)
off = wn.perlin._curl_offsets(None)
n = 512
vol = n ** 3
out = torch.empty(4 * vol, dtype=torch.float32, device="cuda")
o = nm._ptr(out)
g4 = C.byref(wn.GridSpec(n, n, n, 0, n, octave_scale=nm._octave_scale(4)).c())
g1 = C.byref(wn.GridSpec(n, n, n, 0, n).c())
calls = {  # name -> (channels, launch)
    "noise_value": (1, pt.checked(lib.wn_perlin_grid, p._h, g4, o, st)),
    "noise_grad": (4, pt.checked(lib.wn_perlin_grad_grid, p._h, g4, o, st)),
    "noise_curl": (3, pt.checked(lib.wn_perlin_curl_grid, p._h, g4, NOISE, 0, off, o, st)),
    "turb7_value": (1, pt.checked(lib.wn_perlin_turb_grid, p._h, g1, 7, o, st)),
    "turb7_grad": (4, pt.checked(lib.wn_perlin_turb_grad_grid, p._h, g1, 7, o, st)),
    "turb7_curl": (3, pt.checked(lib.wn_perlin_curl_grid, p._h, g1, TURB, 7, off, o, st)),
    "fractal_value": (1, pt.checked(lib.wn_perlin_fractal_grid, p._h, g1, o, st)),
    "fractal_grad": (4, pt.checked(lib.wn_perlin_fractal_grad_grid, p._h, g1, o, st)),
    "fractal_curl": (3, pt.checked(lib.wn_perlin_curl_grid, p._h, g1, FRACTAL, 0, off, o, st)),
}
res = {"label": sys.argv[2]}
for name, (channels, launch) in calls.items():
    mean, best, sustained, k = pt.measure(launch)
    torch.cuda.synchronize()
    digest = hashlib.sha256(out[:channels * vol].cpu().numpy()).hexdigest()
    res[name] = {"sustained_us": round(sustained, 2), "launch_us_min": round(best, 2), "k": k, "sha256": digest}
torch.cuda.synchronize()
print(json.dumps(res), flush=True)
