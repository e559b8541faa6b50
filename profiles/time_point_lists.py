#!/usr/bin/env python3
"""Time WaveletNoise::evaluate3D / WMultibandNoise point lists (the C ABI's wn_eval3d_points / wn_multiband3d_points) on
three kinds of 40 M-point lists -- uniformly random in 3-D, random on an axis-aligned plane, coherent (a scanline-ordered
sweep) -- with HIP events on the launching stream.  Run on the GPU box:  python profiles/time_point_lists.py
"""
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
wn = importlib.import_module("wavelet-noise-in-ray-tracing_amd")

N = 40_000_000
rng = np.random.default_rng(1)
noise = wn.WaveletNoise(128, 12345)
noise.generateNoiseTile3D()
lists = {
    "random_3d": rng.uniform(-40, 40, (N, 3)).astype(np.float32),
    "random_on_plane_y": np.stack([rng.uniform(-40, 40, N), np.full(N, -0.5), rng.uniform(-40, 40, N)], 1).astype(np.float32),
    "coherent_sweep": np.stack([np.tile(np.linspace(-40, 40, 4000), N // 4000), np.full(N, 0.25),
                                np.repeat(np.linspace(-40, 40, N // 4000), 4000)], 1).astype(np.float32),
}
out = {"points": N, "sorted_kernel": "on", "lists": {}}
for name, pts in lists.items():
    dev = torch.from_numpy(pts).cuda()
    row = {}
    for what, call in (("evaluate3D", lambda: noise.evaluate3D(dev)),
                       ("WMultibandNoise5", lambda: noise.WMultibandNoise(dev * 0.1, -16.0, 0, 5, [1.0] * 5))):
        if what == "WMultibandNoise5":
            small = (dev * 0.1).contiguous()
            call = lambda: noise.WMultibandNoise(small, -16.0, 0, 5, [1.0] * 5)  # noqa: E731
        for _ in range(2):
            call()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            call()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / 5
        row[what] = {"ms": round(ms, 3), "Gpoints_per_s": round(N / ms / 1e6, 2)}
    out["lists"][name] = row
    del dev
print(json.dumps(out))
