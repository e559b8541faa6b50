"""CPU checks of the bounded curl brick-list entry points (include/wnoise_bounded_bricks.h): the header declares exactly the
two calls; they are exported by libwnoise_hip.so and bound in _capi.py's BOUNDED_BRICKS_SIGNATURES, a table of their own;
tests/_graph.py's prototypes() parses the header with `stream` last, one output and one device input; the names are no
writers of the completeness table; the Python and host-class wrappers exist; the header states its layout, its tiers, the
near formula and what it leaves out.  Without a HIP device the first check of every batched entry point -- the device --
answers before any other, so in a child process with the devices hidden (it holds on a GPU machine too) every call, valid
or with any of the refusals of tests/test_bounded_host.py's list, returns WN_ERR_NO_DEVICE and writes nothing; the refusals'
order and messages are checked where a device exists, in tests/test_gpu_bounded_bricks.py."""
import importlib
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _graph as G  # noqa: E402

PKG = os.path.join(ROOT, "wavelet-noise-in-ray-tracing_amd")
HEADER = os.path.join(ROOT, "include", "wnoise_bounded_bricks.h")
NAMES = ["wn_eval3d_curl_bounded_bricks", "wn_multiband3d_curl_bounded_bricks"]
BANDS = ["s", "first_band", "nbands", "w_host", "var_per_band"]
OTHER_TABLES = ("SIGNATURES", "PERLIN_CURL_SIGNATURES", "FOOTPRINT_SIGNATURES", "PERLIN_FOOTPRINT_SIGNATURES", "MULTIBAND2D_SIGNATURES",
                "ADVECT_SIGNATURES", "BOUNDED_SIGNATURES", "PERLIN_ADVECT_SIGNATURES", "CURL2D_SIGNATURES", "BOUNDED2D_SIGNATURES",
                "BRICKS_SIGNATURES", "BRICK_FIELDS_SIGNATURES")


def capi():
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(PKG, "libwnoise_hip.so")):
        ge.build()
    return importlib.import_module("wavelet-noise-in-ray-tracing_amd._capi")


def test_every_declared_name_is_exported_and_bound():
    header = open(HEADER).read()
    names = sorted(set(re.findall(r"WN_API\s+[\w\s\*]+?\b(wn_\w+)\s*\(", header)))
    assert names == NAMES, names
    c = capi()
    lib = c.load()
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/wnoise_bounded_bricks.h but not exported"
        assert getattr(lib, n).argtypes == c.BOUNDED_BRICKS_SIGNATURES[n][1] and getattr(lib, n).restype is c.BOUNDED_BRICKS_SIGNATURES[n][0]
    assert set(c.BOUNDED_BRICKS_SIGNATURES) == set(names)
    tables = [t for t in dir(c) if t.endswith("SIGNATURES") and t != "BOUNDED_BRICKS_SIGNATURES"]
    assert set(tables) == set(OTHER_TABLES), tables
    for other in tables:
        assert not set(names) & set(getattr(c, other)), other
    assert '#include "wnoise_brick_fields.h"' in header and '#include "wnoise_bounded.h"' in header
    # the argument lists are the unbounded curl bricks' with (obstacles, nobs) before the output
    for n in names:
        plain = c.BRICK_FIELDS_SIGNATURES[n.replace("_bounded", "")][1]
        assert c.BOUNDED_BRICKS_SIGNATURES[n][1] == plain[:-2] + [c._op, c._i] + plain[-2:], n
    pkg = importlib.import_module("wavelet-noise-in-ray-tracing_amd")
    for wrapper in ("curl_bounded_bricks", "multiband_curl_bounded_bricks"):
        assert callable(getattr(pkg, wrapper)) and wrapper in pkg.__all__, wrapper
    grid_h = open(os.path.join(PKG, "host", "noise_grid.h")).read()
    for fn in ("curlBoundedBricks", "multibandCurlBoundedBricks"):
        assert re.search(r"inline void %s\(" % fn, grid_h), fn
    assert '#include "wnoise_bounded_bricks.h"' in grid_h


def test_the_header_parses_as_a_call_description():
    protos = G.prototypes([HEADER])
    assert sorted(protos) == NAMES
    head = ["tile3d", "g", "bricks_dev", "n", "offsets9_host"]
    tail = ["obstacles_host", "nobs", "out_dev", "stream"]
    assert protos["wn_eval3d_curl_bounded_bricks"] == head + tail
    assert protos["wn_multiband3d_curl_bounded_bricks"] == head + BANDS + tail
    for name, params in protos.items():
        assert params[-1] == "stream" and [p for p in params if G.is_output(p)] == ["out_dev"], name
        assert [p for p in params if G.is_device_input(p)] == ["bricks_dev"], name
        want = ["g", "offsets9_host"] + (["w_host"] if "multiband" in name else []) + ["obstacles_host"]
        assert [p for p in params if G.is_host(p)] == want, name
    # brick lists are neither grids nor point lists: the completeness table of tests/test_gpu_graph_replay.py does not see
    # these names, and tests/test_gpu_bounded_bricks_graph.py holds their rows
    assert all(n.endswith("_bricks") for n in NAMES)
    assert not set(NAMES) & G.writers() and set(NAMES) <= G.declared()


def squeeze(path):
    return " ".join(open(path).read().replace("*", " ").split()).lower()


def test_the_header_states_its_contract_and_what_is_left_out():
    text = squeeze(HEADER)
    for phrase in ("out_dev[(ch n + i) 512 + lx + 8 (ly + 8 lz)]", "ch = 3", "left untouched", "float4 stores",
                   "wn_z_const is refused", "n == 0 is wn_ok", "3 n 512 overflowing size_t", "offsets9_host == null",
                   "wn_err_no_device", "no allocation, no synchronisation", "captured into a graph",
                   "after the tile, offset and band checks and before the brick-list checks", "a refused call writes nothing",
                   "the obstacle list is read before the call returns", "noise-space coordinate c_a",
                   "nobs == 0", "launches no kernel of its own", "wn_grid_exact", "wn_grid_default",
                   "wn_eval3d_curl_bounded_points", "wn_multiband3d_curl_bounded_points", "0.0f out_scale",
                   "v_k = a c_k + (g_a psi_b - g_b psi_a)", "a = (k+1) % 3 and b = (k+2) % 3", "separately rounded float32",
                   "the bits of the default-tier wn_eval3d_curl_bricks", "wn_eval3d_grad_bricks", "rolled by potential k's offset",
                   "its pair partner", "the list length",
                   "a t + v (|g_a| + |g_b|) + da |c_k| + dg (|psi_a| + |psi_b|) + 8 2^-24 (a |c_k| + |g_a psi_b| + |g_b psi_a|)",
                   "tests/test_bounded_host.py",
                   "not provided: gradient or value bricks with obstacles; moving obstacles; projected bricks; dense bounded grids; brick edges other than 8"):
        assert phrase in text, phrase
    # the headers this one completes keep their wording and point here
    fields_h = squeeze(os.path.join(ROOT, "include", "wnoise_brick_fields.h"))
    assert "not provided: projected bricks; bounded curl bricks (" in fields_h
    assert "wnoise_bounded_bricks.h" in fields_h[fields_h.index("not provided: projected bricks; bounded curl bricks ("):]
    bounded_h = squeeze(os.path.join(ROOT, "include", "wnoise_bounded.h"))
    assert "dense grids" in bounded_h and "wnoise_bounded_bricks.h" in bounded_h


CHILD = r"""
import ctypes as C, importlib, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import _bounded as B
c = importlib.import_module("wavelet-noise-in-ray-tracing_amd._capi")
lib = c.load()
count = C.c_int(-1)
lib.wn_device_count(C.byref(count))
assert count.value == 0, count.value
g = c.wn_grid(512, 40, 24, 8, 32, 4.0, 16.0, 2.0, 0, 0.0, 1.0, 0)
zc = c.wn_grid(512, 40, 24, 8, 32, 4.0, 16.0, 2.0, 1, 0.0, 1.0, 0)
w = (C.c_float * 2)(1.0, 1.0)
off = (C.c_int32 * 9)(0, 0, 0, 1, 2, 3, 4, 5, 6)
out = np.full(3 * 512, 7.0, np.float32)
bricks = np.zeros(3, np.int32)
op, bp = out.ctypes.data_as(C.c_void_p), bricks.ctypes.data_as(C.c_void_p)
good = [("sphere", (1.0, 2.0, 3.0), 2.0, 1.0), ("container", (0.0, 0.0, 0.0), 9.0, 3.0), ("halfspace", (0.0, 2.0, 0.0), -1.0, 0.5)]
lists = [(B.obstacle_array(good), 3), (None, 0), (B.obstacle_array(good), -1), (B.obstacle_array(B.SETS["sixteen"] + [B.SPHERE]), 17),
         (None, 1)]
for at, field, value in [(0, "kind", 3), (0, "kind", -1), (0, "r", 0.0), (1, "r", -1.0), (0, "d0", 0.0), (2, "d0", -0.5),
                         (0, "r", np.nan), (1, "r", np.inf), (2, "r", np.inf), (0, "d0", np.nan), (1, "d0", np.inf),
                         (2, "c", (0.0, 0.0, 0.0)), (0, "c", (np.nan, 0.0, 0.0)), (1, "c", (0.0, -np.inf, 0.0)),
                         (2, "c", (0.0, 1.0, np.nan)), (0, "reserved", (1, 0)), (2, "reserved", (0, -1))]:
    arr = B.obstacle_array(good)
    setattr(arr[at], field, type(getattr(arr[at], field))(*value) if isinstance(value, tuple) else value)
    lists.append((arr, 3))
codes = set()
calls = 0
for arr, nobs in lists:
    a = C.cast(arr, c._op) if arr is not None else None
    for grid, n, o9, b_, o_ in ((g, 1, off, bp, op), (zc, 1, off, bp, op), (g, 0, off, None, None), (g, 1, off, None, op),
                                (g, 1, off, bp, None), (g, ((1 << 64) - 1) // 512 // 3 + 1, off, bp, op), (g, 1, None, bp, op),
                                (None, 1, off, bp, op)):
        gp = C.byref(grid) if grid is not None else None
        codes.add(lib.wn_eval3d_curl_bounded_bricks(None, gp, b_, n, o9, a, nobs, o_, None))
        codes.add(lib.wn_multiband3d_curl_bounded_bricks(None, gp, b_, n, o9, -16.0, 0, 2, w, 0.18402, a, nobs, o_, None))
        codes.add(lib.wn_multiband3d_curl_bounded_bricks(None, gp, b_, n, o9, -16.0, 0, 9, None, 0.18402, a, nobs, o_, None))
        calls += 3
assert (out == 7.0).all() and (bricks == 0).all()
print("calls", calls, "codes", *sorted(codes), "|", lib.wn_last_error().decode())
"""


def test_without_a_device_every_call_returns_no_device_and_writes_nothing():
    capi()
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    run = subprocess.run([sys.executable, "-c", CHILD, ROOT], capture_output=True, text=True, env=env, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "calls 528 codes 2 |" in run.stdout, run.stdout          # 22 obstacle lists x 8 argument sets x 3: WN_ERR_NO_DEVICE
