"""CPU checks of the brick-list entry points (include/wnoise_bricks.h): every WN_API name of the header is exported by
libwnoise_hip.so and bound in _capi.py; tests/_graph.py's prototypes() parses the header with `stream` last and one output;
the header states its brick edge, its argument checks and what it leaves out; and without a HIP device both calls return
WN_ERR_NO_DEVICE (run in a child process with the devices hidden, so that it holds on a GPU machine too)."""
import ctypes as C
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
HEADER = os.path.join(ROOT, "include", "wnoise_bricks.h")
NAMES = ["wn_eval3d_bricks", "wn_multiband3d_bricks"]


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
        assert hasattr(lib, n), f"{n} declared in include/wnoise_bricks.h but not exported"
        assert getattr(lib, n).argtypes == c.BRICKS_SIGNATURES[n][1]
    assert set(c.BRICKS_SIGNATURES) == set(names)
    for other in ("SIGNATURES", "ADVECT_SIGNATURES", "BOUNDED_SIGNATURES", "CURL2D_SIGNATURES", "BOUNDED2D_SIGNATURES"):
        assert not set(names) & set(getattr(c, other)), other
    assert re.search(r"#define WN_BRICK\s+8\b", header) and c.WN_BRICK == 8
    assert '#include "wnoise.h"' in header


def test_the_header_parses_as_a_call_description():
    protos = G.prototypes([HEADER])
    assert sorted(protos) == NAMES
    assert protos["wn_eval3d_bricks"] == ["tile3d", "g", "bricks_dev", "n", "out_dev", "stream"]
    assert protos["wn_multiband3d_bricks"] == ["tile3d", "g", "bricks_dev", "n", "s", "first_band", "nbands", "w_host",
                                               "var_per_band", "out_dev", "stream"]
    for name, params in protos.items():
        assert params[-1] == "stream" and [p for p in params if G.is_output(p)] == ["out_dev"], name
        assert [p for p in params if G.is_device_input(p)] == ["bricks_dev"], name
        assert [p for p in params if G.is_host(p)] == (["g"] if name == NAMES[0] else ["g", "w_host"]), name
    # a brick list is neither a grid nor a point list: the completeness table of tests/test_gpu_graph_replay.py does not
    # see these names, and tests/test_gpu_bricks_graph.py holds their rows
    assert not set(NAMES) & G.writers() and set(NAMES) <= G.declared()


def test_the_header_states_its_contract_and_what_is_left_out():
    text = " ".join(open(HEADER).read().replace("*", " ").split()).lower()
    for phrase in ("out_dev[512 i + lx + 8 (ly + 8 lz)]", "left untouched", "duplicates are allowed", "wn_grid_exact",
                   "within 1e-5", "wn_z_const", "n == 0 is wn_ok", "overflowing size_t", "wn_err_no_device",
                   "no allocation, no synchronisation", "not provided: gradient, curl and projected bricks",
                   "brick edges other than 8", "from a mask"):
        assert phrase in text, phrase


CHILD = r"""
import ctypes as C, importlib, sys
sys.path.insert(0, sys.argv[1])
c = importlib.import_module("wavelet-noise-in-ray-tracing_amd._capi")
lib = c.load()
count = C.c_int(-1)
lib.wn_device_count(C.byref(count))
assert count.value == 0, count.value
g = c.wn_grid(512, 40, 24, 8, 32, 4.0, 16.0, 2.0, 0, 0.0, 1.0, 0)
w = (C.c_float * 2)(1.0, 1.0)
a = lib.wn_eval3d_bricks(None, C.byref(g), None, 1, None, None)
ea = lib.wn_last_error().decode()
b = lib.wn_multiband3d_bricks(None, C.byref(g), None, 1, -16.0, 0, 2, w, 0.18402, None, None)
print("codes", a, b, "|", ea)
"""


def test_without_a_device_both_calls_return_no_device():
    capi()
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    run = subprocess.run([sys.executable, "-c", CHILD, ROOT], capture_output=True, text=True, env=env, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "codes 2 2 |" in run.stdout, run.stdout          # WN_ERR_NO_DEVICE
