"""CPU checks of the bounded Perlin curl brick-list entry point (include/wnoise_perlin_bounded_bricks.h): the header's one
WN_API name, and no other, is exported by libwnoise_hip.so and bound in _capi.py's SIGNATURES_PERLIN_BOUNDED_BRICKS, a table
of its own that shares no name with any other table; the header includes wnoise_perlin_bricks.h and wnoise_perlin_bounded.h;
tests/_graph.py's prototypes() parses it with `stream` last and one output; the header states its contract; the Python
wrapper and the host function exist; the octave loop that csrc/wn_perlin_bricks.hip holds as text of its own is the loop of
wn::perlin_brick_walk (csrc/wn_perlin_brick_walk.hpp), token for token; and without a HIP device every call, refusals included, returns WN_ERR_NO_DEVICE (run
in a child process with the devices hidden, so that it holds on a GPU machine too)."""
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
HEADER = os.path.join(ROOT, "include", "wnoise_perlin_bounded_bricks.h")
NAMES = ["wn_perlin_curl_bounded_bricks"]


def capi():
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(PKG, "libwnoise_hip.so")):
        ge.build()
    return importlib.import_module("wavelet-noise-in-ray-tracing_amd._capi")


def test_the_declared_name_is_exported_and_bound():
    header = open(HEADER).read()
    names = sorted(set(re.findall(r"WN_API\s+[\w\s\*]+?\b(wn_\w+)\s*\(", header)))
    assert names == NAMES, names
    c = capi()
    lib = c.load()
    table = c.SIGNATURES_PERLIN_BOUNDED_BRICKS
    assert set(table) == set(names)
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/wnoise_perlin_bounded_bricks.h but not exported"
        assert getattr(lib, n).argtypes == table[n][1] and getattr(lib, n).restype is table[n][0]
    # a table of its own: no name of it in any other table of _capi.py
    others = [t for t in dir(c) if "SIGNATURES" in t and t != "SIGNATURES_PERLIN_BOUNDED_BRICKS" and isinstance(getattr(c, t), dict)]
    assert len(others) >= 15 and "SIGNATURES_PERLIN_BRICKS" in others and "SIGNATURES_PERLIN_BOUNDED" in others, others
    for other in others:
        assert not set(names) & set(getattr(c, other)), other
    assert '#include "wnoise_perlin_bricks.h"' in header and '#include "wnoise_perlin_bounded.h"' in header
    # the argument list is the unbounded curl bricks' with (obstacles, nobs) before the list
    plain = c.SIGNATURES_PERLIN_BRICKS["wn_perlin_curl_bricks"][1]
    assert table[NAMES[0]][1] == plain[:-4] + [c._op, c._i] + plain[-4:]


def test_the_wrapper_and_the_host_function_exist():
    capi()
    pkg = importlib.import_module("wavelet-noise-in-ray-tracing_amd")
    assert callable(pkg.perlin_curl_bounded_bricks) and "perlin_curl_bounded_bricks" in pkg.__all__
    grid_h = open(os.path.join(PKG, "host", "noise_grid.h")).read()
    assert '#include "wnoise_perlin_bounded_bricks.h"' in grid_h
    assert re.search(r"inline void perlinCurlBoundedBricks\(", grid_h)
    assert os.path.exists(os.path.join(HERE, "host_src", "perlin_bounded_bricks_api_check.cpp"))
    makefile = open(os.path.join(PKG, "Makefile")).read()
    assert "csrc/wn_perlin_bounded_bricks.hip" in makefile and "csrc/wn_perlin_brick_walk.hpp" in makefile


def test_the_header_parses_as_a_call_description():
    protos = G.prototypes([HEADER])
    assert sorted(protos) == NAMES
    params = protos[NAMES[0]]
    assert params == ["perm", "g", "kind", "depth", "offsets9_host", "obstacles_host", "nobs", "bricks_dev", "n", "out_dev", "stream"]
    assert [p for p in params if G.is_output(p)] == ["out_dev"]
    assert [p for p in params if G.is_device_input(p)] == ["bricks_dev"]
    assert [p for p in params if G.is_host(p)] == ["g", "offsets9_host", "obstacles_host"]
    # brick lists stand outside the completeness table of tests/test_gpu_graph_replay.py;
    # tests/test_gpu_perlin_bounded_bricks_graph.py holds this row
    assert not set(NAMES) & G.writers() and set(NAMES) <= G.declared()


def test_the_header_states_its_contract_and_what_is_left_out():
    text = " ".join(open(HEADER).read().replace("*", " ").split()).lower()
    for phrase in ("out_dev[(ch n + i) 512 + lx + 8 (ly + 8 lz)]", "the z index is absolute", "left untouched in all three channels",
                   "as wnoise_perlin_bricks.h states them", "any float-aligned out_dev is accepted", "float4 stores",
                   "g->flags is accepted and ignored", "the sample's float lattice coordinate", "are read before the call returns",
                   "(float) of the matching record of wn_perlin_curl_bounded_points_f32", "times out_scale", "every depth >= 0",
                   "no depth cap", "inside samples are (float)0.0 out_scale", "far samples carry the bits of wn_perlin_curl_bricks",
                   "not on its brick's place in the list", "nobs == 0: the call is wn_perlin_curl_bricks", "a null obstacle list is valid",
                   "offsets9_host == null", "the obstacle checks of wnoise_bounded.h", "also with n == 0", "z_mode == wn_z_const",
                   "n == 0 is wn_ok", "3 n 512 overflowing size_t", "an empty volume is wn_ok without a launch", "wn_err_no_device",
                   "a refused call writes nothing", "no allocation, no synchronisation", "captured into a graph",
                   "not provided: potential-value bricks; gradient or value bricks with obstacles; moving obstacles; dense bounded grids"):
        assert phrase in text, phrase
    # the neighbours point here
    bricks_h = " ".join(open(os.path.join(ROOT, "include", "wnoise_perlin_bricks.h")).read().replace("*", " ").split())
    assert "wnoise_perlin_bounded_bricks.h" in bricks_h[bricks_h.index("Not provided: solid boundaries on the curl bricks"):]
    bounded_h = " ".join(open(os.path.join(ROOT, "include", "wnoise_perlin_bounded.h")).read().replace("*", " ").split())
    assert "wnoise_perlin_bounded_bricks.h" in bounded_h[bounded_h.index("Not provided:"):]


CHILD = r"""
import ctypes as C, importlib, sys
sys.path.insert(0, sys.argv[1])
c = importlib.import_module("wavelet-noise-in-ray-tracing_amd._capi")
lib = c.load()
count = C.c_int(-1)
lib.wn_device_count(C.byref(count))
assert count.value == 0, count.value
g = c.wn_grid(512, 40, 24, 8, 32, 4.0, 16.0, 1.0, 0, 0.0, 1.0, 0)
off = (C.c_int32 * 9)(0, 0, 0, 1, 2, 3, 4, 5, 6)
obs = (c.wn_obstacle * 1)()
obs[0].kind, obs[0].r, obs[0].d0 = 0, 1.0, 0.5
bad = (c.wn_obstacle * 1)()
bad[0].kind, bad[0].r, bad[0].d0 = 7, -1.0, 0.0
fn = lib.wn_perlin_curl_bounded_bricks
codes = [fn(None, C.byref(g), 1, 7, off, obs, 1, None, 1, None, None),        # a valid list
         fn(None, C.byref(g), 1, 7, off, None, 0, None, 1, None, None),       # nobs == 0: the unbounded call
         fn(None, C.byref(g), 3, 7, off, obs, 1, None, 1, None, None),        # refusals: kind, depth, grid, offsets, obstacles
         fn(None, C.byref(g), 1, -1, off, obs, 1, None, 1, None, None),
         fn(None, None, 0, 0, off, obs, 1, None, 1, None, None),
         fn(None, C.byref(g), 0, 0, None, obs, 1, None, 1, None, None),
         fn(None, C.byref(g), 0, 0, off, bad, 1, None, 0, None, None),
         fn(None, C.byref(g), 0, 0, off, obs, 17, None, 0, None, None),
         fn(None, C.byref(g), 0, 0, off, obs, 1, None, 0, None, None)]        # n == 0
print("codes", *codes, "|", lib.wn_last_error().decode())
"""


def test_without_a_device_every_call_returns_no_device():
    capi()
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    run = subprocess.run([sys.executable, "-c", CHILD, ROOT], capture_output=True, text=True, env=env, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "codes 2 2 2 2 2 2 2 2 2 |" in run.stdout, run.stdout     # WN_ERR_NO_DEVICE


def octave_loop(text):
    """The octave loop of a file's walk, from its `#pragma nounroll` to the halving of the weight, without comments and with
    every run of white space as one blank."""
    start = text.index("#pragma nounroll\n", text.index("double weight = 1.0;") if "double weight = 1.0;" in text else 0)
    body = text[start:text.index("weight *= 0.5;", start)]
    body = re.sub(r"//[^\n]*", "", body)
    return " ".join(body.split())


def test_the_two_texts_of_the_walk_are_one_walk():
    """csrc/wn_perlin_bricks.hip holds the octave loop of wn::perlin_brick_walk as text of its own (the nine kernels' assembly
    depends on it).  The two texts must stay the same walk: the header's, with a whole row for its part of a row (NQ = 8,
    q0 = 0), without the potential values of kCurlPsi and with the file's names, is the file's, token for token."""
    walk = octave_loop(open(os.path.join(PKG, "csrc", "wn_perlin_brick_walk.hpp")).read())
    mine = octave_loop(open(os.path.join(PKG, "csrc", "wn_perlin_bricks.hip")).read())
    psi = "if (FIELD == kCurlPsi) { double &sp = s[(6 + k) % NS][q]; sp = (KIND == kNoise) ? nv : sp + weight * nv; } "
    assert walk.count(psi) == 1
    for old, new in ((psi, ""), ("((1u << NQ) - 1u) << q0", "0xffu"), (">> (q0 + q)", ">> q"), ("<< (q0 + q)", "<< q"), ("q0 + q", "q"), ("NQ", "kBrickEdge"),
                     ("kBrickAxisEntries", "kAxisEntries"), ("kIsCurl", "FIELD == kCurl"), ("off[", "a.off[")):
        assert old in walk, old
        walk = walk.replace(old, new)
    assert "q0" not in walk and "kCurlPsi" not in walk
    assert mine.replace("wn::", "") == walk
