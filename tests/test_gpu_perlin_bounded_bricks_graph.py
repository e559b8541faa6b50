"""wn_perlin_curl_bounded_bricks (include/wnoise_perlin_bounded_bricks.h) is captured into a graph and replayed, bit for bit:
it only enqueues on the caller's stream -- no allocation, no synchronisation, no launch on the null stream, no host read after
the call returns (offsets9_host and the obstacle list included).  The five steps are those of
tests/test_gpu_perlin_bricks_graph.py, whose module text describes them; the name ends in _bricks and stands outside the
completeness table of tests/test_gpu_graph_replay.py, so its row stands here: `bricks_dev` is a device input, `g`,
`offsets9_host` and `obstacles_host` are host arguments, `out_dev` is the output, a tests/_frame.py frame of three component
arrays.  turb(7) on the 1/128 lattice of tests/test_gpu_perlin_bricks.py (rows cross cells in the last octaves) with the scene
of tests/test_gpu_perlin_bounded_bricks.py, so the list holds far, near and inside samples.

One graph, torch.cuda.graph on one side stream after an eager warm-up, with no environment variable."""
import ctypes as C
import gc
import importlib
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _graph as G  # noqa: E402
import test_gpu_bricks as tbr  # noqa: E402
import test_gpu_perlin_bounded_bricks as tpbb  # noqa: E402
import test_gpu_perlin_bricks as tpb  # noqa: E402

SYMBOL = "wn_perlin_curl_bounded_bricks"


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU (the product has no CPU path)"
    return tpb.Env(importlib.import_module("wavelet-noise-in-ray-tracing_amd"))


@pytest.mark.gpu
def test_replay(env):
    import torch
    nm = env.nm
    n, ch = len(tbr.LIST), 3
    lattice = tpb.LATTICES[1]
    obstacles, nobs = nm.WaveletNoise._obstacles(tpbb.scene(tpbb.step(lattice)))
    args = {"perm": env.perlins[12345]._h, "g": env.grid(lattice, tbr.BOUNDS), "kind": 1, "depth": 7, "offsets9_host": tpb.c_off(),
            "obstacles_host": obstacles, "nobs": nobs, "bricks_dev": None, "n": n, "out_dev": G.Out(ch * 512 * n)}
    sess = G.Session(nm, G.prototypes(), SYMBOL, args)
    assert set(sess.pristine) == {"g", "offsets9_host", "obstacles_host"}
    list_a, list_b = tbr.LIST, np.ascontiguousarray(tbr.LIST[::-1])
    dev = torch.from_numpy(list_a).cuda()
    bricks = C.c_void_p(dev.data_ptr())

    def call(frame, host=None):
        return sess.call({"out_dev": frame, "bricks_dev": bricks}, host)

    def result(frame, bricks_host, what):
        return frame.result(written=np.tile(np.repeat(tbr.in_range(bricks_host, tbr.BOUNDS), 512), ch), what=what)

    # 1. eager (the warm-up)
    eager = sess.outs["out_dev"].frame()
    assert call(eager) == 0, nm._lib.wn_last_error()
    want_a = result(eager, list_a, "eager")
    # 2. capture
    frame, host = sess.outs["out_dev"].frame(), sess.fresh_host()
    graph, rcs = G.capture([lambda: call(frame, host)])
    assert rcs == [0], (rcs, nm._lib.wn_last_error())
    frame.result(written=np.zeros(ch * 512 * n, bool), what="capture records, it does not run")
    # 3. the host arguments are dead after the call; the obstacle list alone, overwritten, already gives other bits
    only = sess.fresh_host()
    G.scribble(only["obstacles_host"])
    G.refill(eager)
    assert call(eager, only) == 0, nm._lib.wn_last_error()
    assert (G.bits(result(eager, list_a, "other obstacles")) != G.bits(want_a)).any(), "the obstacle list is not read"
    for obj in host.values():
        before = bytes(obj)
        G.scribble(obj)
        assert bytes(obj) != before
    G.refill(eager)
    assert call(eager, host) == 0, nm._lib.wn_last_error()
    torch.cuda.synchronize()
    assert (G.bits(eager.tensor.cpu().numpy()) != G.bits(want_a)).any(), "the overwritten host arguments give the original ones' bits"
    host.clear()
    only.clear()
    gc.collect()
    # 4. replay, twice
    G.replay(graph)
    G.same_bits(result(frame, list_a, "replay"), want_a, "replay against the eager call")
    G.refill(frame)
    G.replay(graph)
    G.same_bits(result(frame, list_a, "second replay"), want_a, "second replay")
    # 5. the reversed list in the same device tensor
    dev.copy_(torch.from_numpy(list_b))
    torch.cuda.synchronize()
    G.refill(frame)
    G.refill(eager)
    assert call(eager) == 0, nm._lib.wn_last_error()
    want_b = result(eager, list_b, "eager on the reversed list")
    assert (G.bits(want_a) != G.bits(want_b)).any()
    G.same_bits(want_b.reshape(ch, n, 512)[:, ::-1], want_a.reshape(ch, n, 512), "the reversed list's slots are the list's, reversed")
    G.replay(graph)
    G.same_bits(result(frame, list_b, "replay on the reversed list"), want_b, "replay on the reversed list")
