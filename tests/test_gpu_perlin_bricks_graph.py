"""The Perlin brick-list entry points (include/wnoise_perlin_bricks.h) are captured into a graph and replayed, bit for bit:
they only enqueue on the caller's stream -- no allocation, no synchronisation, no launch on the null stream, no host read
after the call returns (the curl's offsets9_host included).  As for the wavelet bricks (tests/test_gpu_bricks_graph.py, whose
five steps these are), the names end in _bricks and stand outside the completeness table of tests/test_gpu_graph_replay.py,
so their rows stand here: `bricks_dev` is a device input, `g` and `offsets9_host` are host arguments, `out_dev` is the
output, a tests/_frame.py frame of CH channel arrays.

One graph per row, torch.cuda.graph on one side stream with no environment variable:
  1. eager: the call into a frame; its bits (sentinels of out-of-range slots included) are want_A;
  2. capture: the same call into a second frame; the status is 0 and the frame is still unwritten afterwards;
  3. the host arguments the captured call received are overwritten with other valid values and dropped; an eager call with
     the overwritten values gives other bits than want_A;
  4. replay: the frame equals want_A, guards intact; refilled with the sentinel and replayed, again;
  5. the reversed list is copied into the SAME device tensor: the replay equals an eager call on it (want_B != want_A).
Seven symbols; the lattice is the 1/128 one of tests/test_gpu_perlin_bricks.py for turb and fractal_noise (rows cross cells in
the last octaves) and the baseline one for noise."""
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
import test_gpu_perlin_bricks as tpb  # noqa: E402

# symbol: (channels, depth or None, kind or None)
SYMBOLS = {"wn_perlin_bricks": (1, None, None), "wn_perlin_turb_bricks": (1, 7, None), "wn_perlin_fractal_bricks": (1, None, None),
           "wn_perlin_grad_bricks": (4, None, None), "wn_perlin_turb_grad_bricks": (4, 7, None),
           "wn_perlin_fractal_grad_bricks": (4, None, None), "wn_perlin_curl_bricks": (3, 7, 1)}


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU (the product has no CPU path)"
    return tpb.Env(importlib.import_module("wavelet-noise-in-ray-tracing_amd"))


@pytest.mark.gpu
@pytest.mark.parametrize("symbol", list(SYMBOLS))
def test_replay(env, symbol):
    import torch
    nm = env.nm
    ch, depth, kind = SYMBOLS[symbol]
    n = len(tbr.LIST)
    lattice = tpb.LATTICES[0] if depth is None and "fractal" not in symbol else tpb.LATTICES[1]
    args = {"perm": env.perlins[12345]._h, "g": env.grid(lattice, tbr.BOUNDS), "bricks_dev": None, "n": n, "out_dev": G.Out(ch * 512 * n)}
    if depth is not None:
        args.update(depth=depth)
    if kind is not None:
        args.update(kind=kind, offsets9_host=tpb.c_off())
    sess = G.Session(nm, G.prototypes(), symbol, args)
    assert set(sess.pristine) == {"g"} | ({"offsets9_host"} if kind is not None else set())
    list_a, list_b = tbr.LIST, np.ascontiguousarray(tbr.LIST[::-1])
    dev = torch.from_numpy(list_a).cuda()
    bricks = C.c_void_p(dev.data_ptr())

    def call(frame, host=None):
        return sess.call({"out_dev": frame, "bricks_dev": bricks}, host)

    def result(frame, bricks_host, what):
        return frame.result(written=np.tile(np.repeat(tbr.in_range(bricks_host, tbr.BOUNDS), 512), ch), what=what)

    # 1. eager
    eager = sess.outs["out_dev"].frame()
    assert call(eager) == 0, nm._lib.wn_last_error()
    want_a = result(eager, list_a, "eager")
    # 2. capture
    frame, host = sess.outs["out_dev"].frame(), sess.fresh_host()
    graph, rcs = G.capture([lambda: call(frame, host)])
    assert rcs == [0], (rcs, nm._lib.wn_last_error())
    frame.result(written=np.zeros(ch * 512 * n, bool), what="capture records, it does not run")
    # 3. the host arguments are dead after the call
    for obj in host.values():
        before = bytes(obj)
        G.scribble(obj)
        assert bytes(obj) != before
    G.refill(eager)
    assert call(eager, host) == 0, nm._lib.wn_last_error()
    torch.cuda.synchronize()
    assert (G.bits(eager.tensor.cpu().numpy()) != G.bits(want_a)).any(), "the overwritten host arguments give the original ones' bits"
    host.clear()
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
