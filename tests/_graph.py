"""Helpers of tests/test_gpu_graph_replay.py: one C-ABI call described by parameter name, so that the same description can be
called eagerly, captured into a graph, have its host arguments overwritten, and be replayed on other device inputs.

prototypes() parses every header under include/: {entry point: [parameter names]}.  A parameter's name says what it is:
  * `stream`                                   the stream that is current when the call is made;
  * OUTPUTS (`out_dev`, `out4_dev`, `grey_dev`, `xyz_out_dev`, `traj_dev`, ...)  a tests/_frame.py Frame, described by an Out;
  * any other `*_dev`                          a device input: a host array that Session copies to a device tensor ONCE
                                               (before any capture), or None;
  * `*_host`, `g`, `a`, `normal`               a host argument: a ctypes array or structure, or None;
  * everything else                            a handle or a scalar, passed as it is.
Session keeps a pristine copy of every host argument (fresh_host()), so that the ones a captured call received can be
overwritten (scribble) and dropped while later eager calls still get the original values.
"""
import ctypes as C
import os
import re

import numpy as np

from _frame import SENTINEL_BITS, SENTINEL_BITS64, Frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
DECLARED = re.compile(r"WN_API int (wn_\w+)\(")
WRITER = re.compile(r"_(grid|points|points_vec3)$")
OUTPUTS = ("out_dev", "out2_dev", "out3_dev", "out4_dev", "grey_dev", "xyz_out_dev", "xy_out_dev", "traj_dev")
HOST_NAMES = ("g", "a", "normal")


def headers():
    return [os.path.join(INCLUDE, n) for n in sorted(os.listdir(INCLUDE)) if n.endswith(".h")]


def declared(paths=None):
    """Every name a header declares as `WN_API int wn_*(`."""
    names = []
    for path in paths or headers():
        with open(path) as f:
            names += DECLARED.findall(f.read())
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    return set(names)


def writers(paths=None):
    """The declared entry points that write a device buffer the caller owns."""
    return {n for n in declared(paths) if WRITER.search(n)}


def prototypes(paths=None):
    """{entry point: [parameter names, in order]}."""
    out = {}
    for path in paths or headers():
        with open(path) as f:
            text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
        for m in re.finditer(r"WN_API int (wn_\w+)\(([^;{]*?)\)\s*;", text, re.S):
            params = [p.strip() for p in m.group(2).split(",")]
            out[m.group(1)] = [re.search(r"(\w+)\s*(?:\[\d*\])?$", p).group(1) for p in params if p != "void"]
    return out


def is_output(name):
    return name in OUTPUTS


def is_device_input(name):
    return name.endswith("_dev") and name not in OUTPUTS


def is_host(name):
    return name.endswith("_host") or name in HOST_NAMES


class Out:
    """An output buffer: `count` elements of `dtype`, `back_extra` more guard elements behind it; `written_by`: the name of
    the uint8 device input (an active mask) whose non-zero entries say which of the `count` elements are written."""

    def __init__(self, count, dtype=np.float32, back_extra=0, written_by=None):
        self.count, self.dtype, self.back_extra, self.written_by = int(count), np.dtype(dtype), int(back_extra), written_by

    def frame(self):
        return Frame(self.count, 0, back_extra=self.back_extra, dtype=self.dtype)


def floats(values):
    values = [float(v) for v in values]
    return (C.c_float * max(1, len(values)))(*values)


def int32s(values):
    values = [int(v) for v in np.asarray(values).reshape(-1)]
    return (C.c_int32 * len(values))(*values)


def copy_of(obj):
    return None if obj is None else type(obj).from_buffer_copy(obj)


def scribble(obj):
    """Overwrite a host argument in place with OTHER VALID values: a call that still read it would compute something else
    (and, where a lattice or a step count shrinks, write less), never fault."""
    if isinstance(obj, C.Array):
        if issubclass(obj._type_, C.Structure):
            for e in obj:
                scribble(e)
        elif obj._type_ is C.c_float:
            for i in range(len(obj)):
                obj[i] = obj[i] * 0.5 + 0.25
        else:
            assert obj._type_ is C.c_int32, obj._type_
            for i in range(len(obj)):
                obj[i] = obj[i] + 17
        return
    assert isinstance(obj, C.Structure), type(obj)
    fields = {f[0] for f in obj._fields_}
    if "nx" in fields:                       # wn_grid: a one-sample lattice elsewhere
        obj.nx = obj.ny = 1
        obj.z1 = obj.z0 + 1
        obj.octave_scale *= 2.0
        obj.out_scale *= 0.5
    elif "steps" in fields:                  # wn_advect, wn_advect2d
        obj.steps, obj.traj_every = 1, 0
        obj.h *= -0.5
        obj.gain += 1.0
        scribble(obj.drift)
    else:                                    # wn_obstacle, wn_obstacle2d: the same kinds, other shapes
        assert "d0" in fields, fields
        obj.r = obj.r * 0.5 + 1.0 if obj.kind != 2 else obj.r + 10.0
        obj.d0 *= 0.5
        scribble(obj.c)


def refill(frame):
    """Every element of the frame holds the sentinel again."""
    import torch
    if frame.dtype.itemsize == 8:
        frame.buf.view(torch.int64).fill_(int(np.uint64(SENTINEL_BITS64).view(np.int64)))
    else:
        frame.buf.view(torch.int32).fill_(int(np.uint32(SENTINEL_BITS).view(np.int32)))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32).reshape(-1)


def same_bits(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, f"{what}: {bad.size} of {g.size} elements differ, first at index {int(bad[0])}"


class Session:
    """One entry point with its arguments.  `args`: {parameter name: value} as the module docstring describes them."""

    def __init__(self, nm, names, symbol, args):
        import torch
        self.nm, self.symbol, self.fn, self.names = nm, symbol, getattr(nm._lib, symbol), names[symbol]
        assert set(args) == set(self.names) - {"stream"}, (symbol, set(args) ^ (set(self.names) - {"stream"}))
        self.outs = {k: v for k, v in args.items() if is_output(k) and v is not None}
        assert all(isinstance(v, Out) for v in self.outs.values()), symbol
        self.inputs = {k: np.ascontiguousarray(v) for k, v in args.items() if is_device_input(k) and v is not None}
        for k, v in self.inputs.items():      # the element type the header declares: a shorter one would be read past its end
            want = ("uint8",) if k == "active_dev" else ("float32",) if k in ("s_dev", "normals_dev") else ("float32", "float64")
            assert v.dtype.name in want, (symbol, k, v.dtype)
        self.dev = {k: torch.from_numpy(v).cuda() for k, v in self.inputs.items()}
        self.pristine = {k: v for k, v in args.items() if is_host(k) and v is not None}
        assert all(isinstance(v, (C.Array, C.Structure)) for v in self.pristine.values()), symbol
        self.plain = {k: v for k, v in args.items() if not (is_output(k) or is_device_input(k) or is_host(k))}
        self.null = {k for k, v in args.items() if v is None}

    def fresh_host(self):
        return {k: copy_of(v) for k, v in self.pristine.items()}

    def frames(self):
        return {k: o.frame() for k, o in self.outs.items()}

    def call(self, ptrs, host=None):
        """The status of one call on the current stream.  `ptrs`: {parameter: Frame or c_void_p} for the outputs (and for
        any device input that is to come from elsewhere than this session's tensors)."""
        host = self.fresh_host() if host is None else host
        argv = []
        for name in self.names:
            if name == "stream":
                argv.append(self.nm._stream())
            elif name in ptrs:
                argv.append(ptrs[name].ptr if isinstance(ptrs[name], Frame) else ptrs[name])
            elif name in self.dev:
                argv.append(C.c_void_p(self.dev[name].data_ptr()))
            elif name in host:
                argv.append(host[name])
            elif name in self.null:
                argv.append(None)
            else:
                argv.append(self.plain[name])
        return self.fn(*argv)

    def load(self, inputs):
        """Copy another input set into the SAME device tensors."""
        import torch
        for k, v in inputs.items():
            v = np.ascontiguousarray(v)
            assert v.shape == self.inputs[k].shape and v.dtype == self.inputs[k].dtype, k
            self.dev[k].copy_(torch.from_numpy(v))
        torch.cuda.synchronize()

    def written(self, name, inputs):
        """The mask of elements of output `name` that a call on `inputs` writes (None: all)."""
        by = self.outs[name].written_by
        return None if by is None else np.asarray(inputs[by]).reshape(-1) != 0

    def results(self, frames, inputs, what):
        return {k: f.result(written=self.written(k, inputs), what=f"{what} {k}") for k, f in frames.items()}

    def eager(self, frames, inputs, what):
        rc = self.call(frames)
        assert rc == 0, (what, rc, self.nm._lib.wn_last_error())
        return self.results(frames, inputs, what)


def capture(calls):
    """Capture the zero-argument callables, in order, on one side stream: a linear chain of nodes.  Returns the graph and
    their statuses; an invalidated capture raises when it ends."""
    import torch
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            rcs = [c() for c in calls]
    torch.cuda.synchronize()
    return graph, rcs


def replay(graph):
    import torch
    graph.replay()
    torch.cuda.synchronize()
