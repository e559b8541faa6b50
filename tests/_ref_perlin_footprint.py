"""The independent statement of Perlin turb and fractal_noise with the octave limit taken from a footprint per sample
(include/wnoise_perlin_footprint.h), in numpy, composed from parts that exist without the feature:

    t_i = (s + bias) + i and f_i in float32; octave i runs while t_i < 0; f_i = 1 (hard cut) or min(1, -t_i) (fade);
    turb:    accum += (2^-i * float64(f_i)) * oracle.perlin_noise(perm, float64(p doubled i times in float32)), |accum|;
    fractal: result += oracle.perlin_noise(perm, float64(p) * 2^i) * (2^-i * float64(f_i)), divided by the sum of ALL
             `octaves` amplitudes;
    gradients: sum_i float64(f_i) * (the gradient of the EXISTING host evaluator wnhost_perlin_grad at octave i's point), for
             turb times -1 where accum < 0, for fractal divided by the same sum.

Every float64 operation is a single unfused numpy operation in the order above, so the comparison with the evaluators of
csrc/wn_eval.hpp is bit equality.  With every f_i = 1 this composition reproduces oracle.perlin_turb(depth 7) and
oracle.perlin_fractal bit for bit (checked on 2,000 points in [-40, 40]^3; tests/test_perlin_footprint_host.py repeats it
against the host evaluators).
"""
import ctypes as C

import numpy as np

import oracle

FP, DP, IP = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int)
f32 = np.float32
MAX_OCTAVES = 16


def octave_factors(s, bias, octaves, fade):
    """(active, f): (N, octaves) bool and float32.  f is 0 where the octave does not run."""
    s = np.asarray(s, f32).reshape(-1)
    active = np.zeros((s.size, octaves), bool)
    f = np.zeros((s.size, octaves), f32)
    running = np.ones(s.size, bool)
    with np.errstate(invalid="ignore"):
        for i in range(octaves):
            t = (s + f32(bias)) + f32(i)
            running = running & (t < 0)                       # NaN compares false
            active[:, i] = running
            fi = np.minimum(f32(1.0), -t) if fade else np.ones_like(t)
            f[:, i] = np.where(running, fi, f32(0.0))
    return active, f


def octave_count(s, bias, octaves):
    return octave_factors(s, bias, octaves, 0)[0].sum(1)


def _host_grad(host, perm, pts64):
    """wnhost_perlin_grad at every row of the float64 points: (N, 3) gradients."""
    pp = perm.ctypes.data_as(IP)
    g = np.zeros(3)
    gp = g.ctypes.data_as(DP)
    out = np.empty((len(pts64), 3))
    for j, (x, y, z) in enumerate(pts64.tolist()):
        host.wnhost_perlin_grad(pp, x, y, z, gp)
        out[j] = g
    return out


def turb_footprint(perm, pts, s, depth, bias, fade, host=None):
    """(N, 4) float64 records {value, d/dx, d/dy, d/dz}; without `host` the gradient columns are not formed (NaN)."""
    p = np.array(pts, f32).reshape(-1, 3)
    active, f = octave_factors(s, bias, depth, fade)
    accum = np.zeros(len(p))
    g = np.zeros((len(p), 3))
    for i in range(depth):
        a = active[:, i]
        if a.any():
            q = p[a].astype(np.float64)
            fi = f[a, i].astype(np.float64)
            accum[a] += (2.0 ** -i * fi) * oracle.perlin_noise(perm, q)
            if host is not None:
                g[a] += fi[:, None] * _host_grad(host, perm, q)
        p = p * f32(2.0)
    rec = np.full((len(p), 4), np.nan)
    rec[:, 0] = np.abs(accum)
    if host is not None:
        rec[:, 1:] = np.where((accum < 0.0)[:, None], -g, g)
    return rec


def fractal_footprint(perm, pts, s, octaves, bias, fade, host=None):
    p = np.array(pts, f32).reshape(-1, 3).astype(np.float64)
    active, f = octave_factors(s, bias, octaves, fade)
    result = np.zeros(len(p))
    g = np.zeros((len(p), 3))
    max_value = 0.0
    for i in range(octaves):
        a = active[:, i]
        if a.any():
            q = p[a] * 2.0 ** i
            fi = f[a, i].astype(np.float64)
            result[a] += oracle.perlin_noise(perm, q) * (2.0 ** -i * fi)
            if host is not None:
                g[a] += fi[:, None] * _host_grad(host, perm, q)
        max_value += 2.0 ** -i
    rec = np.full((len(p), 4), np.nan)
    if octaves == 0:
        rec[:] = 0.0
        return rec
    rec[:, 0] = result / max_value
    if host is not None:
        rec[:, 1:] = g / max_value
    return rec


def texture_grey(n):
    """(float)(0.5 * (1.0 + n)) of the float64 noise values n."""
    return (0.5 * (1.0 + np.asarray(n, np.float64))).astype(f32)


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def footprints(octaves, bias, count, seed):
    """`count` float32 footprints: -inf, +inf, NaN; the thresholds of every octave and their float32 neighbours; values that
    leave 0, 1, ..., octaves octaves; integer-valued s + bias; uniform ones over the whole range -- shuffled, every special
    value at least once."""
    rng = np.random.default_rng(seed)
    special = [-np.inf, np.inf, np.nan, 0.0, -0.0, 1e-30, -1e-30, -100.0, 100.0]
    for i in range(max(octaves, 1)):
        thr = f32(-i - bias)
        special += [thr, np.nextafter(thr, f32(-np.inf)), np.nextafter(thr, f32(np.inf)), thr - f32(0.5), thr - f32(0.25),
                    thr - f32(0.999), thr + f32(0.25)]
    for c in range(octaves + 1):
        special.append(f32(-c + 0.5 - bias))
    special = np.array(special, f32)
    lo, hi = -octaves - 1.5 - bias, 1.5 - bias
    uniform = rng.uniform(lo, hi, count).astype(f32)
    integers = (rng.integers(-octaves - 2, 3, count) - bias).astype(f32)
    pick = rng.integers(0, 3, count)
    s = np.where(pick == 0, rng.choice(special, count), np.where(pick == 1, uniform, integers)).astype(f32)
    s[:min(count, special.size)] = special[:count]
    return s[rng.permutation(count)]


def points(count, seed):
    """`count` float32 points: four fifths uniform in [-40, 40]^3, one fifth on and next to cell faces (face_points)."""
    import _ref64_perlin_grad
    rng = np.random.default_rng(seed)
    faces = count // 5
    p = np.concatenate([rng.uniform(-40.0, 40.0, (count - faces, 3)), _ref64_perlin_grad.face_points(rng, faces)])
    return np.ascontiguousarray(p[rng.permutation(count)].astype(f32))


# ---- the host evaluators (libwnoise_host.so) -------------------------------------------------------------------------------
def bind_host(lib):
    for name, args in (("wnhost_perlin_grad", [IP, C.c_double, C.c_double, C.c_double, DP]),
                       ("wnhost_perlin_turb", [IP, FP, C.c_int]), ("wnhost_perlin_turb_grad", [IP, FP, C.c_int, DP]),
                       ("wnhost_perlin_fractal", [IP, FP]), ("wnhost_perlin_fractal_grad", [IP, FP, DP]),
                       ("wnhost_perlin_turb_footprint", [IP, FP, C.c_int, C.c_float, C.c_float, C.c_int, DP]),
                       ("wnhost_perlin_fractal_footprint", [IP, FP, C.c_int, C.c_float, C.c_float, C.c_int, DP])):
        getattr(lib, name).restype = C.c_double
        getattr(lib, name).argtypes = args
    lib.wnhost_noise_multiband_texture_value.restype = C.c_float
    lib.wnhost_noise_multiband_texture_value.argtypes = [IP, C.c_double, C.c_int, C.c_float, C.c_int, FP, C.c_float]
    return lib


def host_footprint(lib, perm, kind, pts, s, octaves, bias, fade):
    """wnhost_perlin_turb_footprint (kind "turb") / _fractal_footprint ("fractal") at every point: ((N, 4) float64 of the
    gradient form, (N,) float64 of the value form)."""
    fn = lib.wnhost_perlin_turb_footprint if kind == "turb" else lib.wnhost_perlin_fractal_footprint
    pp = perm.ctypes.data_as(IP)
    pts = np.ascontiguousarray(pts, f32)
    s = np.asarray(s, f32)
    out = np.empty((len(pts), 4))
    val = np.empty(len(pts))
    g = np.zeros(3)
    gp = g.ctypes.data_as(DP)
    for i in range(len(pts)):
        q = pts[i].ctypes.data_as(FP)
        out[i, 0] = fn(pp, q, octaves, s[i], bias, fade, gp)
        out[i, 1:] = g
        val[i] = fn(pp, q, octaves, s[i], bias, fade, None)
    return out, val


def host_texture(lib, perm, scale, pts, s, octaves, bias, fade):
    pp = perm.ctypes.data_as(IP)
    pts = np.ascontiguousarray(pts, f32)
    s = np.asarray(s, f32)
    return np.array([lib.wnhost_noise_multiband_texture_value(pp, scale, octaves, bias, fade, pts[i].ctypes.data_as(FP), s[i])
                     for i in range(len(pts))], f32)
