// wn_advect.hpp -- a particle's trace through a velocity field, stated once for the six advection kernels (wn_wavelet_advect,
// wn_wavelet_bounded, wn_perlin_advect, wn_perlin_bounded, wn_wavelet_curl2d, wn_wavelet_bounded2d .hip) and for the host's wnhost_*_advect
// (host/scalar_eval.cpp): the steps of one launch with their trajectory snapshots (advect_trace, around wn::advect_step of
// wn_eval.hpp), and the chain that cuts a call's trace into launches (advect_chain).  A field supplies its velocity functor
// and its steps-per-launch rule.  Like wn_eval.hpp, no HIP header: a plain C++ compiler includes it.
#pragma once

#include <cstddef>
#include <type_traits>

#include "wn_eval.hpp"
#include "wnoise_advect.h"

namespace wn {

// One launch's part of a trace of `count` particles of D components of T (float: the wavelet potentials; double: Perlin).
template <typename T, int D>
struct AdvectTrace {
    const T *in;    // components interleaved
    T *out;         // the positions after this launch's steps
    T *snap;        // every != 0: the first snapshot this launch writes, a plane of D * count values; time-major
    size_t count;
    int nsteps;     // of this launch
    int every;      // 0: no trajectory
    int until;      // steps until the next snapshot, in 1..every
    int snap_input; // the launch stores its input as a snapshot first (the call's snapshot 0)
    T h, h2, h6, gain, drift[D];
};

// The trace of one particle: p[D] holds its position, loaded by the caller, and is advanced in place by t.nsteps steps.
// store(dst) writes p; the addresses handed to it lie `at` values into a plane of D * t.count values: the snapshots
// t.snap + k * D * t.count in time order, then t.out.  `at` is the particle's own place, D * i, where a lane keeps a running
// snapshot pointer (the four plain kernels: their register counts are those of this form), or the place of a span of
// particles, the same for every lane, where store adds the lane's part (the bounded 2-D kernel); the host passes 0.
template <int METHOD, int D, typename T, typename V, typename S>
WN_EVAL_FN void advect_trace(const AdvectTrace<T, D> &t, T p[D], size_t at, const V &velocity, const S &store)
{
    const size_t snap_stride = (size_t)D * t.count;
    T *snap = t.snap + at; // not dereferenced unless every != 0
    if (t.snap_input) {
        store(snap);
        snap += snap_stride;
    }
    int until = t.until;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (int s = 0; s < t.nsteps; ++s) {
        advect_step<METHOD, D, T>(p, t.h, t.h2, t.h6, t.gain, t.drift, velocity);
        if (t.every && --until == 0) {
            store(snap);
            snap += snap_stride;
            until = t.every;
        }
    }
    store(t.out + at);
}

// Stage velocities of one step.
inline int advect_stages(int method) { return method == WN_ADVECT_EULER ? 1 : (method == WN_ADVECT_MIDPOINT ? 2 : 4); }

// f(std::integral_constant<int, METHOD>) for the runtime `method`, which the caller has checked.
template <typename F>
inline auto with_advect_method(int method, const F &f)
{
    switch (method) {
    case WN_ADVECT_EULER: return f(std::integral_constant<int, WN_ADVECT_EULER>{});
    case WN_ADVECT_MIDPOINT: return f(std::integral_constant<int, WN_ADVECT_MIDPOINT>{});
    default: return f(std::integral_constant<int, WN_ADVECT_RK4>{});
    }
}

// The fields of a trace that every launch of a call shares, from its wn_advect / wn_advect2d: converted to T first, the
// arithmetic in T.
template <typename T, int D, typename A>
inline AdvectTrace<T, D> advect_trace_fill(const A &adv, size_t count)
{
    AdvectTrace<T, D> t{};
    t.count = count;
    t.every = adv.traj_every;
    t.h = (T)adv.h;
    t.h2 = T(0.5) * t.h;
    t.h6 = t.h / T(6);
    t.gain = (T)adv.gain;
    for (int c = 0; c < D; ++c) t.drift[c] = (T)adv.drift[c];
    return t;
}

// A call's trace of `steps` steps as launches of at most per_launch steps, each reading the positions the one before
// wrote to `out`; launch_one(trace) returns a status, and the first that is not 0 ends the chain.  steps == 0 is one launch,
// which copies the input.  A position crosses a launch boundary as the D values it is, so the bits do not depend on where
// the cuts fall.
template <typename T, int D, typename L>
inline int advect_chain(AdvectTrace<T, D> t, const T *in, T *out, T *traj, int steps, int per_launch, const L &launch_one)
{
    const int every = t.every;
    t.out = out;
    int done = 0;
    do {
        t.in = done ? out : in;
        t.nsteps = per_launch < steps - done ? per_launch : steps - done;
        t.snap_input = every && done == 0;
        t.until = every ? every - done % every : 0;
        // snapshot done / every is written (the input, or by the launch before this one); the next one is this launch's
        t.snap = every ? traj + (size_t)(done / every + (done ? 1 : 0)) * D * t.count : nullptr;
        if (const int rc = launch_one(t)) return rc;
        done += t.nsteps;
    } while (done < steps);
    return 0;
}

} // namespace wn
