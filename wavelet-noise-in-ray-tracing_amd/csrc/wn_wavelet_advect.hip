// wn_wavelet_advect.hip -- particles moved through the curl noise of 3-D wavelet noise potentials (include/wnoise_advect.h).
//
// The velocity is wn_wavelet_curl.hip's point evaluator, wn::eval3d_curl_exact / multiband_curl_exact; the time step is
// wn::advect_step (wn_eval.hpp), stated once for this kernel and for the host's wnhost_eval3d_curl_advect.
//
//   curl3d_advect_kernel<PADDED, MB, METHOD>   one particle per lane in a grid-stride loop: the position is loaded once,
//                                              the steps of the launch run on registers (position, stage point, RK4's
//                                              running sum), a trajectory snapshot is three float stores to the
//                                              time-major address, the final position one more store.  No LDS, no
//                                              private segment.
//
// A launch integrates at most kAdvectLaunchSteps steps; a longer trace is a chain of launches on the stream, each reading
// the positions the one before wrote to xyz_out_dev.  A position crosses a launch boundary as the three floats it is, so
// the bits do not depend on where the boundaries fall.
#include "wn_internal.hpp"
#include "wnoise_advect.h"

#include <algorithm>
#include <cmath>

namespace {

using wn::CurlEval;

// A launch on a card that others share must end: a launch integrates at most this many steps.
// Measured on one MI355X, 16 M particles uniform in a 128-cell box, tile 128 (profiles/advect_kernels.txt): one RK4 step
// takes 16.1 ms with single-band potentials (midpoint 8.1 ms, Euler 4.1 ms; sorted by cell 1.9 ms) and 77.7 ms with five
// bands (sorted 14.9 ms).  Three steps keep a single-band launch at 48 ms or less; a five-band RK4 launch on that list
// takes 233 ms, and a launch's time grows with the list and the band count, not with the length of the trace.  A launch
// boundary costs one 24-byte position round trip per particle, 0.1 ms on that list.
constexpr int kAdvectLaunchSteps = 3;

constexpr size_t kAdvectBlockCap = 256u * 8u; // of the curl point kernel's: the lanes hold 27 row loads each

struct AdvectArgs {
    CurlEval e;
    const float *in; // xyz interleaved
    float *out;      // the positions after this launch's steps
    float *snap;     // every != 0: the first snapshot this launch writes
    size_t count;
    int nsteps;      // of this launch
    int every;       // 0: no trajectory
    int until;       // steps until the next snapshot, in 1..every
    int snap_input;  // the launch stores its input as a snapshot first (the call's snapshot 0)
    float h, h2, h6, gain, drift[3];
};

template <bool PADDED, bool MB, int METHOD>
__global__ __launch_bounds__(256) void curl3d_advect_kernel(const AdvectArgs a)
{
    const auto velocity = [&](const float q[3], float v[3]) {
        if (MB) wn::multiband_curl_exact<PADDED>(a.e, q, v);
        else wn::eval3d_curl_exact<PADDED>(a.e.coef, a.e.n, a.e.nmask, a.e.off, q[0], q[1], q[2], v);
    };
    const size_t snap_stride = 3 * a.count;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.count; i += (size_t)gridDim.x * blockDim.x) {
        float p[3] = {a.in[3 * i], a.in[3 * i + 1], a.in[3 * i + 2]};
        float *snap = a.snap + 3 * i; // not dereferenced unless every != 0
        auto store = [&](float *dst) {
            dst[0] = p[0];
            dst[1] = p[1];
            dst[2] = p[2];
        };
        if (a.snap_input) {
            store(snap);
            snap += snap_stride;
        }
        int until = a.until;
#pragma unroll 1
        for (int t = 0; t < a.nsteps; ++t) {
            wn::advect_step<METHOD>(p, a.h, a.h2, a.h6, a.gain, a.drift, velocity);
            if (a.every && --until == 0) {
                store(snap);
                snap += snap_stride;
                until = a.every;
            }
        }
        store(a.out + 3 * i);
    }
}

template <bool PADDED, bool MB>
void launch_method(int method, dim3 grid, hipStream_t stream, const AdvectArgs &a)
{
    const dim3 block(256);
    if (method == WN_ADVECT_EULER) hipLaunchKernelGGL((curl3d_advect_kernel<PADDED, MB, WN_ADVECT_EULER>), grid, block, 0, stream, a);
    else if (method == WN_ADVECT_MIDPOINT)
        hipLaunchKernelGGL((curl3d_advect_kernel<PADDED, MB, WN_ADVECT_MIDPOINT>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((curl3d_advect_kernel<PADDED, MB, WN_ADVECT_RK4>), grid, block, 0, stream, a);
}

// The entry points after their tile, offset and band checks: the checks of `a` and of the three buffers, then the chain of
// launches.
int advect_points(const wn_tile *tile, const CurlEval &e, const float *in_dev, size_t n, const wn_advect *adv, float *out_dev,
                  float *traj_dev, hipStream_t stream)
{
    const int rc = wn::check_advect(adv);
    if (rc || n == 0) return rc;
    if (!in_dev || !out_dev) return wn::fail(WN_ERR_INVALID, "xyz_in_dev / xyz_out_dev is NULL");
    const int every = adv->traj_every;
    if (every && !traj_dev) return wn::fail(WN_ERR_INVALID, "traj_dev is NULL with traj_every = %d", every);
    const uintptr_t in_b = reinterpret_cast<uintptr_t>(in_dev), out_b = reinterpret_cast<uintptr_t>(out_dev);
    const size_t bytes = 3 * n * sizeof(float);
    if (in_b != out_b && in_b < out_b + bytes && out_b < in_b + bytes)
        return wn::fail(WN_ERR_INVALID, "xyz_out_dev overlaps xyz_in_dev without being equal to it");

    AdvectArgs a{};
    a.e = e;
    a.out = out_dev;
    a.count = n;
    a.every = every;
    a.h = adv->h;
    a.h2 = 0.5f * adv->h;
    a.h6 = adv->h / 6.0f;
    a.gain = adv->gain;
    std::copy(adv->drift, adv->drift + 3, a.drift);
    const dim3 grid(wn::stride_blocks(n, kAdvectBlockCap));
    const bool padded = tile->dev_padded != nullptr;
    int done = 0;
    do { // steps == 0: one launch, which copies the input
        a.in = done ? out_dev : in_dev;
        a.nsteps = std::min(kAdvectLaunchSteps, adv->steps - done);
        a.snap_input = every && done == 0;
        a.until = every ? every - done % every : 0;
        // snapshot done / every is written (the input, or by the launch before this one); the next one is this launch's
        a.snap = every ? traj_dev + (size_t)(done / every + (done ? 1 : 0)) * 3 * n : nullptr;
        if (e.mb) {
            if (padded) launch_method<true, true>(adv->method, grid, stream, a);
            else launch_method<false, true>(adv->method, grid, stream, a);
        } else {
            if (padded) launch_method<true, false>(adv->method, grid, stream, a);
            else launch_method<false, false>(adv->method, grid, stream, a);
        }
        WN_LAUNCH_CHECK("curl3d_advect_kernel");
        done += a.nsteps;
    } while (done < adv->steps);
    return WN_OK;
}

} // namespace

using namespace wn;

extern "C" {

int wn_eval3d_curl_advect_points(const wn_tile *tile, const float *xyz_in_dev, size_t n, const int32_t *offsets9_host,
                                 const wn_advect *a, float *xyz_out_dev, float *traj_dev, void *stream)
{
    WN_ENTRY();
    CurlEval e;
    const int rc = curl_eval_args(tile, offsets9_host, "wn_eval3d_curl_advect_points", &e);
    if (rc) return rc;
    return advect_points(tile, e, xyz_in_dev, n, a, xyz_out_dev, traj_dev, as_stream(stream));
}

int wn_multiband3d_curl_advect_points(const wn_tile *tile, const float *xyz_in_dev, size_t n, const int32_t *offsets9_host,
                                      float s, int first_band, int nbands, const float *w_host, float var_per_band,
                                      const wn_advect *a, float *xyz_out_dev, float *traj_dev, void *stream)
{
    WN_ENTRY();
    CurlEval e;
    int rc = curl_eval_args(tile, offsets9_host, "wn_multiband3d_curl_advect_points", &e);
    if (rc) return rc;
    rc = multiband_bands(s, first_band, nbands, w_host, var_per_band, &e);
    if (rc) return rc;
    e.mb = 1;
    return advect_points(tile, e, xyz_in_dev, n, a, xyz_out_dev, traj_dev, as_stream(stream));
}

int wn_advect_launch_steps(void) { return kAdvectLaunchSteps; }

} // extern "C"
