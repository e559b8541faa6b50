// wn_wavelet_advect.hip -- particles moved through the curl noise of 3-D wavelet noise potentials (include/wnoise_advect.h).
//
// The velocity is wn_wavelet_curl.hip's point evaluator, wn::eval3d_curl_exact / multiband_curl_exact; the trace of a
// particle through a launch (wn::advect_trace) and the chain of launches of a call (wn::advect_chain) are wn_advect.hpp's,
// stated once for every advection kernel and for the host's wnhost_eval3d_curl_advect.
//
//   curl3d_advect_kernel<PADDED, MB, METHOD>   one particle per lane in a grid-stride loop: the position is loaded once,
//                                              the steps of the launch run on registers (position, stage point, RK4's
//                                              running sum), a trajectory snapshot is three float stores to the
//                                              time-major address, the final position one more store.  No LDS, no
//                                              private segment.
//
// A launch integrates at most kAdvectLaunchSteps steps; a longer trace is a chain of launches on the stream.
#include "wn_internal.hpp"
#include "wnoise_advect.h"

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
    wn::AdvectTrace<float, 3> t; // xyz interleaved
};

template <bool PADDED, bool MB, int METHOD>
__global__ __launch_bounds__(256) void curl3d_advect_kernel(const AdvectArgs a)
{
    const auto velocity = [&](const float q[3], float v[3]) {
        if (MB) wn::multiband_curl_exact<PADDED>(a.e, q, v);
        else wn::eval3d_curl_exact<PADDED>(a.e.coef, a.e.n, a.e.nmask, a.e.off, q[0], q[1], q[2], v);
    };
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.t.count; i += (size_t)gridDim.x * blockDim.x) {
        float p[3] = {a.t.in[3 * i], a.t.in[3 * i + 1], a.t.in[3 * i + 2]};
        wn::advect_trace<METHOD>(a.t, p, 3 * i, velocity, [&](float *dst) {
            dst[0] = p[0];
            dst[1] = p[1];
            dst[2] = p[2];
        });
    }
}

// The entry points after their tile, offset and band checks: the checks of `adv` and of the three buffers, then the chain of
// launches.
int advect_points(const wn_tile *tile, const CurlEval &e, const float *in_dev, size_t n, const wn_advect *adv, float *out_dev,
                  float *traj_dev, hipStream_t stream)
{
    int rc = wn::check_advect(adv);
    if (rc || n == 0) return rc;
    rc = wn::check_advect_buffers<float, 3>(in_dev, out_dev, traj_dev, n, adv->traj_every, "xyz_in_dev", "xyz_out_dev");
    if (rc) return rc;
    const dim3 grid(wn::stride_blocks(n, kAdvectBlockCap)), block(256);
    const auto launch_one = [&](const wn::AdvectTrace<float, 3> &t) -> int {
        const AdvectArgs a{e, t};
        wn::with_curl_form(tile, e, [&](auto padded, auto mb) {
            wn::with_advect_method(adv->method, [&](auto method) {
                constexpr bool kPadded = decltype(padded)::value, kMb = decltype(mb)::value;
                hipLaunchKernelGGL((curl3d_advect_kernel<kPadded, kMb, decltype(method)::value>), grid, block, 0, stream, a);
            });
        });
        WN_LAUNCH_CHECK("curl3d_advect_kernel");
        return WN_OK;
    };
    return wn::advect_chain(wn::advect_trace_fill<float, 3>(*adv, n), in_dev, out_dev, traj_dev, adv->steps, kAdvectLaunchSteps,
                            launch_one);
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
