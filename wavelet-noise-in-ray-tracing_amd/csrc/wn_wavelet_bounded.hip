// wn_wavelet_bounded.hip -- the curl noise of 3-D wavelet noise potentials with solid boundaries, on point lists and under
// particle advection (include/wnoise_bounded.h).
//
// The velocity is wn::eval3d_curl_bounded_exact / multiband_curl_bounded_exact (wn_eval.hpp), stated once for these kernels
// and for the host's wnhost_eval3d_curl_bounded; a particle's trace through a launch and the chain of launches are
// wn_advect.hpp's (wn::advect_trace, wn::advect_chain).
//
//   curl3d_bounded_points_kernel<PADDED, MB>          one point per lane in a grid-stride loop, records {vx, vy, vz}.
//   curl3d_bounded_advect_kernel<PADDED, MB, METHOD>  one particle per lane in a grid-stride loop; position, stage point and
//                                                     RK4's running sum in registers.
//
// The obstacle list travels by value in the launch arguments (wn_obstacles.hpp; 16 x 32 bytes): it is the same for every lane, so the
// obstacle loop reads it with scalar loads and branches on the kind as a wave.  A lane that is far from every obstacle
// runs the unbounded evaluator and nothing else; a near lane then walks its 27 taps a second time for the three potential
// values (the rows are in cache, the bits are those of one pass), so the far path keeps the unbounded kernel's live set;
// an inside lane evaluates nothing.  No LDS, no private segment.
//
// A launch integrates at most wn_advect_launch_steps() steps, the cap wn_wavelet_advect.hip measured; a longer trace is a
// chain of launches on the stream.
#include "wn_obstacles.hpp"

#include <algorithm>
#include <cmath>

namespace {

using wn::CurlEval;
using wn::Obstacles;
using wn::obstacle_args;

constexpr size_t kBoundedBlockCap = 256u * 8u; // of the curl point kernel's: the lanes hold 27 row loads each

struct BoundedPointsArgs {
    CurlEval e;
    Obstacles o;
    const float *pts; // xyz interleaved
    float *out;       // {vx, vy, vz} per point
    size_t count;
};

struct BoundedAdvectArgs {
    CurlEval e;
    Obstacles o;
    wn::AdvectTrace<float, 3> t; // xyz interleaved
};

template <bool PADDED, bool MB>
__device__ __forceinline__ void bounded_velocity_at(const CurlEval &e, const Obstacles &o, const float q[3], float v[3])
{
    if (MB) wn::multiband_curl_bounded_exact<PADDED>(e, o.list, o.nobs, q, v);
    else wn::eval3d_curl_bounded_exact<PADDED>(e.coef, e.n, e.nmask, e.off, o.list, o.nobs, q, v);
}

template <bool PADDED, bool MB>
__global__ __launch_bounds__(256) void curl3d_bounded_points_kernel(const BoundedPointsArgs a)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.count; i += (size_t)gridDim.x * blockDim.x) {
        const float p[3] = {a.pts[3 * i], a.pts[3 * i + 1], a.pts[3 * i + 2]};
        float v[3];
        bounded_velocity_at<PADDED, MB>(a.e, a.o, p, v);
        a.out[3 * i] = v[0];
        a.out[3 * i + 1] = v[1];
        a.out[3 * i + 2] = v[2];
    }
}

template <bool PADDED, bool MB, int METHOD>
__global__ __launch_bounds__(256) void curl3d_bounded_advect_kernel(const BoundedAdvectArgs a)
{
    const auto velocity = [&](const float q[3], float v[3]) { bounded_velocity_at<PADDED, MB>(a.e, a.o, q, v); };
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.t.count; i += (size_t)gridDim.x * blockDim.x) {
        float p[3] = {a.t.in[3 * i], a.t.in[3 * i + 1], a.t.in[3 * i + 2]};
        wn::advect_trace<METHOD>(a.t, p, 3 * i, velocity, [&](float *dst) {
            dst[0] = p[0];
            dst[1] = p[1];
            dst[2] = p[2];
        });
    }
}

int launch_bounded_points(const wn_tile *tile, const CurlEval &e, const Obstacles &o, const float *xyz_dev, size_t n,
                          float *out3_dev, hipStream_t stream)
{
    if (!xyz_dev || !out3_dev) return wn::fail(WN_ERR_INVALID, "points/out pointer is NULL");
    const BoundedPointsArgs a{e, o, xyz_dev, out3_dev, n};
    const dim3 grid(wn::stride_blocks(n, kBoundedBlockCap)), block(256);
    wn::with_curl_form(tile, e, [&](auto padded, auto mb) {
        hipLaunchKernelGGL((curl3d_bounded_points_kernel<decltype(padded)::value, decltype(mb)::value>), grid, block, 0, stream,
                           a);
    });
    WN_LAUNCH_CHECK("curl3d_bounded_points_kernel");
    return WN_OK;
}

// The entry points after their tile, offset, band and obstacle checks: the checks of `adv` and of the three buffers, then
// the chain of launches, each of at most wn_advect_launch_steps() steps.
int bounded_advect_points(const wn_tile *tile, const CurlEval &e, const Obstacles &o, const float *in_dev, size_t n,
                          const wn_advect *adv, float *out_dev, float *traj_dev, hipStream_t stream)
{
    int rc = wn::check_advect(adv);
    if (rc || n == 0) return rc;
    rc = wn::check_advect_buffers<float, 3>(in_dev, out_dev, traj_dev, n, adv->traj_every, "xyz_in_dev", "xyz_out_dev");
    if (rc) return rc;
    const dim3 grid(wn::stride_blocks(n, kBoundedBlockCap)), block(256);
    const auto launch_one = [&](const wn::AdvectTrace<float, 3> &t) -> int {
        const BoundedAdvectArgs a{e, o, t};
        wn::with_curl_form(tile, e, [&](auto padded, auto mb) {
            wn::with_advect_method(adv->method, [&](auto method) {
                constexpr bool kPadded = decltype(padded)::value, kMb = decltype(mb)::value;
                hipLaunchKernelGGL((curl3d_bounded_advect_kernel<kPadded, kMb, decltype(method)::value>), grid, block, 0, stream,
                                   a);
            });
        });
        WN_LAUNCH_CHECK("curl3d_bounded_advect_kernel");
        return WN_OK;
    };
    return wn::advect_chain(wn::advect_trace_fill<float, 3>(*adv, n), in_dev, out_dev, traj_dev, adv->steps,
                            wn_advect_launch_steps(), launch_one);
}

} // namespace

using namespace wn;

extern "C" {

int wn_eval3d_curl_bounded_points(const wn_tile *tile, const float *xyz_dev, size_t n, const int32_t *offsets9_host,
                                  const wn_obstacle *obstacles_host, int nobs, float *out3_dev, void *stream)
{
    WN_ENTRY();
    CurlEval e;
    Obstacles o;
    int rc = curl_eval_args(tile, offsets9_host, "wn_eval3d_curl_bounded_points", &e);
    if (rc) return rc;
    rc = obstacle_args(obstacles_host, nobs, "wn_eval3d_curl_bounded_points", &o);
    if (rc || n == 0) return rc;
    return launch_bounded_points(tile, e, o, xyz_dev, n, out3_dev, as_stream(stream));
}

int wn_multiband3d_curl_bounded_points(const wn_tile *tile, const float *xyz_dev, size_t n, const int32_t *offsets9_host,
                                       float s, int first_band, int nbands, const float *w_host, float var_per_band,
                                       const wn_obstacle *obstacles_host, int nobs, float *out3_dev, void *stream)
{
    WN_ENTRY();
    CurlEval e;
    Obstacles o;
    int rc = curl_eval_args(tile, offsets9_host, "wn_multiband3d_curl_bounded_points", &e);
    if (rc) return rc;
    rc = multiband_bands(s, first_band, nbands, w_host, var_per_band, &e);
    if (rc) return rc;
    rc = obstacle_args(obstacles_host, nobs, "wn_multiband3d_curl_bounded_points", &o);
    if (rc || n == 0) return rc;
    e.mb = 1;
    return launch_bounded_points(tile, e, o, xyz_dev, n, out3_dev, as_stream(stream));
}

int wn_eval3d_curl_bounded_advect_points(const wn_tile *tile, const float *xyz_in_dev, size_t n, const int32_t *offsets9_host,
                                         const wn_obstacle *obstacles_host, int nobs, const wn_advect *a, float *xyz_out_dev,
                                         float *traj_dev, void *stream)
{
    WN_ENTRY();
    CurlEval e;
    Obstacles o;
    int rc = curl_eval_args(tile, offsets9_host, "wn_eval3d_curl_bounded_advect_points", &e);
    if (rc) return rc;
    rc = obstacle_args(obstacles_host, nobs, "wn_eval3d_curl_bounded_advect_points", &o);
    if (rc) return rc;
    return bounded_advect_points(tile, e, o, xyz_in_dev, n, a, xyz_out_dev, traj_dev, as_stream(stream));
}

int wn_multiband3d_curl_bounded_advect_points(const wn_tile *tile, const float *xyz_in_dev, size_t n,
                                              const int32_t *offsets9_host, float s, int first_band, int nbands,
                                              const float *w_host, float var_per_band, const wn_obstacle *obstacles_host,
                                              int nobs, const wn_advect *a, float *xyz_out_dev, float *traj_dev, void *stream)
{
    WN_ENTRY();
    CurlEval e;
    Obstacles o;
    int rc = curl_eval_args(tile, offsets9_host, "wn_multiband3d_curl_bounded_advect_points", &e);
    if (rc) return rc;
    rc = multiband_bands(s, first_band, nbands, w_host, var_per_band, &e);
    if (rc) return rc;
    rc = obstacle_args(obstacles_host, nobs, "wn_multiband3d_curl_bounded_advect_points", &o);
    if (rc) return rc;
    e.mb = 1;
    return bounded_advect_points(tile, e, o, xyz_in_dev, n, a, xyz_out_dev, traj_dev, as_stream(stream));
}

} // extern "C"
