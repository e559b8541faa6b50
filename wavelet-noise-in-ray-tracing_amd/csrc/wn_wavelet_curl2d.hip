// wn_wavelet_curl2d.hip -- divergence-free curl noise on a 2-D tile and particles moved through it
// (include/wnoise_curl2d.h).  The velocity at a point is one call of wn::multiband2d_curl_exact (wn_eval.hpp): the gradient
// channels of wn_wavelet_multiband2d.hip's evaluator at the call's footprint, rotated; the trace of a particle through a
// launch and the chain of launches of a call are wn_advect.hpp's (wn::advect_trace, wn::advect_chain), in two dimensions.
// The host's wnhost_multiband2d_curl and wnhost_multiband2d_curl_advect compile both too: the same bits.
//
//   curl2d_grid_kernel<LDS>            one sample per lane; a workgroup walks spans of kWorkgroup samples (the lattice
//                                      walk of multiband2d_grid_kernel); two planes, vx and vy.
//   curl2d_points_kernel<LDS>          one point per lane, grid-stride; records {vx, vy}.
//   curl2d_advect_kernel<METHOD, LDS>  one particle per lane, grid-stride: the position is loaded once, the steps of the
//                                      launch run on registers (position, stage point, RK4's running sum), a trajectory
//                                      snapshot is two float stores to the time-major address, the final position two more.
//                                      No private segment.
//
// LDS: as in wn_wavelet_multiband2d.hip a workgroup copies the WHOLE tile into LDS once, before its loop, in the padded
// layout (wn_tile2d_lds.hpp), and every tap of every band, stage and step is read there: the advection kernel touches
// global memory for the position at the start, the position at the end and the snapshots only, so the order of the
// particles does not matter.  The global form of the same kernels (LDS false) gathers from the linear tile in global
// memory; it serves the tiles whose padded copy exceeds kLdsTileMaxBytes (256^2: 258 KiB) and the empty tile, and the
// point lists shorter than kCurl2dPointsLdsMinPoints / kAdvect2dLdsMinPoints, for which staging the tile costs more than
// it saves.  Both forms call the one evaluator on the same coefficients in the same order: identical bits.
//
// The launch is multiband2d's: min(spans, kWorkgroupsPerCu * CUs) workgroups of kWorkgroup lanes.  The shape, the two
// thresholds and the launch cap were settled with profiles/curl2d_timing.py, which times builds of the alternatives made
// with the WN_CURL2D_* / WN_ADVECT2D_* macros below (the product defines none of them); profiles/curl2d_kernels.txt records
// the measurements.
#include "wn_internal.hpp"
#include "wn_tile2d_lds.hpp"
#include "wnoise_curl2d.h"

#include <algorithm>
#include <cmath>

namespace {

using wn::GridArgs;

#ifndef WN_CURL2D_WORKGROUP
#define WN_CURL2D_WORKGROUP 1024
#endif
#ifndef WN_CURL2D_WORKGROUPS_PER_CU
#define WN_CURL2D_WORKGROUPS_PER_CU 2
#endif
#ifndef WN_CURL2D_POINTS_LDS_MIN_POINTS
#define WN_CURL2D_POINTS_LDS_MIN_POINTS 1024
#endif
#ifndef WN_ADVECT2D_LDS_MIN_POINTS
#define WN_ADVECT2D_LDS_MIN_POINTS 1
#endif
#ifndef WN_ADVECT2D_LAUNCH_EVALS
#define WN_ADVECT2D_LAUNCH_EVALS 768
#endif

constexpr int kWorkgroup = WN_CURL2D_WORKGROUP; // lanes per workgroup, every kernel and both forms
// Workgroups that share a CU: with 1024 lanes, two leave 64 VGPRs a lane (44-56 used) and 80 KiB of LDS each.  Measured on one
// MI355X (profiles/curl2d_kernels.txt): one workgroup of 1024 lanes per CU (128 VGPRs) takes 1.09-1.14 x the time on every
// row, two of 512 lanes 1.11-1.15 x.
constexpr int kWorkgroupsPerCu = WN_CURL2D_WORKGROUPS_PER_CU;
constexpr int kWavesPerSimd = kWorkgroupsPerCu * kWorkgroup / 256; // what the launch bounds declare
// The routing of wn_wavelet_multiband2d.hip: a padded tile of up to 80 KiB (142^2) is staged, whatever kWorkgroupsPerCu.
constexpr size_t kLdsTileMaxBytes = 80 * 1024;
constexpr size_t kLdsNoOptIn = 64 * 1024; // dynamic LDS beyond this needs wn::ensure_dynamic_lds
// Point lists from this length on stage the tile in LDS; shorter ones gather from global memory.  Both are the measured
// crossovers on a 128^2 tile with five bands (the sweep of profiles/curl2d_timing.py over 2^0 .. 2^24 points).  The point
// kernel: 256 points take 5.6 us gathering and 7.0 us staging, 1024 points 15.2 and 9.0 us, 16 M 971 and 239 us.  The
// advection kernel (three RK4 steps): staging wins at every length, 30.1 against 33.5 us for one particle, 50.7 against 156.6 us
// for 1024, 2.69 against 11.6 ms for 16 M -- a lane's gathers wait on one another through every stage of every step, and
// the staging copy is paid once per workgroup and launch.
constexpr size_t kCurl2dPointsLdsMinPoints = WN_CURL2D_POINTS_LDS_MIN_POINTS;
constexpr size_t kAdvect2dLdsMinPoints = WN_ADVECT2D_LDS_MIN_POINTS;
// A launch on a card that others share must end: a launch integrates at most this many band evaluations per particle,
// counted as stages * nbands * steps with nbands the call's band count (the bound on the active bands), and at least one
// step -- the form of wn_perlin_advect.hip's octave budget.  Measured on one MI355X, 16 M particles uniform in a 128-cell
// box, tile 128 (profiles/curl2d_kernels.txt): one band evaluation over the list takes 56.9 us in a one-band launch and
// 45.0 us in a five-band one, whatever the method and the order of the particles.  50 ms, the figure the two other advection
// kernels were sized to, hold 878 of the slowest; 768 = 4 * 192 keeps whole RK4 steps together (192 of one band, 38 of five)
// and its longest launch measured 43.7 ms (192 RK4 steps of one band; five bands: 34.7 ms at most).  A single step of more
// evaluations (RK4 on eight bands: 32) is still one launch.  A launch boundary costs one 16-byte position round trip per
// particle.
constexpr int kAdvect2dLaunchEvals = WN_ADVECT2D_LAUNCH_EVALS;
static_assert(kWorkgroup % 256 == 0 && kWorkgroup <= 1024, "whole waves on every SIMD");
static_assert(kWorkgroupsPerCu * kLdsTileMaxBytes <= 160 * 1024, "a staged tile per workgroup on the CU");
static_assert(kWavesPerSimd >= 1 && kWavesPerSimd <= 8, "waves a SIMD holds");
static_assert(kAdvect2dLaunchEvals >= 1, "a launch integrates something");

struct Curl2dArgs : wn::FootprintBands {
    const float *coef; // the tile in global memory, linear layout (n^2, x fastest); an empty tile: never read
    int n, nmask;
    float s;          // the call's footprint
    const float *pts; // point lists: xy interleaved
    float *out;
    size_t count; // points, or samples per plane (nx * ny)
    GridArgs g;   // grids
};

struct Advect2dArgs : wn::FootprintBands {
    const float *coef;
    int n, nmask;
    float s;
    size_t count;                // of t: what launch() sizes the grid by
    wn::AdvectTrace<float, 2> t; // xy interleaved
};

template <bool LDS>
__global__ __launch_bounds__(kWorkgroup, kWavesPerSimd) void curl2d_grid_kernel(const Curl2dArgs a)
{
    extern __shared__ float tile_lds[];
    if constexpr (LDS) wn::stage_tile<kWorkgroup>(tile_lds, a.coef, a.n);
    const float *coef = LDS ? tile_lds : a.coef;
    const GridArgs &g = a.g;
    const float den = (float)g.den;
    const unsigned nx = (unsigned)g.nx;
    // A span of kWorkgroup consecutive samples starts at (x0, y0); the next span of this workgroup lies `step` samples on.
    const size_t step = (size_t)gridDim.x * kWorkgroup;
    const size_t step_y = step / nx;
    const unsigned step_x = (unsigned)(step - step_y * nx);
    size_t base = (size_t)blockIdx.x * kWorkgroup;
    size_t y0 = base / nx;
    unsigned x0 = (unsigned)(base - y0 * nx);
    for (; base < a.count; base += step) {
        const size_t e = base + threadIdx.x;
        if (e < a.count) {
            unsigned x = x0 + threadIdx.x, dy = 0; // x0 < nx < 2^31: no overflow
            if (nx >= (unsigned)kWorkgroup) {
                if (x >= nx) {
                    x -= nx;
                    dy = 1;
                }
            } else {
                dy = x / nx;
                x -= dy * nx;
            }
            const float p[2] = {wn::grid_coord(g, den, (int)x), wn::grid_coord(g, den, (int)(y0 + dy))};
            float v[2];
            wn::multiband2d_curl_exact<LDS>(a, coef, p, a.s, v);
            a.out[e] = v[0] * g.out_scale;
            a.out[e + a.count] = v[1] * g.out_scale;
        }
        x0 += step_x;
        y0 += step_y;
        if (x0 >= nx) {
            x0 -= nx;
            ++y0;
        }
    }
}

template <bool LDS>
__global__ __launch_bounds__(kWorkgroup, kWavesPerSimd) void curl2d_points_kernel(const Curl2dArgs a)
{
    extern __shared__ float tile_lds[];
    if constexpr (LDS) wn::stage_tile<kWorkgroup>(tile_lds, a.coef, a.n);
    const float *coef = LDS ? tile_lds : a.coef;
    for (size_t i = (size_t)blockIdx.x * kWorkgroup + threadIdx.x; i < a.count; i += (size_t)gridDim.x * kWorkgroup) {
        const float p[2] = {a.pts[2 * i], a.pts[2 * i + 1]};
        float v[2];
        wn::multiband2d_curl_exact<LDS>(a, coef, p, a.s, v);
        a.out[2 * i] = v[0];
        a.out[2 * i + 1] = v[1];
    }
}

template <int METHOD, bool LDS>
__global__ __launch_bounds__(kWorkgroup, kWavesPerSimd) void curl2d_advect_kernel(const Advect2dArgs a)
{
    extern __shared__ float tile_lds[];
    if constexpr (LDS) wn::stage_tile<kWorkgroup>(tile_lds, a.coef, a.n);
    const float *coef = LDS ? tile_lds : a.coef;
    const auto velocity = [&](const float q[2], float v[2]) { wn::multiband2d_curl_exact<LDS>(a, coef, q, a.s, v); };
    for (size_t i = (size_t)blockIdx.x * kWorkgroup + threadIdx.x; i < a.t.count; i += (size_t)gridDim.x * kWorkgroup) {
        float p[2] = {a.t.in[2 * i], a.t.in[2 * i + 1]};
        wn::advect_trace<METHOD>(a.t, p, 2 * i, velocity, [&](float *dst) {
            dst[0] = p[0];
            dst[1] = p[1];
        });
    }
}

// Bytes of the padded tile when the LDS form can serve it, else 0 (the empty tile, or a tile past kLdsTileMaxBytes).
size_t lds_tile_bytes(int n)
{
    const size_t bytes = (size_t)n * (n + 2) * sizeof(float);
    return (n > 0 && bytes <= kLdsTileMaxBytes) ? bytes : 0;
}

// Launch lds_kernel with the tile staged, or gather_kernel when the tile does not fit (lds == 0) or the runtime refuses the
// LDS opt-in: the two have the same bits.
template <typename K, typename Args>
int launch(K lds_kernel, K gather_kernel, size_t lds, const Args &a, const char *name, hipStream_t stream)
{
    const int dev = wn::current_device();
    const size_t spans = (a.count + kWorkgroup - 1) / kWorkgroup, cap = (size_t)kWorkgroupsPerCu * wn::device_compute_units(dev);
    const dim3 grid((unsigned)(spans < cap ? spans : cap));
    if (lds && (lds <= kLdsNoOptIn || wn::ensure_dynamic_lds(reinterpret_cast<const void *>(lds_kernel), dev, lds)))
        hipLaunchKernelGGL(lds_kernel, grid, dim3(kWorkgroup), lds, stream, a);
    else
        hipLaunchKernelGGL(gather_kernel, grid, dim3(kWorkgroup), 0, stream, a);
    WN_LAUNCH_CHECK(name);
    return WN_OK;
}

// The checks of wn_multiband2d_grad_points, in their order: the tile, the bands; then the tile's part of the arguments.
template <typename Args>
int common_args(const char *entry, const wn_tile *tile, int first_band, int nbands, const float *w_host, float var_per_band,
                float s, Args *a)
{
    const int rc = wn::check_tile(tile, 2, entry);
    if (rc) return rc;
    if (nbands < 0 || nbands > wn::kFootprintMaxBands)
        return wn::fail(WN_ERR_INVALID, "nbands must be in 0..%d (got %d)", wn::kFootprintMaxBands, nbands);
    if (nbands && !w_host) return wn::fail(WN_ERR_INVALID, "w_host is NULL");
    wn::footprint_bands_fill(first_band, nbands, w_host, var_per_band, 0, a);
    a->coef = tile->dev;
    a->n = tile->count ? tile->n : 0;
    a->nmask = wn::pow2_mask(a->n);
    a->s = s;
    return WN_OK;
}

int launch_steps(int method, int nbands)
{
    const int bands = std::min(std::max(nbands, 1), wn::kFootprintMaxBands);
    return std::max(1, kAdvect2dLaunchEvals / (wn::advect_stages(method) * bands));
}

} // namespace

extern "C" {

int wn_multiband2d_curl_points(const wn_tile *tile, const float *xy_dev, size_t n, float s, int first_band, int nbands,
                               const float *w_host, float var_per_band, float *out2_dev, void *stream)
{
    WN_ENTRY();
    Curl2dArgs a{};
    const int rc = common_args("wn_multiband2d_curl_points", tile, first_band, nbands, w_host, var_per_band, s, &a);
    if (rc || n == 0) return rc;
    if (!xy_dev || !out2_dev) return wn::fail(WN_ERR_INVALID, "points/out pointer is NULL");
    a.pts = xy_dev;
    a.out = out2_dev;
    a.count = n;
    return launch(curl2d_points_kernel<true>, curl2d_points_kernel<false>,
                  n >= kCurl2dPointsLdsMinPoints ? lds_tile_bytes(a.n) : 0, a, "curl2d_points_kernel", wn::as_stream(stream));
}

int wn_multiband2d_curl_grid(const wn_tile *tile, const wn_grid *g, float s, int first_band, int nbands, const float *w_host,
                             float var_per_band, float *out_dev, void *stream)
{
    WN_ENTRY();
    Curl2dArgs a{};
    int rc = common_args("wn_multiband2d_curl_grid", tile, first_band, nbands, w_host, var_per_band, s, &a);
    if (rc) return rc;
    rc = wn::check_grid(g, false, &a.g); // flags: one tier, ignored
    if (rc) return rc;
    a.count = (size_t)a.g.nx * a.g.ny;
    if (a.count == 0) return WN_OK;
    if (!out_dev) return wn::fail(WN_ERR_INVALID, "out_dev is NULL");
    a.out = out_dev;
    return launch(curl2d_grid_kernel<true>, curl2d_grid_kernel<false>, lds_tile_bytes(a.n), a, "curl2d_grid_kernel",
                  wn::as_stream(stream));
}

int wn_multiband2d_curl_advect_points(const wn_tile *tile, const float *xy_in_dev, size_t n, float s, int first_band,
                                      int nbands, const float *w_host, float var_per_band, const wn_advect2d *adv,
                                      float *xy_out_dev, float *traj_dev, void *stream)
{
    WN_ENTRY();
    Advect2dArgs a{};
    int rc = common_args("wn_multiband2d_curl_advect_points", tile, first_band, nbands, w_host, var_per_band, s, &a);
    if (rc) return rc;
    rc = wn::check_advect(adv);
    if (rc || n == 0) return rc;
    rc = wn::check_advect_buffers<float, 2>(xy_in_dev, xy_out_dev, traj_dev, n, adv->traj_every, "xy_in_dev", "xy_out_dev");
    if (rc) return rc;

    a.count = n;
    const size_t lds = n >= kAdvect2dLdsMinPoints ? lds_tile_bytes(a.n) : 0;
    const auto launch_one = [&](const wn::AdvectTrace<float, 2> &t) {
        a.t = t;
        return wn::with_advect_method(adv->method, [&](auto method) {
            constexpr int kMethod = decltype(method)::value;
            return launch(curl2d_advect_kernel<kMethod, true>, curl2d_advect_kernel<kMethod, false>, lds, a,
                          "curl2d_advect_kernel", wn::as_stream(stream));
        });
    };
    return wn::advect_chain(wn::advect_trace_fill<float, 2>(*adv, n), xy_in_dev, xy_out_dev, traj_dev, adv->steps,
                            launch_steps(adv->method, nbands), launch_one);
}

int wn_advect2d_launch_steps(int method, int nbands) { return launch_steps(method, nbands); }

} // extern "C"
