// wn_wavelet_bounded2d.hip -- curl noise on a 2-D tile with solid boundaries and a background stream, on point lists, dense
// lattices and under particle advection (include/wnoise_bounded2d.h).
//
// The velocity is wn::obstacle_ramp<2> followed by wn::multiband2d_curl_bounded_at (wn_eval.hpp), stated once for these
// kernels and for the host's wnhost_multiband2d_curl_bounded; a particle's trace through a launch and the chain of launches
// are wn_advect.hpp's (wn::advect_trace, wn::advect_chain).  The kernels mirror wn_wavelet_curl2d.hip's:
//
//   curl2d_bounded_grid_kernel<LDS>            one sample per lane, the lattice walk of curl2d_grid_kernel; two planes.
//   curl2d_bounded_points_kernel<LDS>          one point per lane, grid-stride; records {vx, vy}.
//   curl2d_bounded_advect_kernel<METHOD, LDS>  one particle per lane, grid-stride; position, stage point and RK4's running
//                                              sum in registers.  No private segment.
//
// The obstacle list travels by value in the launch arguments (16 x 32 bytes): it is the same for every lane, so the obstacle
// loop reads it with scalar loads and branches on the kind as a wave.  The ramp is computed before the band loop, and only
// `where`, A and G stay live across it.  Near an obstacle, and wherever a background stream is present, the velocity needs
// the stream function's value beside its two derivatives: one walk over the nine taps of every band yields all three
// (wn::multiband2d_footprint_exact<GRAD = true>), and its derivative channels have the bits of the curl-only walk.  So one
// wave-uniform decision picks the walk for the whole wave -- any lane near, or a stream present: value and derivatives;
// otherwise the curl-only walk of the unbounded kernels -- and no wave walks its taps twice.  A lane inside a solid evaluates
// nothing and stores zeros; it still takes part in staging and in the barrier.  nobs == 0 without a stream is routed to the
// unbounded entry points of wn_wavelet_curl2d.hip.
//
// The LDS and gather forms, the two list-length thresholds and the fit threshold are wn_wavelet_curl2d.hip's (the constants
// below repeat its values), and so is the launch cap: wn_advect2d_launch_steps().  The workgroup shape is this file's own,
// see kWorkgroupsPerCu; profiles/bounded2d_timing.py builds the alternative with the WN_BOUNDED2D_* macros below (the product
// defines none of them) and profiles/bounded2d_kernels.txt records the measurements.
#include "wn_internal.hpp"
#include "wn_tile2d_lds.hpp"
#include "wnoise_bounded2d.h"

#include <algorithm>
#include <cmath>

namespace {

using wn::GridArgs;

static_assert(sizeof(wn_obstacle2d) == 32 && WN_MAX_OBSTACLES == wn::kMaxObstacles, "include/wnoise_bounded2d.h");

#ifndef WN_BOUNDED2D_WORKGROUP
#define WN_BOUNDED2D_WORKGROUP 1024
#endif
#ifndef WN_BOUNDED2D_WORKGROUPS_PER_CU
#define WN_BOUNDED2D_WORKGROUPS_PER_CU 2
#endif
#ifndef WN_BOUNDED2D_POINTS_LDS_MIN_POINTS
#define WN_BOUNDED2D_POINTS_LDS_MIN_POINTS 1024
#endif
#ifndef WN_BOUNDED2D_ADVECT_LDS_MIN_POINTS
#define WN_BOUNDED2D_ADVECT_LDS_MIN_POINTS 1
#endif

constexpr int kWorkgroup = WN_BOUNDED2D_WORKGROUP; // lanes per workgroup, every kernel and both forms
// Workgroups that share a CU.  Two of 1024 lanes leave 64 VGPRs a lane, the shape of the unbounded kernels; every kernel of
// this file fits it without a private segment (tests/test_bounded2d_register_budget.py).  One workgroup per CU (128 VGPRs) is
// the alternative that profiles/bounded2d_timing.py measures.
constexpr int kWorkgroupsPerCu = WN_BOUNDED2D_WORKGROUPS_PER_CU;
constexpr int kWavesPerSimd = kWorkgroupsPerCu * kWorkgroup / 256; // what the launch bounds declare
constexpr size_t kLdsTileMaxBytes = 80 * 1024; // a padded tile up to this size is staged (142^2), whatever kWorkgroupsPerCu
constexpr size_t kLdsNoOptIn = 64 * 1024;      // dynamic LDS beyond this needs wn::ensure_dynamic_lds
// Lists from these lengths on stage the tile; shorter ones gather from global memory: the crossovers of wn_wavelet_curl2d.hip.
constexpr size_t kPointsLdsMinPoints = WN_BOUNDED2D_POINTS_LDS_MIN_POINTS;
constexpr size_t kAdvectLdsMinPoints = WN_BOUNDED2D_ADVECT_LDS_MIN_POINTS;
static_assert(kWorkgroup % 256 == 0 && kWorkgroup <= 1024, "whole waves on every SIMD");
static_assert(kWorkgroupsPerCu * kLdsTileMaxBytes <= 160 * 1024, "a staged tile per workgroup on the CU");
static_assert(kWavesPerSimd >= 1 && kWavesPerSimd <= 8, "waves a SIMD holds");

struct Bounds2d { // the obstacles and the stream, the same for every lane
    wn_obstacle2d list[WN_MAX_OBSTACLES];
    int nobs;
    int has_flow;
    float flow[2]; // {ux, uy}; read when has_flow
};

struct Bounded2dArgs : wn::FootprintBands { // Curl2dArgs of wn_wavelet_curl2d.hip, and the bounds
    const float *coef; // the tile in global memory, linear layout (n^2, x fastest); an empty tile: never read
    int n, nmask;
    float s;
    const float *pts; // point lists: xy interleaved
    float *out;
    size_t count; // points, or samples per plane (nx * ny)
    GridArgs g;   // grids
    Bounds2d b;
};

struct BoundedAdvect2dArgs : wn::FootprintBands {
    const float *coef;
    int n, nmask;
    float s;
    size_t count;                // of t: what launch() sizes the grid by
    wn::AdvectTrace<float, 2> t; // xy interleaved
    Bounds2d b;
};

// The velocity at q for the active lanes of the wave; every lane of a converged wave calls it together.
template <bool LDS, typename Args>
__device__ __forceinline__ void bounded_velocity_at(const Args &a, const float *coef, const float q[2], float v[2])
{
    float ramp, G[2];
    const int where = wn::obstacle_ramp<2>(a.b.list, a.b.nobs, q, ramp, G);
    const bool wide = a.b.has_flow || __any(where == wn::kBoundNear); // wave-uniform: one walk per wave
    wn::multiband2d_curl_bounded_at<LDS>(a, coef, where, ramp, G, a.b.has_flow ? a.b.flow : nullptr, wide, q, a.s, v);
}

template <bool LDS>
__global__ __launch_bounds__(kWorkgroup, kWavesPerSimd) void curl2d_bounded_grid_kernel(const Bounded2dArgs a)
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
            bounded_velocity_at<LDS>(a, coef, p, v);
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
__global__ __launch_bounds__(kWorkgroup, kWavesPerSimd) void curl2d_bounded_points_kernel(const Bounded2dArgs a)
{
    extern __shared__ float tile_lds[];
    if constexpr (LDS) wn::stage_tile<kWorkgroup>(tile_lds, a.coef, a.n);
    const float *coef = LDS ? tile_lds : a.coef;
    for (size_t i = (size_t)blockIdx.x * kWorkgroup + threadIdx.x; i < a.count; i += (size_t)gridDim.x * kWorkgroup) {
        const float p[2] = {a.pts[2 * i], a.pts[2 * i + 1]};
        float v[2];
        bounded_velocity_at<LDS>(a, coef, p, v);
        a.out[2 * i] = v[0];
        a.out[2 * i + 1] = v[1];
    }
}

template <int METHOD, bool LDS>
__global__ __launch_bounds__(kWorkgroup, kWavesPerSimd) void curl2d_bounded_advect_kernel(const BoundedAdvect2dArgs a)
{
    extern __shared__ float tile_lds[];
    if constexpr (LDS) wn::stage_tile<kWorkgroup>(tile_lds, a.coef, a.n);
    const float *coef = LDS ? tile_lds : a.coef;
    const auto velocity = [&](const float q[2], float v[2]) { bounded_velocity_at<LDS>(a, coef, q, v); };
    // The span's base and the snapshot's plane are the same for every lane (scalar registers); a lane keeps its position
    // alone across the steps and forms its addresses where it stores.
    for (size_t base = (size_t)blockIdx.x * kWorkgroup; base < a.t.count; base += (size_t)gridDim.x * kWorkgroup) {
        if (base + threadIdx.x >= a.t.count) continue;
        float p[2] = {a.t.in[2 * (base + threadIdx.x)], a.t.in[2 * (base + threadIdx.x) + 1]};
        wn::advect_trace<METHOD>(a.t, p, 2 * base, velocity, [&](float *dst) {
            unsigned lane = threadIdx.x;
            asm volatile("" : "+v"(lane)); // the lane's address is formed here, not kept in registers across the steps
            dst[2 * lane] = p[0];
            dst[2 * lane + 1] = p[1];
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

// The checks that follow those of the unbounded entry point: the obstacle list, then the stream.
int bounds_args(const char *entry, const wn_obstacle2d *obstacles_host, int nobs, const float *flow2_host, Bounds2d *b)
{
    if (const char *why = wn::obstacle_fault<2>(obstacles_host, nobs)) return wn::fail(WN_ERR_INVALID, "%s: %s", entry, why);
    if (flow2_host && !(std::isfinite(flow2_host[0]) && std::isfinite(flow2_host[1])))
        return wn::fail(WN_ERR_INVALID, "%s: flow2_host must be finite", entry);
    *b = Bounds2d{};
    std::copy(obstacles_host, obstacles_host + nobs, b->list);
    b->nobs = nobs;
    b->has_flow = flow2_host != nullptr;
    if (flow2_host) std::copy(flow2_host, flow2_host + 2, b->flow);
    return WN_OK;
}

bool unbounded(const Bounds2d &b) { return b.nobs == 0 && !b.has_flow; }

} // namespace

extern "C" {

int wn_multiband2d_curl_bounded_points(const wn_tile *tile, const float *xy_dev, size_t n, float s, int first_band, int nbands,
                                       const float *w_host, float var_per_band, const wn_obstacle2d *obstacles_host, int nobs,
                                       const float *flow2_host, float *out2_dev, void *stream)
{
    WN_ENTRY();
    static const char *const entry = "wn_multiband2d_curl_bounded_points";
    Bounded2dArgs a{};
    int rc = common_args(entry, tile, first_band, nbands, w_host, var_per_band, s, &a);
    if (rc) return rc;
    if (n && (!xy_dev || !out2_dev)) return wn::fail(WN_ERR_INVALID, "points/out pointer is NULL");
    rc = bounds_args(entry, obstacles_host, nobs, flow2_host, &a.b);
    if (rc || n == 0) return rc;
    if (unbounded(a.b))
        return wn_multiband2d_curl_points(tile, xy_dev, n, s, first_band, nbands, w_host, var_per_band, out2_dev, stream);
    a.pts = xy_dev;
    a.out = out2_dev;
    a.count = n;
    return launch(curl2d_bounded_points_kernel<true>, curl2d_bounded_points_kernel<false>,
                  n >= kPointsLdsMinPoints ? lds_tile_bytes(a.n) : 0, a, "curl2d_bounded_points_kernel", wn::as_stream(stream));
}

int wn_multiband2d_curl_bounded_grid(const wn_tile *tile, const wn_grid *g, float s, int first_band, int nbands,
                                     const float *w_host, float var_per_band, const wn_obstacle2d *obstacles_host, int nobs,
                                     const float *flow2_host, float *out_dev, void *stream)
{
    WN_ENTRY();
    static const char *const entry = "wn_multiband2d_curl_bounded_grid";
    Bounded2dArgs a{};
    int rc = common_args(entry, tile, first_band, nbands, w_host, var_per_band, s, &a);
    if (rc) return rc;
    rc = wn::check_grid(g, false, &a.g); // flags: one tier, ignored
    if (rc) return rc;
    a.count = (size_t)a.g.nx * a.g.ny;
    if (a.count && !out_dev) return wn::fail(WN_ERR_INVALID, "out_dev is NULL");
    rc = bounds_args(entry, obstacles_host, nobs, flow2_host, &a.b);
    if (rc || a.count == 0) return rc;
    if (unbounded(a.b)) return wn_multiband2d_curl_grid(tile, g, s, first_band, nbands, w_host, var_per_band, out_dev, stream);
    a.out = out_dev;
    return launch(curl2d_bounded_grid_kernel<true>, curl2d_bounded_grid_kernel<false>, lds_tile_bytes(a.n), a,
                  "curl2d_bounded_grid_kernel", wn::as_stream(stream));
}

int wn_multiband2d_curl_bounded_advect_points(const wn_tile *tile, const float *xy_in_dev, size_t n, float s, int first_band,
                                              int nbands, const float *w_host, float var_per_band,
                                              const wn_obstacle2d *obstacles_host, int nobs, const float *flow2_host,
                                              const wn_advect2d *adv, float *xy_out_dev, float *traj_dev, void *stream)
{
    WN_ENTRY();
    static const char *const entry = "wn_multiband2d_curl_bounded_advect_points";
    BoundedAdvect2dArgs a{};
    int rc = common_args(entry, tile, first_band, nbands, w_host, var_per_band, s, &a);
    if (rc) return rc;
    rc = wn::check_advect(adv);
    if (rc) return rc;
    if (n) rc = wn::check_advect_buffers<float, 2>(xy_in_dev, xy_out_dev, traj_dev, n, adv->traj_every, "xy_in_dev", "xy_out_dev");
    if (rc) return rc;
    rc = bounds_args(entry, obstacles_host, nobs, flow2_host, &a.b);
    if (rc || n == 0) return rc;
    if (unbounded(a.b))
        return wn_multiband2d_curl_advect_points(tile, xy_in_dev, n, s, first_band, nbands, w_host, var_per_band, adv,
                                                 xy_out_dev, traj_dev, stream);

    a.count = n;
    const size_t lds = n >= kAdvectLdsMinPoints ? lds_tile_bytes(a.n) : 0;
    const auto launch_one = [&](const wn::AdvectTrace<float, 2> &t) {
        a.t = t;
        return wn::with_advect_method(adv->method, [&](auto method) {
            constexpr int kMethod = decltype(method)::value;
            return launch(curl2d_bounded_advect_kernel<kMethod, true>, curl2d_bounded_advect_kernel<kMethod, false>, lds, a,
                          "curl2d_bounded_advect_kernel", wn::as_stream(stream));
        });
    };
    return wn::advect_chain(wn::advect_trace_fill<float, 2>(*adv, n), xy_in_dev, xy_out_dev, traj_dev, adv->steps,
                            wn_advect2d_launch_steps(adv->method, nbands), launch_one);
}

} // extern "C"
