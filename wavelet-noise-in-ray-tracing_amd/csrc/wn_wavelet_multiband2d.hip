// wn_wavelet_multiband2d.hip -- WMultibandNoise on a 2-D tile (include/wnoise_multiband2d.h): fused band sums on dense
// grids and point lists, their analytic gradients, and the band limit taken from a footprint per point.  Every sample is
// one call of wn::multiband2d_footprint_exact (wn_eval.hpp), which the host's wnhost_multiband2d_footprint compiles too:
// the same bits.  The uniform-s entry points pass the call's s and fade 0.
//
//   multiband2d_grid_kernel<GRAD, LDS>              one sample per lane; a workgroup walks spans of kWorkgroup samples.
//   multiband2d_points_kernel<GRAD, PER_POINT, LDS> one point per lane, grid-stride; each lane loops over its own bands.
//
// LDS: a 2-D tile is small (128^2: 64 KiB) and the CU has 160 KiB of LDS, so a workgroup copies the WHOLE tile into LDS once
// -- row stride n+2 with two wrap-around columns, the layout of wn_tile::dev_padded for 3-D, so the three x taps of a row
// are adjacent -- and every band of every sample reads its 3 x 3 taps there (wn::eval2d_exact<., PADDED>).  The global
// form of the same kernels (LDS false) gathers from the linear tile in global memory; it serves the tiles whose padded
// copy exceeds kLdsTileMaxBytes (256^2: 258 KiB) and the empty tile, and, for point lists, the lists shorter than
// kPointsLdsMinPoints, for which staging the tile costs more than it saves.  Both forms call the one evaluator on the same
// coefficients in the same order: identical bits.
//
// Two workgroups of kWorkgroup lanes share a CU (2 x 66,560 B of LDS for a 128^2 tile; 32 waves with kWorkgroup = 1024),
// which bounds the registers: see the launch bounds.  kWorkgroup and kPointsLdsMinPoints are to be settled by
// profiles/multiband2d_timing.py, which builds the alternatives with the WN_MB2D_* macros below (the product defines none
// of them); profiles/multiband2d_kernels.txt records what has been measured so far.
#include "wn_internal.hpp"
#include "wn_tile2d_lds.hpp"
#include "wnoise_multiband2d.h"

#include <cmath>

namespace {

using wn::GridArgs;

static_assert(wn::kFootprintMaxBands == wn::kMaxBands, "one band limit for the 2-D and the 3-D entry points");

#ifndef WN_MB2D_WORKGROUP
#define WN_MB2D_WORKGROUP 1024
#endif
#ifndef WN_MB2D_LDS_TILE_MAX_BYTES
#define WN_MB2D_LDS_TILE_MAX_BYTES (80 * 1024)
#endif
#ifndef WN_MB2D_POINTS_LDS_MIN_POINTS
#define WN_MB2D_POINTS_LDS_MIN_POINTS (16 * 4096)
#endif

constexpr int kWorkgroup = WN_MB2D_WORKGROUP; // lanes per workgroup, both kernels and both forms
constexpr int kWorkgroupsPerCu = 2;
// The padded tile must leave room for a second workgroup on the CU: half of its 160 KiB.  A tile of up to 142^2 fits.
constexpr size_t kLdsTileMaxBytes = WN_MB2D_LDS_TILE_MAX_BYTES;
// Point lists from this length on stage the tile in LDS; shorter ones gather from global memory (not yet measured: the
// length at which wn_wavelet_points.hip changes to its chunked routes, until the timing script's sweep has run).
constexpr size_t kPointsLdsMinPoints = WN_MB2D_POINTS_LDS_MIN_POINTS;
constexpr size_t kLdsNoOptIn = 64 * 1024; // dynamic LDS beyond this needs wn::ensure_dynamic_lds
static_assert(kWorkgroup % 128 == 0 && kWorkgroup <= 1024, "whole waves on every SIMD");
static_assert(kWorkgroupsPerCu * kLdsTileMaxBytes <= 160 * 1024, "two staged tiles per CU");

struct Mb2dArgs : wn::FootprintBands {
    const float *coef; // the tile in global memory, linear layout (n^2, x fastest); an empty tile: never read
    int n, nmask;
    float s;            // the call's footprint (uniform entry points)
    const float *pts;   // point lists: xy interleaved
    const float *s_pts; // footprint entry points: one s per point
    float *out;
    size_t count; // points, or samples per plane (nx * ny)
    GridArgs g;   // grids
};

template <bool GRAD, bool LDS>
__global__ __launch_bounds__(kWorkgroup, kWorkgroup / 128) void multiband2d_grid_kernel(const Mb2dArgs a)
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
            float gr[2];
            const float v = wn::multiband2d_footprint_exact<GRAD, LDS>(a, coef, p, a.s, gr);
            a.out[e] = v * g.out_scale;
            if constexpr (GRAD) {
                a.out[e + a.count] = gr[0] * g.out_scale;
                a.out[e + 2 * a.count] = gr[1] * g.out_scale;
            }
        }
        x0 += step_x;
        y0 += step_y;
        if (x0 >= nx) {
            x0 -= nx;
            ++y0;
        }
    }
}

template <bool GRAD, bool PER_POINT, bool LDS>
__global__ __launch_bounds__(kWorkgroup, kWorkgroup / 128) void multiband2d_points_kernel(const Mb2dArgs a)
{
    extern __shared__ float tile_lds[];
    if constexpr (LDS) wn::stage_tile<kWorkgroup>(tile_lds, a.coef, a.n);
    const float *coef = LDS ? tile_lds : a.coef;
    for (size_t i = (size_t)blockIdx.x * kWorkgroup + threadIdx.x; i < a.count; i += (size_t)gridDim.x * kWorkgroup) {
        const float p[2] = {a.pts[2 * i], a.pts[2 * i + 1]};
        const float s = PER_POINT ? a.s_pts[i] : a.s;
        float gr[2];
        const float v = wn::multiband2d_footprint_exact<GRAD, LDS>(a, coef, p, s, gr);
        if constexpr (GRAD) {
            float *o = a.out + 3 * i;
            o[0] = v;
            o[1] = gr[0];
            o[2] = gr[1];
        } else {
            a.out[i] = v;
        }
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
template <typename K>
int launch(K lds_kernel, K gather_kernel, size_t lds, const Mb2dArgs &a, const char *name, hipStream_t stream)
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

// The checks of wn_multiband3d_points, in their order: the tile, the bands; then the tile's part of the arguments.
int common_args(const char *entry, const wn_tile *tile, int first_band, int nbands, const float *w_host, float var_per_band,
                int fade, Mb2dArgs *a)
{
    const int rc = wn::check_tile(tile, 2, entry);
    if (rc) return rc;
    if (nbands < 0 || nbands > wn::kFootprintMaxBands)
        return wn::fail(WN_ERR_INVALID, "nbands must be in 0..%d (got %d)", wn::kFootprintMaxBands, nbands);
    if (nbands && !w_host) return wn::fail(WN_ERR_INVALID, "w_host is NULL");
    wn::footprint_bands_fill(first_band, nbands, w_host, var_per_band, fade, a);
    a->coef = tile->dev;
    a->n = tile->count ? tile->n : 0;
    a->nmask = wn::pow2_mask(a->n);
    return WN_OK;
}

template <bool GRAD>
int grid_entry(const char *entry, const wn_tile *tile, const wn_grid *grid, float s, int first_band, int nbands,
               const float *w_host, float var_per_band, float *out, void *stream)
{
    Mb2dArgs a{};
    int rc = common_args(entry, tile, first_band, nbands, w_host, var_per_band, 0, &a);
    if (rc) return rc;
    rc = wn::check_grid(grid, false, &a.g); // flags: one tier, ignored
    if (rc) return rc;
    a.count = (size_t)a.g.nx * a.g.ny;
    if (a.count == 0) return WN_OK;
    if (!out) return wn::fail(WN_ERR_INVALID, "out_dev is NULL");
    a.s = s;
    a.out = out;
    return launch(multiband2d_grid_kernel<GRAD, true>, multiband2d_grid_kernel<GRAD, false>, lds_tile_bytes(a.n), a,
                  "multiband2d_grid_kernel", wn::as_stream(stream));
}

template <bool GRAD, bool PER_POINT>
int points_entry(const char *entry, const wn_tile *tile, const float *xy, const float *s_dev, float s, size_t n,
                 int first_band, int nbands, const float *w_host, float var_per_band, int fade, float *out, void *stream)
{
    Mb2dArgs a{};
    const int rc = common_args(entry, tile, first_band, nbands, w_host, var_per_band, fade, &a);
    if (rc || n == 0) return rc;
    if (!xy || !out) return wn::fail(WN_ERR_INVALID, "points/out pointer is NULL");
    if (PER_POINT && !s_dev) return wn::fail(WN_ERR_INVALID, "s_dev is NULL");
    a.pts = xy;
    a.s_pts = s_dev;
    a.s = s;
    a.out = out;
    a.count = n;
    return launch(multiband2d_points_kernel<GRAD, PER_POINT, true>, multiband2d_points_kernel<GRAD, PER_POINT, false>,
                  n >= kPointsLdsMinPoints ? lds_tile_bytes(a.n) : 0, a, "multiband2d_points_kernel", wn::as_stream(stream));
}

} // namespace

extern "C" {

int wn_multiband2d_grid(const wn_tile *tile, const wn_grid *g, float s, int first_band, int nbands, const float *w_host,
                        float var_per_band, float *out_dev, void *stream)
{
    WN_ENTRY();
    return grid_entry<false>("wn_multiband2d_grid", tile, g, s, first_band, nbands, w_host, var_per_band, out_dev, stream);
}

int wn_multiband2d_grad_grid(const wn_tile *tile, const wn_grid *g, float s, int first_band, int nbands, const float *w_host,
                             float var_per_band, float *out_dev, void *stream)
{
    WN_ENTRY();
    return grid_entry<true>("wn_multiband2d_grad_grid", tile, g, s, first_band, nbands, w_host, var_per_band, out_dev, stream);
}

int wn_multiband2d_points(const wn_tile *tile, const float *xy_dev, size_t n, float s, int first_band, int nbands,
                          const float *w_host, float var_per_band, float *out_dev, void *stream)
{
    WN_ENTRY();
    return points_entry<false, false>("wn_multiband2d_points", tile, xy_dev, nullptr, s, n, first_band, nbands, w_host,
                                      var_per_band, 0, out_dev, stream);
}

int wn_multiband2d_grad_points(const wn_tile *tile, const float *xy_dev, size_t n, float s, int first_band, int nbands,
                               const float *w_host, float var_per_band, float *out3_dev, void *stream)
{
    WN_ENTRY();
    return points_entry<true, false>("wn_multiband2d_grad_points", tile, xy_dev, nullptr, s, n, first_band, nbands, w_host,
                                     var_per_band, 0, out3_dev, stream);
}

int wn_multiband2d_footprint_points(const wn_tile *tile, const float *xy_dev, const float *s_dev, size_t n, int first_band,
                                    int nbands, const float *w_host, float var_per_band, int fade, float *out_dev,
                                    void *stream)
{
    WN_ENTRY();
    return points_entry<false, true>("wn_multiband2d_footprint_points", tile, xy_dev, s_dev, 0.0f, n, first_band, nbands,
                                     w_host, var_per_band, fade, out_dev, stream);
}

int wn_multiband2d_footprint_grad_points(const wn_tile *tile, const float *xy_dev, const float *s_dev, size_t n,
                                         int first_band, int nbands, const float *w_host, float var_per_band, int fade,
                                         float *out3_dev, void *stream)
{
    WN_ENTRY();
    return points_entry<true, true>("wn_multiband2d_footprint_grad_points", tile, xy_dev, s_dev, 0.0f, n, first_band, nbands,
                                    w_host, var_per_band, fade, out3_dev, stream);
}

} // extern "C"
