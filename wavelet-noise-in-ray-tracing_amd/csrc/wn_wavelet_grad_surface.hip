// wn_wavelet_grad_surface.hip -- analytic gradients of the surface-facing wavelet evaluators: evaluate2D (the texture's
// use_3d == false branch), evaluate3DProjected (Cook & DeRose 3.7, WProjectedNoise) and its WMultibandNoise composition
// (normal != NULL), on point lists and dense grids.
//
// evaluate2D (WaveletNoise.cpp:111-140) is a 3 x 3 quadratic B-spline sum: d/dx reads its 9 coefficients with tap weights
// d_x*w_y, d/dy with w_x*d_y (d = -t, 2t - 1, 1 - t per axis).  evaluate3DProjected (:218-265) sums the cells of a support
// box with weight prod_i B(t_i), t_i = (c_i + n_i*dot/2) - (p_i - 1.5); its gradient with respect to p (the normal held
// fixed) is sum_cells ((n_j/2) S - G_j) c, G_i = B'(t_i) prod_{k!=i} B(t_k), S = sum_i n_i G_i, over EVERY cell with
// 0 < t < 3 on all three axes -- the value's 1e-6 weight cut is not applied to the gradient (wn::projected_grad_exact).
//
//   grad2d_points_kernel                  one point per lane, wn::eval2d_exact<true> (the value has the bits of
//                                         wn_eval2d_points), one {value, d/dx, d/dy} record of 3 floats per point.
//   grad2d_grid_kernel                    one sample per lane at lattice_coord's coordinates; three planes.
//   grad_projected_points_kernel          one point and its normal per lane, wn::projected_grad_exact (the value has the
//                                         bits of wn_eval3d_projected_points), one 16-byte {value, d/dx, d/dy, d/dz} store.
//   grad_projected_grid_kernel            one sample per lane, one normal for the lattice; four volumes.
//   grad_multiband_projected_points_kernel  wn::multiband_exact, one normal for all points or one each.
//
// The projected loop is bound by VALU work (about 40 operations per cell, 175-343 cells per sample), not by its gathers:
// the value and the gradient come from one pass, and the box, p - 1.5 and n/2 are formed once per sample.  Grids write
// consecutive planes / volumes in the layout of the matching value grid (wn_eval2d_grid, wn_eval3d_projected_grid); the
// gradient is taken with respect to the coordinate the sample passes to the evaluator, and out_scale multiplies every
// channel last.  There is one tier: every sample has the bits of the point kernel at the lattice's float coordinates.
#include "wn_internal.hpp"

#include <cmath>

namespace {

using wn::GridArgs;

// ---- point lists -----------------------------------------------------------------------------------------------------
struct SurfPointsArgs : wn::Bands {
    const float *coef; // linear layout (n^2 or n^3, x fastest)
    int n, nmask;
    const float *pts;     // xy or xyz interleaved
    const float *normals; // projected: xyz per point, or one for all (one_normal)
    float *out;           // 2-D: 3 floats per point; projected: 4 (16-byte aligned)
    size_t count;
    int one_normal;
};

__global__ __launch_bounds__(256) void grad2d_points_kernel(const SurfPointsArgs a)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.count; i += (size_t)gridDim.x * blockDim.x) {
        float g[2];
        const float v = wn::eval2d_exact<true>(a.coef, a.n, a.nmask, a.pts[2 * i], a.pts[2 * i + 1], g);
        float *o = a.out + 3 * i;
        o[0] = v;
        o[1] = g[0];
        o[2] = g[1];
    }
}

__global__ __launch_bounds__(256) void grad_projected_points_kernel(const SurfPointsArgs a)
{
    v4f *out = reinterpret_cast<v4f *>(a.out);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.count; i += (size_t)gridDim.x * blockDim.x) {
        const float p[3] = {a.pts[3 * i], a.pts[3 * i + 1], a.pts[3 * i + 2]};
        const float nr[3] = {a.normals[3 * i], a.normals[3 * i + 1], a.normals[3 * i + 2]};
        float g[3];
        const float v = wn::projected_grad_exact(a.coef, a.n, a.nmask, p, nr, g);
        out[i] = v4f{v, g[0], g[1], g[2]};
    }
}

__global__ __launch_bounds__(256) void grad_multiband_projected_points_kernel(const SurfPointsArgs a)
{
    v4f *out = reinterpret_cast<v4f *>(a.out);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.count; i += (size_t)gridDim.x * blockDim.x) {
        const float p[3] = {a.pts[3 * i], a.pts[3 * i + 1], a.pts[3 * i + 2]};
        const float *nrp = a.normals + (a.one_normal ? 0 : 3 * i);
        const float nr[3] = {nrp[0], nrp[1], nrp[2]};
        float g[3];
        const float v = wn::multiband_exact<false, true, true>(a, p, nr, g);
        out[i] = v4f{v, g[0], g[1], g[2]};
    }
}

// ---- dense grids ---------------------------------------------------------------------------------------------------------
struct SurfGridArgs {
    const float *coef;
    float *out;
    size_t vol; // samples per channel plane / volume
    int n, nmask;
    GridArgs g;
    float normal[3]; // projected
};

__global__ __launch_bounds__(256) void grad2d_grid_kernel(const SurfGridArgs a)
{
    const GridArgs &g = a.g;
    const float den = (float)g.den;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < a.vol; e += (size_t)gridDim.x * blockDim.x) {
        float px, py, gr[2];
        wn::lattice_point2d(g, den, e, px, py);
        const float v = wn::eval2d_exact<true>(a.coef, a.n, a.nmask, px, py, gr);
        a.out[e] = v * g.out_scale;
        a.out[e + a.vol] = gr[0] * g.out_scale;
        a.out[e + 2 * a.vol] = gr[1] * g.out_scale;
    }
}

__global__ __launch_bounds__(256) void grad_projected_grid_kernel(const SurfGridArgs a)
{
    const GridArgs &g = a.g;
    const float den = (float)g.den;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < a.vol; e += (size_t)gridDim.x * blockDim.x) {
        float p[3], gr[3];
        wn::lattice_point(g, den, e, p);
        const float v = wn::projected_grad_exact(a.coef, a.n, a.nmask, p, a.normal, gr);
        a.out[e] = v * g.out_scale;
        a.out[e + a.vol] = gr[0] * g.out_scale;
        a.out[e + 2 * a.vol] = gr[1] * g.out_scale;
        a.out[e + 3 * a.vol] = gr[2] * g.out_scale;
    }
}

// The arguments every point entry point checks, in wn_eval3d_grad_points's order: the tile (wn::check_tile), then -- for
// a list that is not empty -- the pointers and, for float4 records, out's 16-byte alignment.
SurfPointsArgs surf_points_args(const wn_tile *tile, const float *pts, const float *normals, size_t n, float *out)
{
    SurfPointsArgs a{};
    a.coef = tile->dev; // the 2-D and the projected evaluators index the linear layout
    a.n = tile->n;
    a.nmask = wn::pow2_mask(tile->n);
    a.pts = pts;
    a.normals = normals;
    a.out = out;
    a.count = n;
    return a;
}

int check_points(const SurfPointsArgs &a, bool projected)
{
    if (!a.pts || !a.out) return wn::fail(WN_ERR_INVALID, "points/out pointer is NULL");
    if (projected && !a.normals) return wn::fail(WN_ERR_INVALID, "normals_dev is NULL");
    if (projected && (reinterpret_cast<uintptr_t>(a.out) & 15)) return wn::fail(WN_ERR_INVALID, "out4_dev must be 16-byte aligned");
    return WN_OK;
}

} // namespace

using namespace wn;

extern "C" {

int wn_eval2d_grad_points(const wn_tile *tile, const float *xy_dev, size_t n, float *out3_dev, void *stream)
{
    WN_ENTRY();
    int rc = check_tile(tile, 2, "wn_eval2d_grad_points");
    if (rc || n == 0) return rc;
    const SurfPointsArgs a = surf_points_args(tile, xy_dev, nullptr, n, out3_dev);
    if ((rc = check_points(a, false)) != WN_OK) return rc;
    hipLaunchKernelGGL(grad2d_points_kernel, dim3(wn::stride_blocks(n)), dim3(256), 0, as_stream(stream), a);
    WN_LAUNCH_CHECK("grad2d_points_kernel");
    return WN_OK;
}

int wn_eval3d_projected_grad_points(const wn_tile *tile, const float *xyz_dev, const float *normals_dev, size_t n,
                                    float *out4_dev, void *stream)
{
    WN_ENTRY();
    int rc = check_tile(tile, 3, "wn_eval3d_projected_grad_points");
    if (rc || n == 0) return rc;
    const SurfPointsArgs a = surf_points_args(tile, xyz_dev, normals_dev, n, out4_dev);
    if ((rc = check_points(a, true)) != WN_OK) return rc;
    hipLaunchKernelGGL(grad_projected_points_kernel, dim3(wn::stride_blocks(n)), dim3(256), 0, as_stream(stream), a);
    WN_LAUNCH_CHECK("grad_projected_points_kernel");
    return WN_OK;
}

int wn_multiband3d_projected_grad_points(const wn_tile *tile, const float *xyz_dev, const float *normals_dev,
                                         int one_normal, size_t n, float s, int first_band, int nbands,
                                         const float *w_host, float var_per_band, float *out4_dev, void *stream)
{
    WN_ENTRY();
    int rc = check_tile(tile, 3, "wn_multiband3d_projected_grad_points");
    if (rc) return rc;
    SurfPointsArgs a = surf_points_args(tile, xyz_dev, normals_dev, n, out4_dev);
    rc = multiband_bands(s, first_band, nbands, w_host, var_per_band, &a);
    if (rc || n == 0) return rc;
    if ((rc = check_points(a, true)) != WN_OK) return rc;
    a.one_normal = one_normal ? 1 : 0;
    hipLaunchKernelGGL(grad_multiband_projected_points_kernel, dim3(wn::stride_blocks(n)), dim3(256), 0,
                       as_stream(stream), a);
    WN_LAUNCH_CHECK("grad_multiband_projected_points_kernel");
    return WN_OK;
}

int wn_eval2d_grad_grid(const wn_tile *tile, const wn_grid *grid, float *out_dev, void *stream)
{
    WN_ENTRY();
    int rc = check_tile(tile, 2, "wn_eval2d_grad_grid");
    if (rc) return rc;
    GridArgs g;
    rc = check_grid(grid, false, &g); // flags: one tier, ignored
    if (rc) return rc;
    const size_t total = (size_t)g.nx * g.ny;
    if (total == 0) return WN_OK;
    if (!out_dev) return fail(WN_ERR_INVALID, "out_dev is NULL");
    SurfGridArgs a{};
    a.coef = tile->dev;
    a.out = out_dev;
    a.vol = total;
    a.n = tile->n;
    a.nmask = pow2_mask(tile->n);
    a.g = g;
    hipLaunchKernelGGL(grad2d_grid_kernel, dim3(wn::stride_blocks(total)), dim3(256), 0, as_stream(stream), a);
    WN_LAUNCH_CHECK("grad2d_grid_kernel");
    return WN_OK;
}

int wn_eval3d_projected_grad_grid(const wn_tile *tile, const wn_grid *grid, const float normal[3], float *out_dev,
                                  void *stream)
{
    WN_ENTRY();
    int rc = check_tile(tile, 3, "wn_eval3d_projected_grad_grid");
    if (rc) return rc;
    if (!normal) return fail(WN_ERR_INVALID, "normal is NULL");
    GridArgs g;
    rc = check_grid(grid, true, &g); // flags: one tier, ignored
    if (rc) return rc;
    const size_t total = (size_t)g.nx * g.ny * g.nz;
    if (total == 0) return WN_OK;
    if (!out_dev) return fail(WN_ERR_INVALID, "out_dev is NULL");
    SurfGridArgs a{};
    a.coef = tile->dev;
    a.out = out_dev;
    a.vol = total;
    a.n = tile->n;
    a.nmask = pow2_mask(tile->n);
    a.g = g;
    for (int i = 0; i < 3; ++i) a.normal[i] = normal[i];
    hipLaunchKernelGGL(grad_projected_grid_kernel, dim3(wn::stride_blocks(total)), dim3(256), 0,
                       as_stream(stream), a);
    WN_LAUNCH_CHECK("grad_projected_grid_kernel");
    return WN_OK;
}

} // extern "C"
