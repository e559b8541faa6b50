// wn_wavelet_grad.hip -- analytic gradients of 3-D wavelet noise: evaluate3D and WMultibandNoise (normal == NULL) with
// their gradients, on point lists and on dense grids.
//
// evaluate3D (WaveletNoise.cpp:185-215) is a tensor-product quadratic B-spline sum.  Per axis bspline gives mid and
// t = mid - (p - 0.5) and the weights w0 = t^2/2, w2 = (1-t)^2/2, w1 = 1 - w0 - w2; as dt/dp = -1 their derivatives are
// d0 = -t, d1 = 2t - 1, d2 = 1 - t on the same taps.  The spline is C1: the gradient is continuous, also where mid flips.
// Each derivative reads the value's 27 coefficients; only the per-axis weights change.
//
//   grad3d_points_kernel<PADDED, MB>   one point per lane, wn::eval3d_grad_exact / multiband_exact (the value
//                                      channel has the bits of wn_eval3d_points / wn_multiband3d_points), one 16-byte
//                                      {value, d/dx, d/dy, d/dz} store per point.
//   grad3d_grid_direct_kernel<PADDED>  WN_GRID_EXACT and every lattice the brick kernel declines: one sample per lane, the
//                                      point kernel's device function at lattice_coord's coordinates; four volumes.
//   grad3d_grid_sep_kernel<NB>         the default tier: the brick's coefficient box staged in LDS, contracted one axis at
//                                      a time (z -> 2 values, y -> 3 values per column, x -> the 4 channels), float4 rows.
//
// Grids write four consecutive volumes of nx * ny * nz samples (value, d/dx, d/dy, d/dz), each in wn_eval3d_grid's layout.
// The gradient is taken with respect to the coordinate the sample passes to evaluate3D (multiband: the lattice coordinate
// p), and out_scale multiplies all four channels last.
#include "wn_brick.hpp"

#include <algorithm>
#include <cmath>

namespace {

using wn::GridArgs;
using wn::kMaxBands;

// ---- point lists -----------------------------------------------------------------------------------------------------
struct GradPointsArgs : wn::Bands {
    const float *coef;
    int n, nmask;
    const float *pts; // xyz interleaved
    v4f *out;         // {value, d/dx, d/dy, d/dz} per point
    size_t count;
};

template <bool PADDED, bool MB>
__global__ __launch_bounds__(256) void grad3d_points_kernel(const GradPointsArgs a)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.count; i += (size_t)gridDim.x * blockDim.x) {
        const float p[3] = {a.pts[3 * i], a.pts[3 * i + 1], a.pts[3 * i + 2]};
        float g[3];
        const float v = MB ? wn::multiband_exact<PADDED, false, true>(a, p, nullptr, g)
                           : wn::eval3d_grad_exact<PADDED>(a.coef, a.n, a.nmask, p[0], p[1], p[2], g);
        a.out[i] = v4f{v, g[0], g[1], g[2]};
    }
}

// ---- dense grids, exact tier ---------------------------------------------------------------------------------------------
struct GradDirectArgs : wn::Bands { // nbands == 0: plain evaluate3D
    const float *coef;
    float *out;
    size_t vol; // samples per channel volume
    int n, nmask;
    GridArgs g;
};

template <bool PADDED>
__global__ __launch_bounds__(256) void grad3d_grid_direct_kernel(const GradDirectArgs a)
{
    const GridArgs &g = a.g;
    const float den = (float)g.den;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < a.vol; e += (size_t)gridDim.x * blockDim.x) {
        float p[3], gr[3];
        wn::lattice_point(g, den, e, p);
        const float v = a.nbands == 0 ? wn::eval3d_grad_exact<PADDED>(a.coef, a.n, a.nmask, p[0], p[1], p[2], gr)
                                      : wn::multiband_exact<PADDED, false, true>(a, p, nullptr, gr);
        a.out[e] = v * g.out_scale;
        a.out[e + a.vol] = gr[0] * g.out_scale;
        a.out[e + 2 * a.vol] = gr[1] * g.out_scale;
        a.out[e + 3 * a.vol] = gr[2] * g.out_scale;
    }
}

// ---- dense grids, default tier: the separable brick kernel ---------------------------------------------------------------
// The brick frame of wn_brick.hpp with one coefficient box per band.  Per row and band the lane contracts the 4 box
// columns under its samples' taps with the gradient contraction stated there (z, then y, written out here from wn::tap3
// for the reason given there; then wn::grad_x in the 4-wide window), and stores a float4 per channel.  Every sample is
// summed in the same order from its own weights and coefficients, wherever it sits in a brick: its bits do not depend
// on how the volume was cut into z-slabs.  Fused (FMA) arithmetic; within 1e-5 scaled.
using wn::kGWaves;
using wn::kGX;
using wn::kGY;
using wn::kGZ;
constexpr int kGMaxBoxFloats = 12 * 1024; // 48 KB of LDS for all bands' boxes

struct GradBand : wn::BrickBand {
    float fv, fg; // factors of its value and of its gradient: w_b / out_div * out_scale, and that * qmul
};

struct GradSepArgs {
    const float *coef; // linear tile
    float *out;
    size_t vol;
    int n, nmask;
    GridArgs g;
    int vec4_ok;
    GradBand band[kMaxBands];
};

template <int NB>
__global__ __launch_bounds__(64 * kGWaves) void grad3d_grid_sep_kernel(const GradSepArgs a)
{
    extern __shared__ float box[];
    __shared__ int s_geo[NB][6]; // per band: ix0, jy0, kz0, ex, ey, ez
    const GridArgs &g = a.g;
    const float den = (float)g.den;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int x_first = blockIdx.x * kGX, y_first = blockIdx.y * kGY, z_first = blockIdx.z * kGZ;
    auto coord = [&](int i) { return wn::grid_coord(g, den, i); };
    auto zcoord = [&](int zi) { return wn::grid_zcoord(g, den, zi); };

    // ---- the boxes: coordinates are monotone in the index, so the mids of an axis's first and last sample bound all of
    // them; one column / row / plane of support on either side, and one more column (the window's fourth, at zero weight)
    if (tid < 3 * NB) {
        const int b = tid / 3, ax = tid - 3 * b;
        const int lo_i = ax == 0 ? x_first : (ax == 1 ? y_first : z_first);
        const int n_i = ax == 0 ? g.nx : (ax == 1 ? g.ny : g.nz);
        const int hi_i = min(lo_i + (ax == 0 ? kGX : (ax == 1 ? kGY : kGZ)), n_i) - 1;
        const float qm = a.band[b].qmul;
        const float c_lo = (ax == 2 ? zcoord(lo_i) : coord(lo_i)) * qm, c_hi = (ax == 2 ? zcoord(hi_i) : coord(hi_i)) * qm;
        int m_lo, m_hi;
        float w0, w1, w2;
        wn::bspline(c_lo, m_lo, w0, w1, w2);
        wn::bspline(c_hi, m_hi, w0, w1, w2);
        s_geo[b][ax] = min(m_lo, m_hi) - 1;
        s_geo[b][3 + ax] = abs(m_hi - m_lo) + (ax == 0 ? 4 : 3);
    }
    __syncthreads();

    // ---- fill: box_b[k][j][i] = coef[Mod(kz0+k)][Mod(jy0+j)][Mod(ix0+i)]
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        if (!wn::brick_box_fits(s_geo[b], a.band[b].box_cap)) return; // never
        wn::brick_fill(box + a.band[b].box_off, a.coef, a.n, a.nmask, s_geo[b], 0, 0, 0, wave, lane);
    }

    // ---- x: this lane's 4 samples (coordinates once: the bands scale them) in a 4-column window per band
    const int x0 = x_first + lane * 4;
    float px[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) px[q] = coord(min(x0 + q, g.nx - 1));
    wn::XWin xw1;
    if (NB == 1) wn::brick_x_window(px, a.band[0].qmul, s_geo[0][0], xw1);
    __syncthreads();

    const int rows_y = min(kGY, g.ny - y_first), rows_z = min(kGZ, g.nz - z_first);
    for (int r = wave; r < rows_y * rows_z; r += kGWaves) {
        const int yi = r % rows_y, zi = r / rows_y;
        const float py = coord(y_first + yi), pz = zcoord(z_first + zi);
        float acc[4][4] = {}; // [channel][sample]
        // bands one after the other (not unrolled: each band's x window is live only inside its iteration)
#pragma unroll 1
        for (int b = 0; b < NB; ++b) {
            const float qm = a.band[b].qmul;
            wn::XWin xwb;
            if (NB != 1) wn::brick_x_window(px, qm, s_geo[b][0], xwb);
            const wn::XWin &xw = NB == 1 ? xw1 : xwb;
            int my, mz;
            float wy[3], dy[3], wz[3], dz[3];
            wn::bspline_grad(py * qm, my, wy, dy);
            wn::bspline_grad(pz * qm, mz, wz, dz);
            const int ex = s_geo[b][3], ey = s_geo[b][4];
            const float *base = box + a.band[b].box_off + ((mz - 1 - s_geo[b][2]) * ey + (my - 1 - s_geo[b][1])) * ex + xw.col;
            float A[4], B[4], D[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float zw[3], zd[3];
#pragma unroll
                for (int fy = 0; fy < 3; ++fy) {
                    const float c0 = base[(0 * ey + fy) * ex + c], c1 = base[(1 * ey + fy) * ex + c], c2 = base[(2 * ey + fy) * ex + c];
                    zw[fy] = wn::tap3(wz, c0, c1, c2);
                    zd[fy] = wn::tap3(dz, c0, c1, c2);
                }
                A[c] = wn::tap3(wy, zw[0], zw[1], zw[2]);
                B[c] = wn::tap3(dy, zw[0], zw[1], zw[2]);
                D[c] = wn::tap3(wy, zd[0], zd[1], zd[2]);
            }
            const float fv = a.band[b].fv, fg = a.band[b].fg;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const wn::GradSample s = wn::grad_x(xw.w[q], xw.d[q], A, B, D);
                acc[0][q] = __builtin_fmaf(fv, s.v, acc[0][q]);
                acc[1][q] = __builtin_fmaf(fg, s.gx, acc[1][q]);
                acc[2][q] = __builtin_fmaf(fg, s.gy, acc[2][q]);
                acc[3][q] = __builtin_fmaf(fg, s.gz, acc[3][q]);
            }
        }
        float *dst = a.out + ((size_t)(z_first + zi) * g.ny + (y_first + yi)) * g.nx + x0;
        wn::brick_store_row(dst, a.vol, a.vec4_ok, x0, g.nx, acc);
    }
}

// Launches the brick kernel when the lattice is in its regime (wn::brick_plan) with boxes that fit 48 KB of LDS (never
// binding inside two_mids: <= 3.2 K floats for one band, < 2x that for eight; no opt-in needed).  nbands bands with
// coordinate multipliers qmul[b] and the factors of value and gradient.
int grad_sep_try(const wn_tile *tile, const GridArgs &g, int nbands, const float *qmul, const float *fv, const float *fg,
                 float *out_dev, hipStream_t stream)
{
    GradSepArgs a{};
    dim3 grid;
    size_t lds;
    if (!wn::brick_plan(tile, g, nbands, qmul, 1, kGMaxBoxFloats, out_dev, &a, &grid, &lds)) return wn::kDeclined;
    for (int b = 0; b < nbands; ++b) {
        a.band[b].fv = fv[b];
        a.band[b].fg = fg[b];
    }
    wn::brick_dispatch(nbands, [&](auto nb) {
        hipLaunchKernelGGL(grad3d_grid_sep_kernel<decltype(nb)::value>, grid, dim3(64 * kGWaves), lds, stream, a);
        return WN_OK;
    });
    WN_LAUNCH_CHECK("grad3d_grid_sep_kernel");
    return WN_OK;
}

// The grid entry points after their tile (and band) checks; d carries the bands of a multiband call (mb).  The brick
// kernel (nbands >= 1) unless the caller asks for WN_GRID_EXACT or it declines, then the exact kernel on the tile's padded
// copy when it has one.
int grad_grid(const wn_tile *tile, const wn_grid *grid, GradDirectArgs d, bool mb, float *out_dev, hipStream_t stream)
{
    GridArgs g;
    int rc = wn::check_grid(grid, true, &g);
    if (rc) return rc;
    d.vol = (size_t)g.nx * g.ny * g.nz;
    if (d.vol == 0) return WN_OK;
    if (!out_dev) return wn::fail(WN_ERR_INVALID, "out_dev is NULL");
    if (!(grid->flags & WN_GRID_EXACT) && (!mb || d.nbands >= 1)) {
        const wn::BandFactors f = wn::band_factors(d, mb, g.out_scale);
        if ((rc = grad_sep_try(tile, g, f.nbands, f.qmul, f.fv, f.fg, out_dev, stream)) != wn::kDeclined) return rc;
    }
    if (mb) d.zero_band_if_none();
    d.coef = tile->dev_padded ? tile->dev_padded : tile->dev;
    d.out = out_dev;
    d.n = tile->n;
    d.nmask = wn::pow2_mask(tile->n);
    d.g = g;
    const dim3 blocks(wn::stride_blocks(d.vol)), block(256);
    if (tile->dev_padded) hipLaunchKernelGGL(grad3d_grid_direct_kernel<true>, blocks, block, 0, stream, d);
    else hipLaunchKernelGGL(grad3d_grid_direct_kernel<false>, blocks, block, 0, stream, d);
    WN_LAUNCH_CHECK(mb ? "grad3d_grid_direct_kernel(multiband)" : "grad3d_grid_direct_kernel");
    return WN_OK;
}

// The arguments every gradient entry point checks: the tile (wn::check_tile), and out4_dev 16-byte aligned for points.
int grad_points_args(const wn_tile *tile, const float *xyz_dev, size_t n, float *out4_dev, const char *entry,
                     GradPointsArgs *a)
{
    const int rc = wn::check_tile(tile, 3, entry);
    if (rc) return rc;
    *a = GradPointsArgs{};
    a->coef = tile->dev_padded ? tile->dev_padded : tile->dev;
    a->n = tile->n;
    a->nmask = wn::pow2_mask(tile->n);
    a->pts = xyz_dev;
    a->out = reinterpret_cast<v4f *>(out4_dev);
    a->count = n;
    return WN_OK;
}

int launch_grad_points(const wn_tile *tile, const GradPointsArgs &a, bool mb, hipStream_t stream)
{
    if (!a.pts || !a.out) return wn::fail(WN_ERR_INVALID, "points/out pointer is NULL");
    if (reinterpret_cast<uintptr_t>(a.out) & 15) return wn::fail(WN_ERR_INVALID, "out4_dev must be 16-byte aligned");
    const dim3 grid(wn::stride_blocks(a.count)), block(256);
    const bool padded = tile->dev_padded != nullptr;
    if (mb) {
        if (padded) hipLaunchKernelGGL((grad3d_points_kernel<true, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((grad3d_points_kernel<false, true>), grid, block, 0, stream, a);
    } else {
        if (padded) hipLaunchKernelGGL((grad3d_points_kernel<true, false>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((grad3d_points_kernel<false, false>), grid, block, 0, stream, a);
    }
    WN_LAUNCH_CHECK("grad3d_points_kernel");
    return WN_OK;
}

} // namespace

using namespace wn;

extern "C" {

int wn_eval3d_grad_points(const wn_tile *tile, const float *xyz_dev, size_t n, float *out4_dev, void *stream)
{
    WN_ENTRY();
    GradPointsArgs a;
    const int rc = grad_points_args(tile, xyz_dev, n, out4_dev, "wn_eval3d_grad_points", &a);
    if (rc || n == 0) return rc;
    return launch_grad_points(tile, a, false, as_stream(stream));
}

int wn_multiband3d_grad_points(const wn_tile *tile, const float *xyz_dev, size_t n, float s, int first_band, int nbands,
                               const float *w_host, float var_per_band, float *out4_dev, void *stream)
{
    WN_ENTRY();
    GradPointsArgs a;
    int rc = grad_points_args(tile, xyz_dev, n, out4_dev, "wn_multiband3d_grad_points", &a);
    if (rc) return rc;
    rc = multiband_bands(s, first_band, nbands, w_host, var_per_band, &a);
    if (rc || n == 0) return rc;
    return launch_grad_points(tile, a, true, as_stream(stream));
}

int wn_eval3d_grad_grid(const wn_tile *tile, const wn_grid *grid, float *out_dev, void *stream)
{
    WN_ENTRY();
    const int rc = check_tile(tile, 3, "wn_eval3d_grad_grid");
    if (rc) return rc;
    return grad_grid(tile, grid, GradDirectArgs{}, false, out_dev, as_stream(stream));
}

int wn_multiband3d_grad_grid(const wn_tile *tile, const wn_grid *grid, float s, int first_band, int nbands,
                             const float *w_host, float var_per_band, float *out_dev, void *stream)
{
    WN_ENTRY();
    int rc = check_tile(tile, 3, "wn_multiband3d_grad_grid");
    if (rc) return rc;
    GradDirectArgs d{};
    rc = multiband_bands(s, first_band, nbands, w_host, var_per_band, &d);
    if (rc) return rc;
    return grad_grid(tile, grid, d, true, out_dev, as_stream(stream));
}

} // extern "C"
