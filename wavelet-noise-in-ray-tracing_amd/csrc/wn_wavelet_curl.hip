// wn_wavelet_curl.hip -- divergence-free curl noise from 3-D wavelet noise potentials, on point lists and dense grids.
//
// The vector potential Psi = (psi0, psi1, psi2) is evaluate3D (or WMultibandNoise, normal == NULL) of three whole-cell
// shifts of ONE tile: psi_k reads C[Mod(z+oz_k)][Mod(y+oy_k)][Mod(x+ox_k)].  The velocity is
//     v = curl Psi = (d psi2/dy - d psi1/dz, d psi0/dz - d psi2/dx, d psi1/dx - d psi0/dy).
// The tensor-product quadratic B-spline is C1 and its mixed second partials commute: div v = 0, v continuous across cell
// faces.  Whole-cell shifts leave a sample's mids, weights and derivatives alone: bspline_grad runs once per axis for the
// three potentials; six derivative sums, three output channels.
//
//   curl3d_points_kernel<PADDED, MB>   one point per lane, wn::eval3d_curl_exact / multiband_curl_exact (every component has
//                                      the bits of the subtraction of two channels of wn_eval3d_grad_points /
//                                      wn_multiband3d_grad_points on the shifted tiles), records {vx, vy, vz}.
//   curl3d_grid_direct_kernel<PADDED>  WN_GRID_EXACT and every lattice the brick kernel declines: one sample per lane, the
//                                      point kernel's device function at lattice_coord's coordinates; three volumes.
//   curl3d_grid_sep_kernel<NB>         the default tier: per band three coefficient boxes (one per potential) staged in LDS,
//                                      contracted one axis at a time, float4 rows.
//
// Grids write three consecutive volumes of nx * ny * nz samples (vx, vy, vz), each in wn_eval3d_grid's layout.  Derivatives
// are taken with respect to the coordinate the sample passes to evaluate3D (multiband: the lattice coordinate p), and
// out_scale multiplies all three channels last.
#include "wn_brick.hpp"

#include <algorithm>
#include <cmath>

namespace {

using wn::GridArgs;
using wn::CurlEval;
using wn::curl_eval_args;
using wn::kMaxBands;

// ---- point lists -----------------------------------------------------------------------------------------------------
struct CurlPointsArgs {
    CurlEval e;
    const float *pts; // xyz interleaved
    float *out;       // {vx, vy, vz} per point
    size_t count;
};

template <bool PADDED, bool MB>
__global__ __launch_bounds__(256) void curl3d_points_kernel(const CurlPointsArgs a)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.count; i += (size_t)gridDim.x * blockDim.x) {
        const float p[3] = {a.pts[3 * i], a.pts[3 * i + 1], a.pts[3 * i + 2]};
        float v[3];
        if (MB) wn::multiband_curl_exact<PADDED>(a.e, p, v);
        else wn::eval3d_curl_exact<PADDED>(a.e.coef, a.e.n, a.e.nmask, a.e.off, p[0], p[1], p[2], v);
        a.out[3 * i] = v[0];
        a.out[3 * i + 1] = v[1];
        a.out[3 * i + 2] = v[2];
    }
}

// ---- dense grids, exact tier ---------------------------------------------------------------------------------------------
struct CurlDirectArgs {
    CurlEval e;
    float *out;
    size_t vol; // samples per channel volume
    GridArgs g;
};

template <bool PADDED>
__global__ __launch_bounds__(256) void curl3d_grid_direct_kernel(const CurlDirectArgs a)
{
    const GridArgs &g = a.g;
    const float den = (float)g.den;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < a.vol; e += (size_t)gridDim.x * blockDim.x) {
        float p[3], v[3];
        wn::lattice_point(g, den, e, p);
        if (a.e.mb) wn::multiband_curl_exact<PADDED>(a.e, p, v);
        else wn::eval3d_curl_exact<PADDED>(a.e.coef, a.e.n, a.e.nmask, a.e.off, p[0], p[1], p[2], v);
        a.out[e] = v[0] * g.out_scale;
        a.out[e + a.vol] = v[1] * g.out_scale;
        a.out[e + 2 * a.vol] = v[2] * g.out_scale;
    }
}

// ---- dense grids, default tier: the separable brick kernel ---------------------------------------------------------------
// The brick frame of wn_brick.hpp.  Per band the workgroup stages THREE boxes, box_k[k][j][i] = coef[Mod(kz0+k+oz_k)]
// [Mod(jy0+j+oy_k)][Mod(ix0+i+ox_k)], of one geometry (the potentials share the mids), and the lane forms the 4-wide x
// window (Wx, Dx) once.  Per row and band the lane contracts the 4 box columns under its samples' taps with the curl
// contraction stated in wn_brick.hpp (two of the three column contractions per potential, written out here from wn::tap3
// for the reason given there; then wn::curl_x, the components accumulated with signs).  Every sample is summed in the same order from its own weights and
// coefficients, wherever it sits in a brick: its bits do not depend on how the volume was cut into z-slabs.  Fused (FMA)
// arithmetic.
using wn::kGWaves;
using wn::kGX;
using wn::kGY;
using wn::kGZ;
// LDS: one band's three boxes are at most 3 x 3.2 K floats inside two_mids, eight bands' less than twice that (each lower
// band's step halves): < 77 KB.  Up to 48 KB the launch needs nothing; beyond, the kernel is opted in to the request
// (wn::ensure_dynamic_lds; the CU has 160 KB, so two workgroups still share one).  The cap never binds inside two_mids.
constexpr int kCMaxBoxFloats = 36 * 1024; // 144 KB
constexpr size_t kLdsNoOptIn = 48 * 1024;

struct CurlBand : wn::BrickBand { // potential k's box is box k
    float fg; // factor of its derivatives: out_scale, or w_b / out_div * out_scale * qmul
};

struct CurlSepArgs {
    const float *coef; // linear tile
    float *out;
    size_t vol;
    int n, nmask;
    int off[9];
    GridArgs g;
    int vec4_ok;
    CurlBand band[kMaxBands];
};

template <int NB>
__global__ __launch_bounds__(64 * kGWaves) void curl3d_grid_sep_kernel(const CurlSepArgs a)
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

    // ---- the boxes' geometry (shared by the three potentials): the mids of an axis's first and last sample bound all of
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

    // ---- fill: a potential's box is the tile's, shifted by its offsets
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        if (!wn::brick_box_fits(s_geo[b], a.band[b].box_cap)) return; // never
#pragma unroll 1
        for (int k3 = 0; k3 < 3; ++k3)
            wn::brick_fill(box + a.band[b].box_off + k3 * a.band[b].box_cap, a.coef, a.n, a.nmask, s_geo[b], a.off[3 * k3],
                           a.off[3 * k3 + 1], a.off[3 * k3 + 2], wave, lane);
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
        float acc[3][4] = {}; // [component][sample]
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
            const int cap = a.band[b].box_cap;
            const float *base = box + a.band[b].box_off + ((mz - 1 - s_geo[b][2]) * ey + (my - 1 - s_geo[b][1])) * ex + xw.col;
            // per window column (wn_brick.hpp): P = B2 - D1 (for vx), D0 and A2 (vy), A1 and B0 (vz)
            wn::CurlColumns cols;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float zw[3][3], zd[2][3]; // [potential][fy]: Z for all three, Z' for psi0 and psi1
#pragma unroll
                for (int k3 = 0; k3 < 3; ++k3)
#pragma unroll
                    for (int fy = 0; fy < 3; ++fy) {
                        const float *bk = base + k3 * cap;
                        const float c0 = bk[(0 * ey + fy) * ex + c], c1 = bk[(1 * ey + fy) * ex + c], c2 = bk[(2 * ey + fy) * ex + c];
                        zw[k3][fy] = wn::tap3(wz, c0, c1, c2);
                        if (k3 < 2) zd[k3][fy] = wn::tap3(dz, c0, c1, c2);
                    }
                cols.B0[c] = wn::tap3(dy, zw[0][0], zw[0][1], zw[0][2]);
                cols.D0[c] = wn::tap3(wy, zd[0][0], zd[0][1], zd[0][2]);
                cols.A1[c] = wn::tap3(wy, zw[1][0], zw[1][1], zw[1][2]);
                const float D1 = wn::tap3(wy, zd[1][0], zd[1][1], zd[1][2]);
                cols.A2[c] = wn::tap3(wy, zw[2][0], zw[2][1], zw[2][2]);
                const float B2 = wn::tap3(dy, zw[2][0], zw[2][1], zw[2][2]);
                cols.P[c] = B2 - D1;
                // one column's 27 LDS reads in flight, not all 108: 127 VGPRs (4 waves per SIMD) instead of 170 (2); measured
                // 597 against 742 us at 512^3 (profiles/curl_kernels.txt)
                __builtin_amdgcn_sched_barrier(0);
            }
            const float fg = a.band[b].fg;
#pragma unroll
            for (int q = 0; q < 4; ++q) wn::curl_x(xw.w[q], xw.d[q], cols, fg, acc, q);
        }
        float *dst = a.out + ((size_t)(z_first + zi) * g.ny + (y_first + yi)) * g.nx + x0;
        wn::brick_store_row(dst, a.vol, a.vec4_ok, x0, g.nx, acc);
    }
}

constexpr size_t kPointBlockCap = 256u * 8u;  // of the point kernel's: its lanes hold 27 row loads each

// Launches the brick kernel when the lattice is in its regime (wn::brick_plan, three boxes per band) and the runtime grants
// the boxes' LDS (see kCMaxBoxFloats); when it refuses, the exact kernel serves the lattice.  nbands bands with coordinate
// multipliers qmul[b] and the factors fg[b] of their derivatives.
int curl_sep_try(const wn_tile *tile, const GridArgs &g, const int off[9], int nbands, const float *qmul, const float *fg,
                 float *out_dev, hipStream_t stream)
{
    CurlSepArgs a{};
    dim3 grid;
    size_t lds;
    if (!wn::brick_plan(tile, g, nbands, qmul, 3, kCMaxBoxFloats, out_dev, &a, &grid, &lds)) return wn::kDeclined;
    for (int b = 0; b < nbands; ++b) a.band[b].fg = fg[b];
    std::copy(off, off + 9, a.off);
    return wn::brick_dispatch(nbands, [&](auto nb) {
        constexpr auto kernel = curl3d_grid_sep_kernel<decltype(nb)::value>;
        if (lds > kLdsNoOptIn && !wn::ensure_dynamic_lds(reinterpret_cast<const void *>(kernel), wn::current_device(), lds))
            return (int)wn::kDeclined;
        hipLaunchKernelGGL(kernel, grid, dim3(64 * kGWaves), lds, stream, a);
        WN_LAUNCH_CHECK("curl3d_grid_sep_kernel");
        return (int)WN_OK;
    });
}

int launch_curl_points(const wn_tile *tile, const CurlEval &e, const float *xyz_dev, size_t n, float *out3_dev,
                       hipStream_t stream)
{
    if (!xyz_dev || !out3_dev) return wn::fail(WN_ERR_INVALID, "points/out pointer is NULL");
    CurlPointsArgs a{e, xyz_dev, out3_dev, n};
    const dim3 grid(wn::stride_blocks(n, kPointBlockCap)), block(256);
    const bool padded = tile->dev_padded != nullptr;
    if (e.mb) {
        if (padded) hipLaunchKernelGGL((curl3d_points_kernel<true, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((curl3d_points_kernel<false, true>), grid, block, 0, stream, a);
    } else {
        if (padded) hipLaunchKernelGGL((curl3d_points_kernel<true, false>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((curl3d_points_kernel<false, false>), grid, block, 0, stream, a);
    }
    WN_LAUNCH_CHECK("curl3d_points_kernel");
    return WN_OK;
}

// The grid entry points after their argument checks: the brick kernel (bands given by qmul / fg, nbands >= 1) unless the
// caller asks for WN_GRID_EXACT or it declines, then the exact kernel.
int curl_grid(const wn_tile *tile, const wn_grid *grid, const CurlEval &e, float *out_dev, hipStream_t stream)
{
    GridArgs g;
    int rc = wn::check_grid(grid, true, &g);
    if (rc) return rc;
    const size_t total = (size_t)g.nx * g.ny * g.nz;
    if (total == 0) return WN_OK;
    if (!out_dev) return wn::fail(WN_ERR_INVALID, "out_dev is NULL");
    if (!(grid->flags & WN_GRID_EXACT) && (!e.mb || e.nbands >= 1)) {
        const wn::BandFactors f = wn::band_factors(e, e.mb, g.out_scale);
        if ((rc = curl_sep_try(tile, g, e.off, f.nbands, f.qmul, f.fg, out_dev, stream)) != wn::kDeclined) return rc;
    }
    CurlDirectArgs d{e, out_dev, total, g};
    const dim3 blocks(wn::stride_blocks(total)), block(256);
    if (tile->dev_padded) hipLaunchKernelGGL(curl3d_grid_direct_kernel<true>, blocks, block, 0, stream, d);
    else hipLaunchKernelGGL(curl3d_grid_direct_kernel<false>, blocks, block, 0, stream, d);
    WN_LAUNCH_CHECK("curl3d_grid_direct_kernel");
    return WN_OK;
}

} // namespace

using namespace wn;

extern "C" {

int wn_eval3d_curl_points(const wn_tile *tile, const float *xyz_dev, size_t n, const int32_t *offsets9_host, float *out3_dev,
                          void *stream)
{
    WN_ENTRY();
    CurlEval e;
    const int rc = curl_eval_args(tile, offsets9_host, "wn_eval3d_curl_points", &e);
    if (rc || n == 0) return rc;
    return launch_curl_points(tile, e, xyz_dev, n, out3_dev, as_stream(stream));
}

int wn_multiband3d_curl_points(const wn_tile *tile, const float *xyz_dev, size_t n, const int32_t *offsets9_host, float s,
                               int first_band, int nbands, const float *w_host, float var_per_band, float *out3_dev,
                               void *stream)
{
    WN_ENTRY();
    CurlEval e;
    int rc = curl_eval_args(tile, offsets9_host, "wn_multiband3d_curl_points", &e);
    if (rc) return rc;
    rc = multiband_bands(s, first_band, nbands, w_host, var_per_band, &e);
    if (rc || n == 0) return rc;
    e.mb = 1;
    return launch_curl_points(tile, e, xyz_dev, n, out3_dev, as_stream(stream));
}

int wn_eval3d_curl_grid(const wn_tile *tile, const wn_grid *grid, const int32_t *offsets9_host, float *out_dev, void *stream)
{
    WN_ENTRY();
    CurlEval e;
    const int rc = curl_eval_args(tile, offsets9_host, "wn_eval3d_curl_grid", &e);
    if (rc) return rc;
    return curl_grid(tile, grid, e, out_dev, as_stream(stream));
}

int wn_multiband3d_curl_grid(const wn_tile *tile, const wn_grid *grid, const int32_t *offsets9_host, float s, int first_band,
                             int nbands, const float *w_host, float var_per_band, float *out_dev, void *stream)
{
    WN_ENTRY();
    CurlEval e;
    int rc = curl_eval_args(tile, offsets9_host, "wn_multiband3d_curl_grid", &e);
    if (rc) return rc;
    rc = multiband_bands(s, first_band, nbands, w_host, var_per_band, &e);
    if (rc) return rc;
    e.mb = 1;
    return curl_grid(tile, grid, e, out_dev, as_stream(stream));
}

} // extern "C"
