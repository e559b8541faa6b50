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
#include "wn_internal.hpp"

#include <algorithm>
#include <cmath>

namespace {

using wn::GridArgs;
using wn::kMaxBands;

typedef float v4f __attribute__((ext_vector_type(4)));

// ---- point lists -----------------------------------------------------------------------------------------------------
struct GradPointsArgs {
    const float *coef;
    int n, nmask;
    const float *pts; // xyz interleaved
    v4f *out;         // {value, d/dx, d/dy, d/dz} per point
    size_t count;
    // multiband (wn::multiband_bands)
    int nbands;
    float band_scale[kMaxBands], band_w[kMaxBands];
    float out_div;
    int apply_div;
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
struct GradDirectArgs {
    const float *coef;
    float *out;
    size_t vol; // samples per channel volume
    int n, nmask;
    GridArgs g;
    // multiband (nbands == 0: plain evaluate3D)
    int nbands;
    float band_scale[kMaxBands], band_w[kMaxBands];
    float out_div;
    int apply_div;
};

template <bool PADDED>
__global__ __launch_bounds__(256) void grad3d_grid_direct_kernel(const GradDirectArgs a)
{
    const GridArgs &g = a.g;
    const float den = (float)g.den;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < a.vol; e += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(e % g.nx);
        const size_t r = e / g.nx;
        const int y = (int)(r % g.ny), z = (int)(r / g.ny);
        const float p[3] = {wn::lattice_coord(x, den, g.base_range, g.octave_scale, g.post_scale),
                            wn::lattice_coord(y, den, g.base_range, g.octave_scale, g.post_scale),
                            g.z_const_mode ? g.z_const
                                           : wn::lattice_coord(g.z0 + z, den, g.base_range, g.octave_scale, g.post_scale)};
        float gr[3];
        const float v = a.nbands == 0 ? wn::eval3d_grad_exact<PADDED>(a.coef, a.n, a.nmask, p[0], p[1], p[2], gr)
                                      : wn::multiband_exact<PADDED, false, true>(a, p, nullptr, gr);
        a.out[e] = v * g.out_scale;
        a.out[e + a.vol] = gr[0] * g.out_scale;
        a.out[e + 2 * a.vol] = gr[1] * g.out_scale;
        a.out[e + 3 * a.vol] = gr[2] * g.out_scale;
    }
}

// ---- dense grids, default tier: the separable brick kernel ---------------------------------------------------------------
// A workgroup (4 waves) owns a brick of 256 x 8 x 8 samples.  For every band it stages the brick's coefficient box in LDS
// (periodic wrap resolved, x fastest) once.  A lane owns 4 consecutive x samples, a wave rows (y, z) of the brick.  Per
// row and band the lane contracts the 4 box columns under its samples' taps (4 consecutive samples span at most two mids:
// columns m0 - 1 .. m0 + 2):
//     z:  Z = sum_k wz_k C[k][j][i],  Z' = sum_k dz_k C[k][j][i]             (2 values per (j, i))
//     y:  A = sum_j wy_j Z,  B = sum_j dy_j Z,  D = sum_j wy_j Z'           (3 values per column i)
//     x:  value = sum_i Wx_i A, d/dx = sum_i Dx_i A, d/dy = sum_i Wx_i B, d/dz = sum_i Wx_i D
// with the x weights of each sample placed in a 4-wide window (Wx, Dx: zero outside its three taps), and stores a float4
// per channel.  Every sample is summed in the same order from its own weights and coefficients, wherever it sits in a
// brick: its bits do not depend on how the volume was cut into z-slabs.  Fused (FMA) arithmetic; within 1e-5 scaled.
constexpr int kGX = 256, kGY = 8, kGZ = 8; // samples per brick
constexpr int kGWaves = 4;
constexpr int kGMaxBoxFloats = 12 * 1024; // 48 KB of LDS for all bands' boxes

struct GradBand {
    float qmul;   // the band's coordinate is q = p * qmul (1; multiband 2 * 2^(first_band+b): exact)
    float fv, fg; // factors of its value and of its gradient: w_b / out_div * out_scale, and that * qmul
    int box_off;  // float offset of its box in dynamic LDS
    int box_cap;  // floats reserved for it
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
    auto coord = [&](int i) { return wn::lattice_coord(i, den, g.base_range, g.octave_scale, g.post_scale); };
    auto zcoord = [&](int zi) { return g.z_const_mode ? g.z_const : coord(g.z0 + zi); };

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

    // ---- fill: box_b[k][j][i] = coef[Mod(kz0+k)][Mod(jy0+j)][Mod(ix0+i)]; a wave takes whole (k, j) rows
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int ix0 = s_geo[b][0], jy0 = s_geo[b][1], kz0 = s_geo[b][2];
        const int ex = s_geo[b][3], ey = s_geo[b][4], ez = s_geo[b][5];
        if ((long long)ex * ey * ez > a.band[b].box_cap) return; // never: the host bounds the box (memory safety); uniform
        float *bb = box + a.band[b].box_off;
        for (int r = wave; r < ey * ez; r += kGWaves) {
            const int k = r / ey, j = r - k * ey;
            const float *row = a.coef + ((size_t)wn::dmod(kz0 + k, a.n, a.nmask) * a.n + wn::dmod(jy0 + j, a.n, a.nmask)) * a.n;
            for (int i = lane; i < ex; i += 64) bb[r * ex + i] = row[wn::dmod(ix0 + i, a.n, a.nmask)];
        }
    }

    // ---- x: this lane's 4 samples (coordinates once: the bands scale them) in a 4-column window per band
    const int x0 = x_first + lane * 4;
    float px[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) px[q] = coord(min(x0 + q, g.nx - 1));
    struct XWin { int col; float w[4][4], d[4][4]; }; // window's first box column; per sample q the window's weights
    auto x_window = [&](int b, XWin &xw) {
        int m[4];
        float w[4][3], d[4][3];
#pragma unroll
        for (int q = 0; q < 4; ++q) wn::bspline_grad(px[q] * a.band[b].qmul, m[q], w[q], d[q]);
        xw.col = m[0] - 1 - s_geo[b][0];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const bool sh = m[q] != m[0]; // then m[q] == m[0] + 1 (the host's two_mids)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                xw.w[q][c] = sh ? (c == 0 ? 0.0f : w[q][c - 1]) : (c == 3 ? 0.0f : w[q][c]);
                xw.d[q][c] = sh ? (c == 0 ? 0.0f : d[q][c - 1]) : (c == 3 ? 0.0f : d[q][c]);
            }
        }
    };
    XWin xw1;
    if (NB == 1) x_window(0, xw1);
    __syncthreads();

    const int rows_y = min(kGY, g.ny - y_first), rows_z = min(kGZ, g.nz - z_first);
    for (int r = wave; r < rows_y * rows_z; r += kGWaves) {
        const int yi = r % rows_y, zi = r / rows_y;
        const float py = coord(y_first + yi), pz = zcoord(z_first + zi);
        float acc[4][4] = {}; // [channel][sample]
        // bands one after the other (not unrolled: each band's x window is live only inside its iteration)
#pragma unroll 1
        for (int b = 0; b < NB; ++b) {
            XWin xwb;
            if (NB != 1) x_window(b, xwb);
            const XWin &xw = NB == 1 ? xw1 : xwb;
            const float qm = a.band[b].qmul;
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
                    zw[fy] = __builtin_fmaf(wz[2], c2, __builtin_fmaf(wz[1], c1, wz[0] * c0));
                    zd[fy] = __builtin_fmaf(dz[2], c2, __builtin_fmaf(dz[1], c1, dz[0] * c0));
                }
                A[c] = __builtin_fmaf(wy[2], zw[2], __builtin_fmaf(wy[1], zw[1], wy[0] * zw[0]));
                B[c] = __builtin_fmaf(dy[2], zw[2], __builtin_fmaf(dy[1], zw[1], dy[0] * zw[0]));
                D[c] = __builtin_fmaf(wy[2], zd[2], __builtin_fmaf(wy[1], zd[1], wy[0] * zd[0]));
            }
            const float fv = a.band[b].fv, fg = a.band[b].fg;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float v = 0.0f, gx = 0.0f, gy = 0.0f, gz = 0.0f;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    v = __builtin_fmaf(xw.w[q][c], A[c], v);
                    gx = __builtin_fmaf(xw.d[q][c], A[c], gx);
                    gy = __builtin_fmaf(xw.w[q][c], B[c], gy);
                    gz = __builtin_fmaf(xw.w[q][c], D[c], gz);
                }
                acc[0][q] = __builtin_fmaf(fv, v, acc[0][q]);
                acc[1][q] = __builtin_fmaf(fg, gx, acc[1][q]);
                acc[2][q] = __builtin_fmaf(fg, gy, acc[2][q]);
                acc[3][q] = __builtin_fmaf(fg, gz, acc[3][q]);
            }
        }
        float *dst = a.out + ((size_t)(z_first + zi) * g.ny + (y_first + yi)) * g.nx + x0;
        if (a.vec4_ok && x0 + 3 < g.nx) {
#pragma unroll
            for (int ch = 0; ch < 4; ++ch)
                *reinterpret_cast<v4f *>(dst + ch * a.vol) = v4f{acc[ch][0], acc[ch][1], acc[ch][2], acc[ch][3]};
        } else {
#pragma unroll
            for (int ch = 0; ch < 4; ++ch)
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (x0 + q < g.nx) dst[ch * a.vol + q] = acc[ch][q];
        }
    }
}

constexpr size_t kBlockCap = 256u * 8u * 8u; // workgroups of a grid-stride launch (wn::stride_blocks)

// Launches the brick kernel when the lattice is in its regime: a tile that is not empty (any size: the box is filled modulo
// n), steps >= 0 at which 4 consecutive samples span at most two mids in every band (wn::LatticeStep::two_mids: step < 1/3
// cell), and boxes that fit 48 KB of LDS (never binding inside two_mids: <= 3.2 K floats for one band, < 2x that for eight).
// Nothing in it depends on how many planes the call computes beyond lattice_step's bound on the coordinates.  nbands
// bands (1..kMaxBands) with coordinate multipliers qmul[b] and the factors of value and gradient.
int grad_sep_try(const wn_tile *tile, const GridArgs &g, int nbands, const float *qmul, const float *fv, const float *fg,
                 float *out_dev, hipStream_t stream)
{
    if (tile->n == 0 || nbands < 1 || nbands > kMaxBands || g.nx <= 0 || g.ny <= 0 || g.nz <= 0) return wn::kDeclined;
    GradSepArgs a{};
    long long box_total = 0;
    for (int b = 0; b < nbands; ++b) {
        wn::LatticeStep ls;
        if (!wn::lattice_step(g, g.octave_scale * qmul[b], true, false, 0.0, &ls) || !ls.two_mids()) return wn::kDeclined;
        const long long ex = ls.extent(kGX) + 1, ey = ls.extent(kGY), ez = g.z_const_mode ? 3 : ls.extent(kGZ);
        a.band[b].qmul = qmul[b];
        a.band[b].fv = fv[b];
        a.band[b].fg = fg[b];
        a.band[b].box_off = (int)box_total;
        a.band[b].box_cap = (int)(ex * ey * ez);
        box_total += ex * ey * ez;
        if (box_total > kGMaxBoxFloats) return wn::kDeclined;
    }
    const int nbx = (g.nx + kGX - 1) / kGX, nby = (g.ny + kGY - 1) / kGY, nbz = (g.nz + kGZ - 1) / kGZ;
    if (nby > 65535 || nbz > 65535) return wn::kDeclined;
    a.coef = tile->dev;
    a.out = out_dev;
    a.vol = (size_t)g.nx * g.ny * g.nz;
    a.n = tile->n;
    a.nmask = wn::pow2_mask(tile->n);
    a.g = g;
    a.vec4_ok = wn::vec4_ok(out_dev, g.nx);
    const size_t lds = (size_t)box_total * sizeof(float); // <= 48 KB: no opt-in needed
    const dim3 grid(nbx, nby, nbz), block(64 * kGWaves);
    switch (nbands) {
    case 1: hipLaunchKernelGGL(grad3d_grid_sep_kernel<1>, grid, block, lds, stream, a); break;
    case 2: hipLaunchKernelGGL(grad3d_grid_sep_kernel<2>, grid, block, lds, stream, a); break;
    case 3: hipLaunchKernelGGL(grad3d_grid_sep_kernel<3>, grid, block, lds, stream, a); break;
    case 4: hipLaunchKernelGGL(grad3d_grid_sep_kernel<4>, grid, block, lds, stream, a); break;
    case 5: hipLaunchKernelGGL(grad3d_grid_sep_kernel<5>, grid, block, lds, stream, a); break;
    case 6: hipLaunchKernelGGL(grad3d_grid_sep_kernel<6>, grid, block, lds, stream, a); break;
    case 7: hipLaunchKernelGGL(grad3d_grid_sep_kernel<7>, grid, block, lds, stream, a); break;
    default: hipLaunchKernelGGL(grad3d_grid_sep_kernel<8>, grid, block, lds, stream, a); break;
    }
    WN_LAUNCH_CHECK("grad3d_grid_sep_kernel");
    return WN_OK;
}

// The exact tier on the tile's padded copy when it has one; the caller checks the launch.
void launch_grad_direct(GradDirectArgs a, const wn_tile *tile, hipStream_t stream)
{
    a.coef = tile->dev_padded ? tile->dev_padded : tile->dev;
    const dim3 grid(wn::stride_blocks(a.vol, kBlockCap)), block(256);
    if (tile->dev_padded) hipLaunchKernelGGL(grad3d_grid_direct_kernel<true>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(grad3d_grid_direct_kernel<false>, grid, block, 0, stream, a);
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
    const dim3 grid(wn::stride_blocks(a.count, kBlockCap)), block(256);
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
    int rc = check_tile(tile, 3, "wn_eval3d_grad_grid");
    if (rc) return rc;
    GridArgs g;
    rc = check_grid(grid, true, &g);
    if (rc) return rc;
    const size_t total = (size_t)g.nx * g.ny * g.nz;
    if (total == 0) return WN_OK;
    if (!out_dev) return fail(WN_ERR_INVALID, "out_dev is NULL");
    const hipStream_t st = as_stream(stream);
    if (!(grid->flags & WN_GRID_EXACT)) {
        const float one = 1.0f, os = g.out_scale;
        if ((rc = grad_sep_try(tile, g, 1, &one, &os, &os, out_dev, st)) != kDeclined) return rc;
    }
    GradDirectArgs d{};
    d.out = out_dev;
    d.vol = total;
    d.n = tile->n;
    d.nmask = pow2_mask(tile->n);
    d.g = g;
    launch_grad_direct(d, tile, st);
    WN_LAUNCH_CHECK("grad3d_grid_direct_kernel");
    return WN_OK;
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
    GridArgs g;
    rc = check_grid(grid, true, &g);
    if (rc) return rc;
    const size_t total = (size_t)g.nx * g.ny * g.nz;
    if (total == 0) return WN_OK;
    if (!out_dev) return fail(WN_ERR_INVALID, "out_dev is NULL");
    const hipStream_t st = as_stream(stream);
    if (!(grid->flags & WN_GRID_EXACT) && d.nbands >= 1) {
        // band b: q = p * (2 * 2^(first_band+b)); value factor w_b / out_div * out_scale, gradient factor that * 2 * 2^(..)
        float qmul[kMaxBands], fv[kMaxBands], fg[kMaxBands];
        for (int b = 0; b < d.nbands; ++b) {
            qmul[b] = 2.0f * d.band_scale[b];
            const double f = (double)d.band_w[b] / (double)d.out_div * (double)g.out_scale;
            fv[b] = (float)f;
            fg[b] = (float)(f * (double)qmul[b]);
        }
        if ((rc = grad_sep_try(tile, g, d.nbands, qmul, fv, fg, out_dev, st)) != kDeclined) return rc;
    }
    if (d.nbands == 0) {
        // no band contributes: 0 (/ out_div) * out_scale in all four channels, evaluated on the device
        d.nbands = 1;
        d.band_scale[0] = 1.0f;
        d.band_w[0] = 0.0f;
    }
    d.out = out_dev;
    d.vol = total;
    d.n = tile->n;
    d.nmask = pow2_mask(tile->n);
    d.g = g;
    launch_grad_direct(d, tile, st);
    WN_LAUNCH_CHECK("grad3d_grid_direct_kernel(multiband)");
    return WN_OK;
}

} // extern "C"
