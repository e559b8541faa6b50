// wn_wavelet_bricks.hip -- sparse brick lists of the 3-D wavelet volume (include/wnoise_bricks.h): evaluate3D and
// WMultibandNoise (normal == NULL) on a device list of 8 x 8 x 8 leaves of the lattice a wn_grid describes, each written to
// its own 512-float slot, out[512 i + lx + 8 (ly + 8 lz)].
//
//   bricks_exact_kernel<PADDED, MB>  WN_GRID_EXACT and every lattice the separable kernel declines: one sample per lane, a
//                                    brick's 512 samples in consecutive lanes (a wave never straddles two bricks), grid-stride
//                                    over the samples of the list; wn::eval3d_exact / multiband_exact at the sample's float
//                                    coordinates: the bits of the point lists and of the exact dense grids.
//   bricks_sep_kernel<NB>            the default tier.  The frame of wn_brick.hpp at another brick geometry: 8 x 8 x 8 samples
//                                    instead of 256 x 8 x 8, so a brick occupies 128 lanes (a lane owns 4 consecutive x samples:
//                                    lane l of a brick holds its floats 4 l .. 4 l + 3) and a 256-lane workgroup works on two
//                                    bricks at a time, striding over the list in pairs.  Per brick and band one coefficient box
//                                    (periodic wrap resolved, x fastest: brick_fill's layout) of at most 7 x 6 x 6 floats -- the
//                                    6^3 cells under 8 samples at a step below 1/3 cell, and the window's fourth column -- is
//                                    staged in LDS; every lane then contracts the 4 box columns under its samples over z, then
//                                    y, then x (fused), and the band sum is one FMA per band.  Nothing is summed across samples:
//                                    a sample's bits depend on its own lattice index, the lattice, the tile and the bands only.
//                                    A wave's 64 float4 stores are 1 KiB contiguous.
//
// Both kernels read a brick's triple with the same address in every lane of a wave and decide in-range per brick, wave-uniformly;
// an out-of-range brick's slot is not touched.
#include "wn_brick.hpp"
#include "wnoise_bricks.h"

#include <climits>
#include <cstdint>

namespace {

using wn::GridArgs;
using wn::kMaxBands;

constexpr int kEdge = WN_BRICK, kSamples = kEdge * kEdge * kEdge;

// The bricks of the volume: 0 <= bx < nbx, 0 <= by < nby, bz0 <= bz < bz1.
struct BrickRange {
    int nbx, nby, bz0, bz1;
};

__device__ __forceinline__ bool brick_in_range(const BrickRange &r, int bx, int by, int bz)
{
    return bx >= 0 && bx < r.nbx && by >= 0 && by < r.nby && bz >= r.bz0 && bz < r.bz1;
}

// The coordinate of lattice index i (x, y and z alike: z indices are absolute), wn::lattice_coord's bits: the division is an
// exact multiply when den is a power of two (inv_den = wn::inv_den_of(den), else 0).
__device__ __forceinline__ float brick_coord(const GridArgs &g, float den, float inv_den, int i)
{
    return wn::lattice_coord_fast(i, den, inv_den, g.base_range, g.octave_scale, g.post_scale);
}

// ---- exact tier --------------------------------------------------------------------------------------------------------------
struct BricksExactArgs : wn::Bands {
    const float *coef; // the tile's padded copy when it has one
    int n, nmask;
    GridArgs g; // z0 == 0: the kernels pass absolute z indices
    float inv_den;
    BrickRange range;
    const int32_t *bricks;
    size_t count; // bricks
    float *out;
};

template <bool PADDED, bool MB>
__global__ __launch_bounds__(256) void bricks_exact_kernel(const BricksExactArgs a)
{
    const GridArgs &g = a.g;
    const float den = (float)g.den;
    const size_t total = a.count * kSamples;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const size_t i = e / kSamples; // the same in every lane of a wave: 512 is a multiple of 64
        const int l = (int)(e % kSamples);
        const int bx = __builtin_amdgcn_readfirstlane(a.bricks[3 * i]);
        const int by = __builtin_amdgcn_readfirstlane(a.bricks[3 * i + 1]);
        const int bz = __builtin_amdgcn_readfirstlane(a.bricks[3 * i + 2]);
        if (!brick_in_range(a.range, bx, by, bz)) continue;
        const float p[3] = {brick_coord(g, den, a.inv_den, kEdge * bx + (l & 7)),
                            brick_coord(g, den, a.inv_den, kEdge * by + ((l >> 3) & 7)),
                            brick_coord(g, den, a.inv_den, kEdge * bz + (l >> 6))};
        const float v = MB ? wn::multiband_exact<PADDED, false, false>(a, p, nullptr, nullptr)
                           : wn::eval3d_exact<PADDED>(a.coef, a.n, a.nmask, p[0], p[1], p[2]);
        a.out[e] = v * g.out_scale;
    }
}

// ---- default tier: the separable kernel -----------------------------------------------------------------------------------------
constexpr int kBoxCap = 7 * 6 * 6;        // floats per box: extent(8) <= 6 cells per axis inside two_mids, + the window's fourth column
constexpr size_t kSepBlockCap = 256u * 8u; // workgroups of the pair-stride launch: 8 per compute unit, 32 waves

struct ListBand : wn::BrickBand {
    float f; // everything that scales the band: w_b / out_div * out_scale
};

struct BricksSepArgs {
    const float *coef; // linear tile
    int n, nmask;
    GridArgs g; // z0 == 0
    float inv_den;
    BrickRange range;
    const int32_t *bricks;
    size_t count;
    float *out;
    int vec4_ok; // out is 16-byte aligned, and with it every slot
    ListBand band[kMaxBands];
};

// One axis of a band's box under the 8 samples from index `first`: coordinates are monotone in the index, so the mids of the
// first and the last sample bound all of them; one cell of support on either side.
__device__ __forceinline__ void box_axis(const GridArgs &g, float den, float inv_den, int first, float qmul, int &lo, int &ext)
{
    int m0, m1;
    float w0, w1, w2;
    wn::bspline(brick_coord(g, den, inv_den, first) * qmul, m0, w0, w1, w2);
    wn::bspline(brick_coord(g, den, inv_den, first + kEdge - 1) * qmul, m1, w0, w1, w2);
    lo = min(m0, m1) - 1;
    ext = abs(m1 - m0) + 3;
}

// geo = (ix0, jy0, kz0, ex, ey, ez) of wn::brick_fill; x carries the window's fourth column (zero weight, finite values).
__device__ __forceinline__ void box_geometry(const GridArgs &g, float den, float inv_den, int bx, int by, int bz, float qmul,
                                             int geo[6])
{
    box_axis(g, den, inv_den, kEdge * bx, qmul, geo[0], geo[3]);
    box_axis(g, den, inv_den, kEdge * by, qmul, geo[1], geo[4]);
    box_axis(g, den, inv_den, kEdge * bz, qmul, geo[2], geo[5]);
    geo[3] += 1;
}

template <int NB>
__global__ __launch_bounds__(256) void bricks_sep_kernel(const BricksSepArgs a)
{
    __shared__ float box[2][NB][kBoxCap]; // [brick of the pair][band]: the only LDS
    const GridArgs &g = a.g;
    const float den = (float)g.den;
    const int tid = threadIdx.x;
    const int half = __builtin_amdgcn_readfirstlane(tid >> 7); // waves 0, 1: the pair's first brick; 2, 3: its second
    const int l = tid & 127;                                   // the lane's floats of the slot: 4 l .. 4 l + 3
    const int x_in = (l & 1) * 4, y_in = (l >> 1) & 7, z_in = l >> 4;
    const size_t pairs = (a.count + 1) / 2;

    for (size_t pair = blockIdx.x; pair < pairs; pair += gridDim.x) {
        const size_t i = 2 * pair + half;
        int bx = 0, by = 0, bz = 0;
        bool live = i < a.count;
        if (live) {
            bx = __builtin_amdgcn_readfirstlane(a.bricks[3 * i]);
            by = __builtin_amdgcn_readfirstlane(a.bricks[3 * i + 1]);
            bz = __builtin_amdgcn_readfirstlane(a.bricks[3 * i + 2]);
            live = brick_in_range(a.range, bx, by, bz);
        }
        __syncthreads(); // the previous pair's reads are done: the boxes may be overwritten

        // ---- fill: box[k][j][i] = coef[Mod(kz0+k)][Mod(jy0+j)][Mod(ix0+i)], the brick's 128 lanes over the flat box (rows are
        // at most 7 cells: brick_fill's row per wave would leave 57 of 64 lanes idle)
        if (live) {
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                int geo[6];
                box_geometry(g, den, a.inv_den, bx, by, bz, a.band[b].qmul, geo);
                if (!wn::brick_box_fits(geo, a.band[b].box_cap)) { // never: the planner bounds the box from the same coordinates
                    live = false;
                    break;
                }
                const int ex = geo[3], exy = geo[3] * geo[4], cells = exy * geo[5];
                float *bb = box[half][b];
                for (int c = l; c < cells; c += 128) {
                    const int k = c / exy, r = c - k * exy;
                    const int j = r / ex, ii = r - j * ex;
                    bb[c] = a.coef[((size_t)wn::dmod(geo[2] + k, a.n, a.nmask) * a.n + wn::dmod(geo[1] + j, a.n, a.nmask)) * a.n +
                                   wn::dmod(geo[0] + ii, a.n, a.nmask)];
                }
            }
        }
        __syncthreads();
        if (!live) continue;

        // ---- this lane's 4 samples: z, then y, then x in each band's 4-column window; bands one after the other
        float px[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) px[q] = brick_coord(g, den, a.inv_den, kEdge * bx + x_in + q);
        const float py = brick_coord(g, den, a.inv_den, kEdge * by + y_in), pz = brick_coord(g, den, a.inv_den, kEdge * bz + z_in);
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
        for (int b = 0; b < NB; ++b) {
            const float qm = a.band[b].qmul;
            int geo[6];
            box_geometry(g, den, a.inv_den, bx, by, bz, qm, geo);
            wn::XWin xw;
            wn::brick_x_window(px, qm, geo[0], xw);
            int my, mz;
            float wy[3], wz[3];
            wn::bspline(py * qm, my, wy[0], wy[1], wy[2]);
            wn::bspline(pz * qm, mz, wz[0], wz[1], wz[2]);
            const int ex = geo[3], ey = geo[4];
            const float *base = box[half][b] + ((mz - 1 - geo[2]) * ey + (my - 1 - geo[1])) * ex + xw.col;
            float A[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float zw[3];
#pragma unroll
                for (int fy = 0; fy < 3; ++fy) {
                    const float c0 = base[(0 * ey + fy) * ex + c], c1 = base[(1 * ey + fy) * ex + c], c2 = base[(2 * ey + fy) * ex + c];
                    zw[fy] = __builtin_fmaf(wz[2], c2, __builtin_fmaf(wz[1], c1, wz[0] * c0));
                }
                A[c] = __builtin_fmaf(wy[2], zw[2], __builtin_fmaf(wy[1], zw[1], wy[0] * zw[0]));
            }
            const float f = a.band[b].f;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float v = 0.0f;
#pragma unroll
                for (int c = 0; c < 4; ++c) v = __builtin_fmaf(xw.w[q][c], A[c], v);
                acc[q] = __builtin_fmaf(f, v, acc[q]);
            }
        }
        float *dst = a.out + i * kSamples + 4 * l;
        if (a.vec4_ok) {
            *reinterpret_cast<v4f *>(dst) = v4f{acc[0], acc[1], acc[2], acc[3]};
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) dst[q] = acc[q];
        }
    }
}

// Launches the separable kernel when the lattice, rounded up to whole bricks (gr), is in its regime: a tile that is not
// empty, and in every band a step >= 0 below 1/3 cell (LatticeStep::two_mids) with coordinates inside the planners' gate;
// the box of 8 samples then has at most 6 cells per axis and always fits.
int sep_try(const wn_tile *tile, const GridArgs &g, const GridArgs &gr, const BrickRange &range, int nbands, const float *qmul,
            const float *f, const int32_t *bricks, size_t n, float *out_dev, hipStream_t stream)
{
    if (tile->n == 0 || nbands < 1 || nbands > kMaxBands) return wn::kDeclined;
    BricksSepArgs a{};
    for (int b = 0; b < nbands; ++b) {
        wn::LatticeStep ls;
        if (!wn::lattice_step(gr, g.octave_scale * qmul[b], false, false, 0.0, &ls) || !ls.two_mids()) return wn::kDeclined;
        if ((ls.extent(kEdge) + 1) * ls.extent(kEdge) * ls.extent(kEdge) > kBoxCap) return wn::kDeclined; // never inside two_mids
        a.band[b].qmul = qmul[b];
        a.band[b].box_off = b * kBoxCap;
        a.band[b].box_cap = kBoxCap;
        a.band[b].f = f[b];
    }
    a.coef = tile->dev;
    a.n = tile->n;
    a.nmask = wn::pow2_mask(tile->n);
    a.g = g;
    a.inv_den = wn::inv_den_of(g.den);
    a.range = range;
    a.bricks = bricks;
    a.count = n;
    a.out = out_dev;
    a.vec4_ok = (reinterpret_cast<uintptr_t>(out_dev) & 15) == 0;
    const size_t pairs = (n + 1) / 2;
    wn::brick_dispatch(nbands, [&](auto nb) {
        hipLaunchKernelGGL(bricks_sep_kernel<decltype(nb)::value>, dim3(wn::stride_blocks(pairs * 256, kSepBlockCap)), dim3(256),
                           0, stream, a);
        return WN_OK;
    });
    WN_LAUNCH_CHECK("bricks_sep_kernel");
    return WN_OK;
}

inline long long floor_div8(long long v) { return v >= 0 ? v / kEdge : -((-v + kEdge - 1) / kEdge); }

// The entry points after their tile (and band) checks; d carries the bands of a multiband call (mb).
int bricks_call(const wn_tile *tile, const wn_grid *grid, BricksExactArgs d, bool mb, const int32_t *bricks_dev, size_t n,
                float *out_dev, hipStream_t stream)
{
    GridArgs g;
    int rc = wn::check_grid(grid, true, &g);
    if (rc) return rc;
    if (grid->z_mode == WN_Z_CONST)
        return wn::fail(WN_ERR_INVALID, "wn_grid.z_mode must be WN_Z_LATTICE: bricks are three-dimensional");
    if (n == 0) return WN_OK;
    if (!bricks_dev) return wn::fail(WN_ERR_INVALID, "bricks_dev is NULL");
    if (!out_dev) return wn::fail(WN_ERR_INVALID, "out_dev is NULL");
    if (n > SIZE_MAX / kSamples) return wn::fail(WN_ERR_INVALID, "n * 512 overflows size_t");
    if (g.nx == 0 || g.ny == 0 || g.nz == 0) return WN_OK; // an empty volume: no brick is in range

    // the volume in bricks, and the lattice rounded up to whole bricks (what an in-range brick can reach) for the regime
    const long long bz0 = floor_div8(g.z0), bz1 = -floor_div8(-((long long)g.z0 + g.nz));
    const BrickRange range{(int)(((long long)g.nx + kEdge - 1) / kEdge), (int)(((long long)g.ny + kEdge - 1) / kEdge), (int)bz0,
                           (int)bz1};
    const long long rx = (long long)range.nbx * kEdge, ry = (long long)range.nby * kEdge;
    const bool roundable = rx <= INT_MAX && ry <= INT_MAX && bz0 * kEdge >= INT_MIN && bz1 * kEdge <= INT_MAX;
    g.z0 = 0; // the kernels form z coordinates from absolute indices
    g.nz = 0;

    if (!(grid->flags & WN_GRID_EXACT) && roundable && (!mb || d.nbands >= 1)) {
        GridArgs gr = g;
        gr.nx = (int)rx;
        gr.ny = (int)ry;
        gr.z0 = (int)(bz0 * kEdge);
        gr.nz = (int)((bz1 - bz0) * kEdge);
        // band b: q = p * (2 * 2^(first_band+b)), factor w_b / out_div * out_scale
        float qmul[kMaxBands] = {1.0f}, f[kMaxBands] = {g.out_scale};
        for (int b = 0; mb && b < d.nbands; ++b) {
            qmul[b] = 2.0f * d.band_scale[b];
            f[b] = (float)((double)d.band_w[b] / (double)d.out_div * (double)g.out_scale);
        }
        if ((rc = sep_try(tile, g, gr, range, mb ? d.nbands : 1, qmul, f, bricks_dev, n, out_dev, stream)) != wn::kDeclined)
            return rc;
    }
    if (mb && d.nbands == 0) {
        // no band contributes: 0 (/ out_div) * out_scale, evaluated on the device
        d.nbands = 1;
        d.band_scale[0] = 1.0f;
        d.band_w[0] = 0.0f;
    }
    d.coef = tile->dev_padded ? tile->dev_padded : tile->dev;
    d.n = tile->n;
    d.nmask = wn::pow2_mask(tile->n);
    d.g = g;
    d.inv_den = wn::inv_den_of(g.den);
    d.range = range;
    d.bricks = bricks_dev;
    d.count = n;
    d.out = out_dev;
    const bool padded = tile->dev_padded != nullptr;
    if (mb) {
        if (padded) hipLaunchKernelGGL((bricks_exact_kernel<true, true>), dim3(wn::stride_blocks(n * kSamples)), dim3(256), 0, stream, d);
        else hipLaunchKernelGGL((bricks_exact_kernel<false, true>), dim3(wn::stride_blocks(n * kSamples)), dim3(256), 0, stream, d);
    } else {
        if (padded) hipLaunchKernelGGL((bricks_exact_kernel<true, false>), dim3(wn::stride_blocks(n * kSamples)), dim3(256), 0, stream, d);
        else hipLaunchKernelGGL((bricks_exact_kernel<false, false>), dim3(wn::stride_blocks(n * kSamples)), dim3(256), 0, stream, d);
    }
    WN_LAUNCH_CHECK(mb ? "bricks_exact_kernel(multiband)" : "bricks_exact_kernel");
    return WN_OK;
}

} // namespace

using namespace wn;

extern "C" {

int wn_eval3d_bricks(const wn_tile *tile, const wn_grid *grid, const int32_t *bricks_dev, size_t n, float *out_dev, void *stream)
{
    WN_ENTRY();
    const int rc = check_tile(tile, 3, "wn_eval3d_bricks");
    if (rc) return rc;
    return bricks_call(tile, grid, BricksExactArgs{}, false, bricks_dev, n, out_dev, as_stream(stream));
}

int wn_multiband3d_bricks(const wn_tile *tile, const wn_grid *grid, const int32_t *bricks_dev, size_t n, float s, int first_band,
                          int nbands, const float *w_host, float var_per_band, float *out_dev, void *stream)
{
    WN_ENTRY();
    int rc = check_tile(tile, 3, "wn_multiband3d_bricks");
    if (rc) return rc;
    BricksExactArgs d{};
    rc = multiband_bands(s, first_band, nbands, w_host, var_per_band, &d);
    if (rc) return rc;
    return bricks_call(tile, grid, d, true, bricks_dev, n, out_dev, as_stream(stream));
}

} // extern "C"
