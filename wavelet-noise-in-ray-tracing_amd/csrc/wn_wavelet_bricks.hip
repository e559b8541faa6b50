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
//                                    y, then x (the value contraction wn_brick.hpp states, from wn::tap3), and the band sum is
//                                    one FMA per band.  Nothing is summed across samples: a sample's bits depend on its own
//                                    lattice index, the lattice, the tile and the bands only.  A wave's 64 float4 stores are
//                                    1 KiB contiguous.
//
// Both kernels read a brick's triple with the same address in every lane of a wave and decide in-range per brick, wave-uniformly;
// an out-of-range brick's slot is not touched.
//
// The in-range decision, a sample's coordinate, a box's geometry and the separable kernel's arguments, regime and frame are
// wn_brick_list.hpp's, shared with the gradient and curl bricks of wn_wavelet_brick_fields.hip.
#include "wn_brick_list.hpp"
#include "wnoise_bricks.h"

namespace {

using wn::BrickRange;
using wn::BrickSepArgs;
using wn::GridArgs;
using wn::box_geometry;
using wn::brick_coord;
using wn::brick_in_range;

constexpr int kEdge = WN_BRICK, kSamples = kEdge * kEdge * kEdge;
static_assert(kEdge == wn::kBrickEdge && kSamples == wn::kBrickSamples, "wn_brick_list.hpp's brick");

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

template <int NB>
__global__ __launch_bounds__(256) void bricks_sep_kernel(const BrickSepArgs a)
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
        int bx, by, bz;
        bool live = wn::pair_brick(a, i, bx, by, bz);
        __syncthreads(); // the previous pair's reads are done: the boxes may be overwritten
        if (live) {
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                int geo[6];
                box_geometry(g, den, a.inv_den, bx, by, bz, a.band[b].qmul, geo);
                if (!wn::brick_box_fits(geo, a.band[b].box_cap)) { // never: the planner bounds the box from the same coordinates
                    live = false;
                    break;
                }
                wn::fill_box(box[half][b], a, geo, 0, 0, 0, l);
            }
        }
        __syncthreads();
        if (!live) continue;

        // ---- this lane's 4 samples: z, then y, then x in each band's 4-column window; bands one after the other
        float px[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) px[q] = brick_coord(g, den, a.inv_den, kEdge * bx + x_in + q);
        const float py = brick_coord(g, den, a.inv_den, kEdge * by + y_in), pz = brick_coord(g, den, a.inv_den, kEdge * bz + z_in);
        float acc[1][4] = {};
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
                    zw[fy] = wn::tap3(wz, c0, c1, c2);
                }
                A[c] = wn::tap3(wy, zw[0], zw[1], zw[2]);
            }
            const float fv = a.band[b].fv;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float v = 0.0f;
#pragma unroll
                for (int c = 0; c < 4; ++c) v = __builtin_fmaf(xw.w[q][c], A[c], v);
                acc[0][q] = __builtin_fmaf(fv, v, acc[0][q]);
            }
        }
        wn::store_slots(a.out + i * kSamples + 4 * l, kSamples, a.vec4_ok, acc);
    }
}

// Launches the separable kernel when the lattice, rounded up to whole bricks (plan.gr), is in the regime of
// wn::brick_sep_args (wn_brick_list.hpp).
int sep_try(const wn_tile *tile, const wn::BrickListPlan &plan, const wn::BandFactors &f, const int32_t *bricks, size_t n,
            float *out_dev, hipStream_t stream)
{
    BrickSepArgs a{};
    if (!wn::brick_sep_args(tile, plan, nullptr, 1, kBoxCap, f, bricks, n, out_dev, &a)) return wn::kDeclined;
    const size_t pairs = (n + 1) / 2;
    wn::brick_dispatch(f.nbands, [&](auto nb) {
        hipLaunchKernelGGL(bricks_sep_kernel<decltype(nb)::value>, dim3(wn::stride_blocks(pairs * 256, kSepBlockCap)), dim3(256),
                           0, stream, a);
        return WN_OK;
    });
    WN_LAUNCH_CHECK("bricks_sep_kernel");
    return WN_OK;
}

// The entry points after their tile (and band) checks; d carries the bands of a multiband call (mb).
int bricks_call(const wn_tile *tile, const wn_grid *grid, BricksExactArgs d, bool mb, const int32_t *bricks_dev, size_t n,
                float *out_dev, hipStream_t stream)
{
    wn::BrickListPlan plan;
    bool launch;
    int rc = wn::brick_list_plan(grid, bricks_dev, n, 1, out_dev, &plan, &launch);
    if (!launch) return rc;
    const GridArgs &g = plan.g;
    const BrickRange &range = plan.range;

    if (!(grid->flags & WN_GRID_EXACT) && plan.roundable && (!mb || d.nbands >= 1)) {
        const wn::BandFactors f = wn::band_factors(d, mb, g.out_scale);
        if ((rc = sep_try(tile, plan, f, bricks_dev, n, out_dev, stream)) != wn::kDeclined) return rc;
    }
    if (mb) d.zero_band_if_none();
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
