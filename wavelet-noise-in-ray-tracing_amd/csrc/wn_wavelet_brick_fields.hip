// wn_wavelet_brick_fields.hip -- gradient and curl brick lists of the 3-D wavelet volume (include/wnoise_brick_fields.h): the
// lattices of wn_eval3d_grad_grid / wn_eval3d_curl_grid and their multiband forms on a device list of 8 x 8 x 8 leaves, CH
// consecutive slot arrays, out[(ch n + i) 512 + lx + 8 (ly + 8 lz)]; CH = 4 {value, d/dx, d/dy, d/dz} or 3 {vx, vy, vz}.
//
//   brick_fields_exact_kernel<PADDED, MB, CURL>  WN_GRID_EXACT and every lattice the separable kernels decline: the shape of
//                                    bricks_exact_kernel (wn_wavelet_bricks.hip) -- one sample per lane, a brick's 512 samples in
//                                    consecutive lanes, grid-stride -- around wn::eval3d_grad_exact / multiband_exact<.., true>
//                                    or wn::eval3d_curl_exact / multiband_curl_exact: the bits of the point lists and of the
//                                    exact dense derivative grids.
//   grad_bricks_sep_kernel<NB>       the default tier: the frame of bricks_sep_kernel (256 lanes, two bricks per workgroup, 128
//   curl_bricks_sep_kernel<NB>       lanes per brick, a lane owns 4 consecutive x samples, per brick and band a box of at most
//                                    7 x 6 x 6 coefficients in static LDS; the curl keeps three, one per potential, each filled
//                                    from the tile shifted by its offset) around the column contractions of wn_brick.hpp,
//                                    which grad3d_grid_sep_kernel (wn_wavelet_grad.hip), curl3d_grid_sep_kernel
//                                    (wn_wavelet_curl.hip) and bricks_sep_kernel call too (the gradient's column step is
//                                    written out in both gradient kernels, line for line).  A sample therefore has the bits of
//                                    the dense default-tier grid wherever that runs its separable kernel (both windows start at
//                                    multiples of 4), and the gradient's channel 0 has the bits of bricks_sep_kernel.  One
//                                    float4 per channel and lane: a wave writes 1 KiB contiguous per channel.
//
// All kernels read a brick's triple with the same address in every lane of a wave and decide in-range per brick,
// wave-uniformly; an out-of-range brick's slots are not touched in any channel.
#include "wn_brick_list.hpp"
#include "wnoise_brick_fields.h"

#include <algorithm>

namespace {

using wn::BrickRange;
using wn::CurlEval;
using wn::BrickSepArgs;
using wn::GridArgs;
using wn::box_geometry;
using wn::brick_coord;
using wn::brick_in_range;
using wn::fill_box;
using wn::pair_brick;
using wn::store_slots;

constexpr int kEdge = wn::kBrickEdge, kSamples = wn::kBrickSamples;

// ---- exact tier --------------------------------------------------------------------------------------------------------------
struct FieldsExactArgs {
    CurlEval e; // the tile (its padded copy when it has one), the bands, and the curl's offsets
    GridArgs g; // z0 == 0: the kernels pass absolute z indices
    float inv_den;
    BrickRange range;
    const int32_t *bricks;
    size_t count; // bricks
    float *out;
};

template <bool PADDED, bool MB, bool CURL>
__global__ __launch_bounds__(256) void brick_fields_exact_kernel(const FieldsExactArgs a)
{
    const GridArgs &g = a.g;
    const float den = (float)g.den;
    const size_t total = a.count * kSamples; // one channel array
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        // the brick is the same in every lane of a wave (512 is a multiple of 64): its index is made uniform first, so that the
        // triple comes through the scalar cache and leaves the vector memory path to the evaluator's gathers
        const size_t iv = e / kSamples;
        const size_t i = ((size_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(iv >> 32)) << 32) |
                         (unsigned)__builtin_amdgcn_readfirstlane((int)iv);
        const int l = (int)(e % kSamples);
        const int bx = a.bricks[3 * i], by = a.bricks[3 * i + 1], bz = a.bricks[3 * i + 2];
        if (!brick_in_range(a.range, bx, by, bz)) continue;
        const float p[3] = {brick_coord(g, den, a.inv_den, kEdge * bx + (l & 7)),
                            brick_coord(g, den, a.inv_den, kEdge * by + ((l >> 3) & 7)),
                            brick_coord(g, den, a.inv_den, kEdge * bz + (l >> 6))};
        if (CURL) {
            float v[3];
            if (MB) wn::multiband_curl_exact<PADDED>(a.e, p, v);
            else wn::eval3d_curl_exact<PADDED>(a.e.coef, a.e.n, a.e.nmask, a.e.off, p[0], p[1], p[2], v);
            a.out[e] = v[0] * g.out_scale;
            a.out[e + total] = v[1] * g.out_scale;
            a.out[e + 2 * total] = v[2] * g.out_scale;
        } else {
            float gr[3];
            const float v = MB ? wn::multiband_exact<PADDED, false, true>(a.e, p, nullptr, gr)
                               : wn::eval3d_grad_exact<PADDED>(a.e.coef, a.e.n, a.e.nmask, p[0], p[1], p[2], gr);
            a.out[e] = v * g.out_scale;
            a.out[e + total] = gr[0] * g.out_scale;
            a.out[e + 2 * total] = gr[1] * g.out_scale;
            a.out[e + 3 * total] = gr[2] * g.out_scale;
        }
    }
}

// ---- default tier: the separable kernels ----------------------------------------------------------------------------------------
constexpr int kBoxCap = 7 * 6 * 6;              // floats per box, as wn_wavelet_bricks.hip derives it
constexpr size_t kSepBlockCap = 256u * 8u;       // workgroups of the pair-stride launches
constexpr size_t kCurlExactBlockCap = 256u * 8u; // of the exact curl launch: the cap of curl3d_points_kernel, whose body it runs

template <int NB>
__global__ __launch_bounds__(256) void grad_bricks_sep_kernel(const BrickSepArgs a)
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
        bool live = pair_brick(a, i, bx, by, bz);
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
                fill_box(box[half][b], a, geo, 0, 0, 0, l);
            }
        }
        __syncthreads();
        if (!live) continue;

        // ---- this lane's 4 samples: the gradient contraction (wn_brick.hpp; its column step exactly as
        // grad3d_grid_sep_kernel writes it) per band, bands one after the other
        float px[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) px[q] = brick_coord(g, den, a.inv_den, kEdge * bx + x_in + q);
        const float py = brick_coord(g, den, a.inv_den, kEdge * by + y_in), pz = brick_coord(g, den, a.inv_den, kEdge * bz + z_in);
        float acc[4][4] = {}; // [channel][sample]
#pragma unroll 1
        for (int b = 0; b < NB; ++b) {
            const float qm = a.band[b].qmul;
            int geo[6];
            box_geometry(g, den, a.inv_den, bx, by, bz, qm, geo);
            wn::XWin xw;
            wn::brick_x_window(px, qm, geo[0], xw);
            int my, mz;
            float wy[3], dy[3], wz[3], dz[3];
            wn::bspline_grad(py * qm, my, wy, dy);
            wn::bspline_grad(pz * qm, mz, wz, dz);
            const int ex = geo[3], ey = geo[4];
            const float *base = box[half][b] + ((mz - 1 - geo[2]) * ey + (my - 1 - geo[1])) * ex + xw.col;
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
        store_slots(a.out + i * kSamples + 4 * l, a.count * kSamples, a.vec4_ok, acc);
    }
}

template <int NB>
__global__ __launch_bounds__(256) void curl_bricks_sep_kernel(const BrickSepArgs a)
{
    __shared__ float box[2][NB][3][kBoxCap]; // [brick of the pair][band][potential]: the only LDS
    const GridArgs &g = a.g;
    const float den = (float)g.den;
    const int tid = threadIdx.x;
    const int half = __builtin_amdgcn_readfirstlane(tid >> 7);
    const int l = tid & 127;
    const int x_in = (l & 1) * 4, y_in = (l >> 1) & 7, z_in = l >> 4;
    const size_t pairs = (a.count + 1) / 2;

    for (size_t pair = blockIdx.x; pair < pairs; pair += gridDim.x) {
        const size_t i = 2 * pair + half;
        int bx, by, bz;
        bool live = pair_brick(a, i, bx, by, bz);
        __syncthreads(); // the previous pair's reads are done: the boxes may be overwritten
        if (live) {
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                int geo[6]; // shared by the three potentials: whole-cell shifts leave the mids alone
                box_geometry(g, den, a.inv_den, bx, by, bz, a.band[b].qmul, geo);
                if (!wn::brick_box_fits(geo, a.band[b].box_cap)) { // never
                    live = false;
                    break;
                }
#pragma unroll 1
                for (int k3 = 0; k3 < 3; ++k3) fill_box(box[half][b][k3], a, geo, a.off[3 * k3], a.off[3 * k3 + 1], a.off[3 * k3 + 2], l);
            }
        }
        __syncthreads();
        if (!live) continue;

        // ---- this lane's 4 samples: the curl contraction (wn_brick.hpp) per band, bands one after the other
        float px[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) px[q] = brick_coord(g, den, a.inv_den, kEdge * bx + x_in + q);
        const float py = brick_coord(g, den, a.inv_den, kEdge * by + y_in), pz = brick_coord(g, den, a.inv_den, kEdge * bz + z_in);
        float acc[3][4] = {}; // [component][sample]
#pragma unroll 1
        for (int b = 0; b < NB; ++b) {
            const float qm = a.band[b].qmul;
            int geo[6];
            box_geometry(g, den, a.inv_den, bx, by, bz, qm, geo);
            wn::XWin xw;
            wn::brick_x_window(px, qm, geo[0], xw);
            int my, mz;
            float wy[3], dy[3], wz[3], dz[3];
            wn::bspline_grad(py * qm, my, wy, dy);
            wn::bspline_grad(pz * qm, mz, wz, dz);
            const int ex = geo[3], ey = geo[4];
            const float *base = box[half][b][0] + ((mz - 1 - geo[2]) * ey + (my - 1 - geo[1])) * ex + xw.col;
            // per window column (wn_brick.hpp): P = B2 - D1 (for vx), D0 and A2 (vy), A1 and B0 (vz)
            wn::CurlColumns cols;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float zw[3][3], zd[2][3]; // [potential][fy]: Z for all three, Z' for psi0 and psi1
#pragma unroll
                for (int k3 = 0; k3 < 3; ++k3)
#pragma unroll
                    for (int fy = 0; fy < 3; ++fy) {
                        const float *bk = base + k3 * kBoxCap;
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
                // one column's 27 LDS reads in flight, not all 108, as in curl3d_grid_sep_kernel (registers with and without:
                // profiles/brick_fields_kernels.txt)
                __builtin_amdgcn_sched_barrier(0);
            }
            const float fg = a.band[b].fg;
#pragma unroll
            for (int q = 0; q < 4; ++q) wn::curl_x(xw.w[q], xw.d[q], cols, fg, acc, q);
        }
        store_slots(a.out + i * kSamples + 4 * l, a.count * kSamples, a.vec4_ok, acc);
    }
}

// Launches a separable kernel when the lattice, rounded up to whole bricks (plan.gr), is in the regime of
// wn::brick_sep_args (wn_brick_list.hpp).
int sep_try(const wn_tile *tile, const wn::BrickListPlan &plan, const CurlEval &e, bool curl, const wn::BandFactors &f,
            const int32_t *bricks, size_t n, float *out_dev, hipStream_t stream)
{
    BrickSepArgs a{};
    if (!wn::brick_sep_args(tile, plan, e.off, curl ? 3 : 1, kBoxCap, f, bricks, n, out_dev, &a)) return wn::kDeclined;
    const dim3 blocks(wn::stride_blocks((n + 1) / 2 * 256, kSepBlockCap)), block(256);
    wn::brick_dispatch(f.nbands, [&](auto nb) {
        if (curl) hipLaunchKernelGGL(curl_bricks_sep_kernel<decltype(nb)::value>, blocks, block, 0, stream, a);
        else hipLaunchKernelGGL(grad_bricks_sep_kernel<decltype(nb)::value>, blocks, block, 0, stream, a);
        return WN_OK;
    });
    WN_LAUNCH_CHECK(curl ? "curl_bricks_sep_kernel" : "grad_bricks_sep_kernel");
    return WN_OK;
}

template <bool CURL>
void launch_exact(const wn_tile *tile, const FieldsExactArgs &d, hipStream_t stream)
{
    const dim3 blocks(CURL ? wn::stride_blocks(d.count * kSamples, kCurlExactBlockCap) : wn::stride_blocks(d.count * kSamples)), block(256);
    wn::with_curl_form(tile, d.e, [&](auto padded, auto mb) {
        hipLaunchKernelGGL((brick_fields_exact_kernel<decltype(padded)::value, decltype(mb)::value, CURL>), blocks, block, 0, stream, d);
    });
}

// The entry points after their tile, offsets and band checks: e carries the tile, the bands of a multiband call (e.mb) and the
// curl's offsets.
int fields_call(const wn_tile *tile, const wn_grid *grid, CurlEval e, bool curl, const int32_t *bricks_dev, size_t n,
                float *out_dev, hipStream_t stream)
{
    wn::BrickListPlan plan;
    bool launch;
    int rc = wn::brick_list_plan(grid, bricks_dev, n, curl ? 3 : 4, out_dev, &plan, &launch);
    if (!launch) return rc;
    const GridArgs &g = plan.g;

    if (!(grid->flags & WN_GRID_EXACT) && (!e.mb || e.nbands >= 1)) {
        // the bands and factors of grad_grid (wn_wavelet_grad.hip) and curl_grid (wn_wavelet_curl.hip)
        const wn::BandFactors f = wn::band_factors(e, e.mb, g.out_scale);
        if ((rc = sep_try(tile, plan, e, curl, f, bricks_dev, n, out_dev, stream)) != wn::kDeclined) return rc;
    }
    if (!curl && e.mb) e.zero_band_if_none(); // as grad_grid does
    const FieldsExactArgs d{e, g, wn::inv_den_of(g.den), plan.range, bricks_dev, n, out_dev};
    if (curl) launch_exact<true>(tile, d, stream);
    else launch_exact<false>(tile, d, stream);
    WN_LAUNCH_CHECK(curl ? "brick_fields_exact_kernel(curl)" : "brick_fields_exact_kernel(gradient)");
    return WN_OK;
}

// A gradient entry point's CurlEval: the tile's fields, no offsets.
int grad_eval_args(const wn_tile *tile, const char *entry, CurlEval *e)
{
    const int rc = wn::check_tile(tile, 3, entry);
    if (rc) return rc;
    *e = CurlEval{};
    e->coef = tile->dev_padded ? tile->dev_padded : tile->dev;
    e->n = tile->n;
    e->nmask = wn::pow2_mask(tile->n);
    return WN_OK;
}

} // namespace

using namespace wn;

extern "C" {

int wn_eval3d_grad_bricks(const wn_tile *tile, const wn_grid *grid, const int32_t *bricks_dev, size_t n, float *out_dev,
                          void *stream)
{
    WN_ENTRY();
    CurlEval e;
    const int rc = grad_eval_args(tile, "wn_eval3d_grad_bricks", &e);
    if (rc) return rc;
    return fields_call(tile, grid, e, false, bricks_dev, n, out_dev, as_stream(stream));
}

int wn_multiband3d_grad_bricks(const wn_tile *tile, const wn_grid *grid, const int32_t *bricks_dev, size_t n, float s,
                               int first_band, int nbands, const float *w_host, float var_per_band, float *out_dev, void *stream)
{
    WN_ENTRY();
    CurlEval e;
    int rc = grad_eval_args(tile, "wn_multiband3d_grad_bricks", &e);
    if (rc) return rc;
    rc = multiband_bands(s, first_band, nbands, w_host, var_per_band, &e);
    if (rc) return rc;
    e.mb = 1;
    return fields_call(tile, grid, e, false, bricks_dev, n, out_dev, as_stream(stream));
}

int wn_eval3d_curl_bricks(const wn_tile *tile, const wn_grid *grid, const int32_t *bricks_dev, size_t n,
                          const int32_t *offsets9_host, float *out_dev, void *stream)
{
    WN_ENTRY();
    CurlEval e;
    const int rc = curl_eval_args(tile, offsets9_host, "wn_eval3d_curl_bricks", &e);
    if (rc) return rc;
    return fields_call(tile, grid, e, true, bricks_dev, n, out_dev, as_stream(stream));
}

int wn_multiband3d_curl_bricks(const wn_tile *tile, const wn_grid *grid, const int32_t *bricks_dev, size_t n,
                               const int32_t *offsets9_host, float s, int first_band, int nbands, const float *w_host,
                               float var_per_band, float *out_dev, void *stream)
{
    WN_ENTRY();
    CurlEval e;
    int rc = curl_eval_args(tile, offsets9_host, "wn_multiband3d_curl_bricks", &e);
    if (rc) return rc;
    rc = multiband_bands(s, first_band, nbands, w_host, var_per_band, &e);
    if (rc) return rc;
    e.mb = 1;
    return fields_call(tile, grid, e, true, bricks_dev, n, out_dev, as_stream(stream));
}

} // extern "C"
