// wn_wavelet_bounded_bricks.hip -- curl brick lists of the 3-D wavelet volume with solid boundaries
// (include/wnoise_bounded_bricks.h): the lattices and lists of wn_eval3d_curl_bricks / wn_multiband3d_curl_bricks
// (wn_wavelet_brick_fields.hip) with the obstacles of include/wnoise_bounded.h, v = A curl Psi + grad A x Psi; three slot
// arrays, out[(ch n + i) 512 + lx + 8 (ly + 8 lz)].
//
//   bounded_bricks_exact_kernel<PADDED, MB>  WN_GRID_EXACT and every lattice the separable kernel declines: the shape of
//                                    brick_fields_exact_kernel<.., CURL = true> -- one sample per lane, a brick's 512 samples in
//                                    consecutive lanes, grid-stride -- around wn::eval3d_curl_bounded_exact /
//                                    multiband_curl_bounded_exact: the bits of the bounded point lists.  No LDS.
//   curl_bounded_bricks_sep_kernel<NB>       the default tier: the frame of curl_bricks_sep_kernel around the same curl
//                                    contraction (wn_brick.hpp), line for line, so a far sample has that kernel's bits.  The
//                                    y-z contraction A0 of psi0 beside A1 and A2, and three more x contractions, give the
//                                    potential values of grad A x Psi with the bits of grad_bricks_sep_kernel's channel 0 on
//                                    the tile rolled by the potential's offset; the boxes are walked once.
//
// The obstacle list travels by value in the launch arguments (wn_obstacles.hpp): the same for every lane, read with scalar
// loads.  A lane of the separable kernel classifies its 4 samples with wn::obstacle_ramp before the band loop, and a wave
// skips by ballot what none of its 256 samples needs: the band loop when all are inside, the value sums and the combination
// when none is near.  A brick whose 512 samples are all inside also skips its box fill: its two waves say so in kFlagBytes of
// LDS before the pair's first barrier and read both flags after it (the next pair's write follows the second barrier).
// Every lane reaches both barriers of every pair, whatever its brick's class; skipping never changes a written bit.
#include "wn_brick_list.hpp"
#include "wn_obstacles.hpp"
#include "wnoise_bounded_bricks.h"

namespace {

using wn::BrickRange;
using wn::CurlEval;
using wn::GridArgs;
using wn::Obstacles;
using wn::box_geometry;
using wn::brick_coord;
using wn::brick_in_range;
using wn::fill_box;
using wn::pair_brick;
using wn::store_slots;

constexpr int kEdge = wn::kBrickEdge, kSamples = wn::kBrickSamples;

// ---- exact tier --------------------------------------------------------------------------------------------------------------
constexpr size_t kBoundedExactBlockCap = 256u * 8u; // workgroups: the cap of curl3d_bounded_points_kernel, whose body it runs

struct BoundedExactArgs {
    CurlEval e; // the tile (its padded copy when it has one), the bands, the offsets
    Obstacles o;
    GridArgs g; // z0 == 0: the kernel passes absolute z indices
    float inv_den;
    BrickRange range;
    const int32_t *bricks;
    size_t count; // bricks
    float *out;
};

template <bool PADDED, bool MB>
__global__ __launch_bounds__(256) void bounded_bricks_exact_kernel(const BoundedExactArgs a)
{
    const GridArgs &g = a.g;
    const float den = (float)g.den;
    const size_t total = a.count * kSamples; // one component's array
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        // the brick is the same in every lane of a wave: its index is made uniform first, as brick_fields_exact_kernel does
        const size_t iv = e / kSamples;
        const size_t i = ((size_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(iv >> 32)) << 32) |
                         (unsigned)__builtin_amdgcn_readfirstlane((int)iv);
        const int l = (int)(e % kSamples);
        const int bx = a.bricks[3 * i], by = a.bricks[3 * i + 1], bz = a.bricks[3 * i + 2];
        if (!brick_in_range(a.range, bx, by, bz)) continue;
        const float p[3] = {brick_coord(g, den, a.inv_den, kEdge * bx + (l & 7)),
                            brick_coord(g, den, a.inv_den, kEdge * by + ((l >> 3) & 7)),
                            brick_coord(g, den, a.inv_den, kEdge * bz + (l >> 6))};
        float v[3];
        if (MB) wn::multiband_curl_bounded_exact<PADDED>(a.e, a.o.list, a.o.nobs, p, v);
        else wn::eval3d_curl_bounded_exact<PADDED>(a.e.coef, a.e.n, a.e.nmask, a.e.off, a.o.list, a.o.nobs, p, v);
        a.out[e] = v[0] * g.out_scale;
        a.out[e + total] = v[1] * g.out_scale;
        a.out[e + 2 * total] = v[2] * g.out_scale;
    }
}

// ---- default tier: the separable kernel -----------------------------------------------------------------------------------------
constexpr int kBoxCap = 7 * 6 * 6;                 // floats per box, as wn_wavelet_bricks.hip derives it
constexpr int kFlagBytes = 4 * 4;                   // one int per wave: does the wave hold a sample that is not inside
constexpr size_t kBoundedSepBlockCap = 256u * 8u;   // workgroups of the pair-stride launch, as curl_bricks_sep_kernel's

struct BoundedSepArgs : wn::BrickSepArgs {
    Obstacles o;
};

template <int NB>
__global__ __launch_bounds__(256) void curl_bounded_bricks_sep_kernel(const BoundedSepArgs a)
{
    __shared__ float box[2][NB][3][kBoxCap]; // [brick of the pair][band][potential]
    __shared__ int open_wave[kFlagBytes / 4]; // [wave]: some sample of the wave is not inside
    const GridArgs &g = a.g;
    const float den = (float)g.den;
    const int tid = threadIdx.x;
    const int half = __builtin_amdgcn_readfirstlane(tid >> 7);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l = tid & 127;
    const int x_in = (l & 1) * 4, y_in = (l >> 1) & 7, z_in = l >> 4;
    const size_t pairs = (a.count + 1) / 2;

    for (size_t pair = blockIdx.x; pair < pairs; pair += gridDim.x) {
        const size_t i = 2 * pair + half;
        int bx, by, bz;
        bool live = pair_brick(a, i, bx, by, bz);

        // ---- this lane's 4 samples and their classes (a dead half: coordinates of brick (0, 0, 0), classes unused):
        float px[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) px[q] = brick_coord(g, den, a.inv_den, kEdge * bx + x_in + q);
        const float py = brick_coord(g, den, a.inv_den, kEdge * by + y_in), pz = brick_coord(g, den, a.inv_den, kEdge * bz + z_in);
        // two bits per sample; A and G are formed again after the band loop, by the same function and so with the same bits,
        // instead of living through it in 16 registers
        int where = 0;
        bool lane_near = false;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float p[3] = {px[q], py, pz};
            float ramp, G[3];
            const int w = wn::obstacle_ramp(a.o.list, a.o.nobs, p, ramp, G);
            where |= w << (2 * q);
            lane_near = lane_near || w == wn::kBoundNear;
        }
        const bool lane_open = where != (wn::kBoundInside * 0x55);
        // wave-uniform by ballot: `live` is the same in the wave's 64 lanes, which all serve one brick
        const bool wave_open = live && __ballot(lane_open) != 0;
        const bool wave_near = live && __ballot(lane_near) != 0;
        if ((tid & 63) == 0) open_wave[wave] = wave_open;
        __syncthreads(); // the previous pair's reads are done: the boxes may be overwritten; this pair's flags are written
        // the same in all 128 lanes of the half, from the samples' own classes: a brick that is wholly inside reads no box
        const bool fill = open_wave[2 * half] != 0 || open_wave[2 * half + 1] != 0;
        if (fill) {
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
        __syncthreads(); // the boxes are filled; the flags have been read
        if (!live) continue;

        float acc[3][4]; // [component][sample]
        if (!wave_open) {
            const float zero = 0.0f * g.out_scale;
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[k][q] = zero;
            store_slots(a.out + i * kSamples + 4 * l, a.count * kSamples, a.vec4_ok, acc);
            continue;
        }

        // ---- the curl contraction (wn_brick.hpp) per band, bands one after the other; with a near sample in the wave, the
        // potential values beside it
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[k][q] = 0.0f;
        float psi[3][4] = {}; // [potential][sample]
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
            float A0[4] = {}; // psi0's A beside A1 and A2 with a near sample in the wave: the three values
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
                if (wave_near) A0[c] = wn::tap3(wy, zw[0][0], zw[0][1], zw[0][2]);
                // one column's 27 LDS reads in flight, not all 108, as in curl_bricks_sep_kernel
                __builtin_amdgcn_sched_barrier(0);
            }
            const float fg = a.band[b].fg;
#pragma unroll
            for (int q = 0; q < 4; ++q) wn::curl_x(xw.w[q], xw.d[q], cols, fg, acc, q);
            if (wave_near) {
                // grad_bricks_sep_kernel's channel 0 on the three boxes: the value sum over the window, folded with fv
                const float fv = a.band[b].fv;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float v0 = 0.0f, v1 = 0.0f, v2 = 0.0f;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        v0 = __builtin_fmaf(xw.w[q][c], A0[c], v0);
                        v1 = __builtin_fmaf(xw.w[q][c], cols.A1[c], v1);
                        v2 = __builtin_fmaf(xw.w[q][c], cols.A2[c], v2);
                    }
                    psi[0][q] = __builtin_fmaf(fv, v0, psi[0][q]);
                    psi[1][q] = __builtin_fmaf(fv, v1, psi[1][q]);
                    psi[2][q] = __builtin_fmaf(fv, v2, psi[2][q]);
                }
            }
        }
        // ---- v = A c + G x Psi at the near samples, c at the far ones, 0 * out_scale inside: each operation rounded on its own
        const float zero = 0.0f * g.out_scale;
        if (wave_near) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float p[3] = {px[q], py, pz};
                float ramp, G[3];
                const bool near = wn::obstacle_ramp(a.o.list, a.o.nobs, p, ramp, G) == wn::kBoundNear;
                float v[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const int ka = (k + 1) % 3, kb = (k + 2) % 3;
                    const float t1 = G[ka] * psi[kb][q], t2 = G[kb] * psi[ka][q];
                    const float x = t1 - t2;
                    const float t = ramp * acc[k][q];
                    v[k] = t + x;
                }
#pragma unroll
                for (int k = 0; k < 3; ++k) acc[k][q] = near ? v[k] : acc[k][q];
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int k = 0; k < 3; ++k) acc[k][q] = ((where >> (2 * q)) & 3) == wn::kBoundInside ? zero : acc[k][q];
        store_slots(a.out + i * kSamples + 4 * l, a.count * kSamples, a.vec4_ok, acc);
    }
}

// Launches the separable kernel when the lattice is in the regime of wn::brick_sep_args (wn_brick_list.hpp): exactly the
// unbounded curl bricks' regime.
int sep_try(const wn_tile *tile, const wn::BrickListPlan &plan, const CurlEval &e, const Obstacles &o, const wn::BandFactors &f,
            const int32_t *bricks, size_t n, float *out_dev, hipStream_t stream)
{
    BoundedSepArgs a{};
    if (!wn::brick_sep_args(tile, plan, e.off, 3, kBoxCap, f, bricks, n, out_dev, &a)) return wn::kDeclined;
    a.o = o;
    const dim3 blocks(wn::stride_blocks((n + 1) / 2 * 256, kBoundedSepBlockCap)), block(256);
    wn::brick_dispatch(f.nbands, [&](auto nb) {
        hipLaunchKernelGGL(curl_bounded_bricks_sep_kernel<decltype(nb)::value>, blocks, block, 0, stream, a);
        return WN_OK;
    });
    WN_LAUNCH_CHECK("curl_bounded_bricks_sep_kernel");
    return WN_OK;
}

// The entry points after their tile, offset, band and obstacle checks, with at least one obstacle.
int bounded_bricks_call(const wn_tile *tile, const wn_grid *grid, const CurlEval &e, const Obstacles &o, const int32_t *bricks_dev,
                        size_t n, float *out_dev, hipStream_t stream)
{
    wn::BrickListPlan plan;
    bool launch;
    int rc = wn::brick_list_plan(grid, bricks_dev, n, 3, out_dev, &plan, &launch);
    if (!launch) return rc;
    const GridArgs &g = plan.g;

    if (!(grid->flags & WN_GRID_EXACT) && (!e.mb || e.nbands >= 1)) {
        // the value factor of the gradient bricks and the derivative factor of the curl bricks (wn_wavelet_brick_fields.hip)
        const wn::BandFactors f = wn::band_factors(e, e.mb, g.out_scale);
        if ((rc = sep_try(tile, plan, e, o, f, bricks_dev, n, out_dev, stream)) != wn::kDeclined) return rc;
    }
    const BoundedExactArgs d{e, o, g, wn::inv_den_of(g.den), plan.range, bricks_dev, n, out_dev};
    const dim3 blocks(wn::stride_blocks(d.count * kSamples, kBoundedExactBlockCap)), block(256);
    wn::with_curl_form(tile, d.e, [&](auto padded, auto mb) {
        hipLaunchKernelGGL((bounded_bricks_exact_kernel<decltype(padded)::value, decltype(mb)::value>), blocks, block, 0, stream, d);
    });
    WN_LAUNCH_CHECK("bounded_bricks_exact_kernel");
    return WN_OK;
}

} // namespace

using namespace wn;

extern "C" {

int wn_eval3d_curl_bounded_bricks(const wn_tile *tile, const wn_grid *grid, const int32_t *bricks_dev, size_t n,
                                  const int32_t *offsets9_host, const wn_obstacle *obstacles_host, int nobs, float *out_dev,
                                  void *stream)
{
    WN_ENTRY();
    CurlEval e;
    Obstacles o;
    int rc = curl_eval_args(tile, offsets9_host, "wn_eval3d_curl_bounded_bricks", &e);
    if (rc) return rc;
    rc = obstacle_args(obstacles_host, nobs, "wn_eval3d_curl_bounded_bricks", &o);
    if (rc) return rc;
    // no obstacle: the unbounded call, its kernels and its bits
    if (nobs == 0) return wn_eval3d_curl_bricks(tile, grid, bricks_dev, n, offsets9_host, out_dev, stream);
    return bounded_bricks_call(tile, grid, e, o, bricks_dev, n, out_dev, as_stream(stream));
}

int wn_multiband3d_curl_bounded_bricks(const wn_tile *tile, const wn_grid *grid, const int32_t *bricks_dev, size_t n,
                                       const int32_t *offsets9_host, float s, int first_band, int nbands, const float *w_host,
                                       float var_per_band, const wn_obstacle *obstacles_host, int nobs, float *out_dev,
                                       void *stream)
{
    WN_ENTRY();
    CurlEval e;
    Obstacles o;
    int rc = curl_eval_args(tile, offsets9_host, "wn_multiband3d_curl_bounded_bricks", &e);
    if (rc) return rc;
    rc = multiband_bands(s, first_band, nbands, w_host, var_per_band, &e);
    if (rc) return rc;
    rc = obstacle_args(obstacles_host, nobs, "wn_multiband3d_curl_bounded_bricks", &o);
    if (rc) return rc;
    if (nobs == 0)
        return wn_multiband3d_curl_bricks(tile, grid, bricks_dev, n, offsets9_host, s, first_band, nbands, w_host, var_per_band,
                                          out_dev, stream);
    e.mb = 1;
    return bounded_bricks_call(tile, grid, e, o, bricks_dev, n, out_dev, as_stream(stream));
}

} // extern "C"
