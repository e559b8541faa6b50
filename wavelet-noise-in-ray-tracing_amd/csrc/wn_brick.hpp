// wn_brick.hpp -- the frame of the separable brick kernels of the derivative grids: grad3d_grid_sep_kernel<NB>
// (wn_wavelet_grad.hip) and curl3d_grid_sep_kernel<NB> (wn_wavelet_curl.hip).
//
// A workgroup (4 waves) owns a brick of 256 x 8 x 8 samples.  For every band it stages `boxes` coefficient boxes (gradient 1;
// curl 3, one per potential, of one geometry) in LDS once, periodic wrap resolved, x fastest.  A lane owns 4 consecutive x
// samples, a wave rows (y, z) of the brick; 4 consecutive samples span at most two mids, so their taps lie in the 4 box
// columns m0 - 1 .. m0 + 2, and each sample's x weights are placed in that window (zero outside its three taps).  The
// arithmetic between staging and store -- the value, gradient and curl contractions of those columns over z, then y, then
// x -- is stated here once, for these two kernels and for the brick-list kernels of wn_brick_list.hpp, which promise the
// dense grids' bits; so are the bands' factors (wn::band_factors).  A sample's bits depend on its own weights and
// coefficients only, not on its place in a brick or z-slab.
//
// The geometry step (first and last mids per band and axis -> s_geo) stays written out in both kernels: as a forceinline
// helper (storing to s_geo itself, or returning the first cell and the extent) it takes grad3d_grid_sep_kernel<1> from 80
// to 87 VGPRs, 6 waves per SIMD to 5.
#pragma once

#include "wn_internal.hpp"

#include <type_traits>

namespace wn {

constexpr int kGX = 256, kGY = 8, kGZ = 8; // samples per brick
constexpr int kGWaves = 4;

// What the planner places per band; the kernels' band structs begin with it.
struct BrickBand {
    float qmul;  // the band's coordinate is q = p * qmul (1; multiband 2 * 2^(first_band+b): exact)
    int box_off; // float offset of its first box in dynamic LDS; box k at box_off + k * box_cap
    int box_cap; // floats reserved for each of its boxes
};

// Plans a brick launch into *a (coef, out, vol, n, nmask, g, vec4_ok and every band's BrickBand) when the lattice is in the
// regime: a tile that is not empty (any size: the boxes are filled modulo n), steps >= 0 at which 4 consecutive samples
// span at most two mids in every band (LatticeStep::two_mids: step < 1/3 cell), at most max_floats of LDS for all boxes
// and a grid within the launch limits.  Nothing in it depends on how many planes the call computes beyond lattice_step's
// bound on the coordinates.  nbands bands (1..kMaxBands) with coordinate multipliers qmul[b].
template <typename Args>
bool brick_plan(const wn_tile *tile, const GridArgs &g, int nbands, const float *qmul, int boxes, long long max_floats,
                float *out_dev, Args *a, dim3 *grid, size_t *lds)
{
    if (tile->n == 0 || nbands < 1 || nbands > kMaxBands || g.nx <= 0 || g.ny <= 0 || g.nz <= 0) return false;
    long long box_total = 0;
    for (int b = 0; b < nbands; ++b) {
        LatticeStep ls;
        if (!lattice_step(g, g.octave_scale * qmul[b], true, false, 0.0, &ls) || !ls.two_mids()) return false;
        const long long ex = ls.extent(kGX) + 1, ey = ls.extent(kGY), ez = g.z_const_mode ? 3 : ls.extent(kGZ);
        a->band[b].qmul = qmul[b];
        a->band[b].box_off = (int)box_total;
        a->band[b].box_cap = (int)(ex * ey * ez);
        box_total += boxes * ex * ey * ez;
        if (box_total > max_floats) return false;
    }
    const int nbx = (g.nx + kGX - 1) / kGX, nby = (g.ny + kGY - 1) / kGY, nbz = (g.nz + kGZ - 1) / kGZ;
    if (nby > 65535 || nbz > 65535) return false;
    a->coef = tile->dev;
    a->out = out_dev;
    a->vol = (size_t)g.nx * g.ny * g.nz;
    a->n = tile->n;
    a->nmask = pow2_mask(tile->n);
    a->g = g;
    a->vec4_ok = vec4_ok(out_dev, g.nx);
    *grid = dim3(nbx, nby, nbz);
    *lds = (size_t)box_total * sizeof(float);
    return true;
}

// f(std::integral_constant<int, nbands>) for nbands in 1..kMaxBands: the kernels are templates of their band count.
template <typename F>
int brick_dispatch(int nbands, F &&f)
{
    switch (nbands) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    case 6: return f(std::integral_constant<int, 6>{});
    case 7: return f(std::integral_constant<int, 7>{});
    default: return f(std::integral_constant<int, 8>{});
    }
}

// The bands of a separable launch and their factors.  evaluate3D (mb == false): one band, q = p, every factor out_scale.
// WMultibandNoise: band b at q = p * qmul, qmul = 2 * 2^(first_band+b) (exact), with the factor of its value
// fv = w_b / out_div * out_scale and of its derivatives fg = fv * qmul, formed in double and rounded once each.  Written
// as one expression, w / div * scale * qmul associates left to right into the same double operations as fv's then * qmul.
struct BandFactors {
    int nbands;
    float qmul[kMaxBands], fv[kMaxBands], fg[kMaxBands];
};

inline BandFactors band_factors(const Bands &d, bool mb, float out_scale)
{
    BandFactors f{1, {1.0f}, {out_scale}, {out_scale}};
    if (!mb) return f;
    f.nbands = d.nbands;
    for (int b = 0; b < d.nbands; ++b) {
        f.qmul[b] = 2.0f * d.band_scale[b];
        const double v = (double)d.band_w[b] / (double)d.out_div * (double)out_scale;
        f.fv[b] = (float)v;
        f.fg[b] = (float)(v * (double)f.qmul[b]);
    }
    return f;
}

#if defined(__HIPCC__)
// The box of geometry geo fits the cap floats the planner reserved for it: always (the planner bounds the box from the same
// coordinates); the kernels return when it does not, uniformly, so that no fill can write past its box.
__device__ __forceinline__ bool brick_box_fits(const int *geo, int cap) { return (long long)geo[3] * geo[4] * geo[5] <= cap; }

// Fills one box of geometry geo (ix0, jy0, kz0, ex, ey, ez) from the tile shifted by (ox, oy, oz) whole cells:
// bb[k][j][i] = coef[Mod(kz0+k+oz)][Mod(jy0+j+oy)][Mod(ix0+i+ox)]; a wave takes whole (k, j) rows.
__device__ __forceinline__ void brick_fill(float *bb, const float *coef, int n, int nmask, const int *geo, int ox, int oy,
                                           int oz, int wave, int lane)
{
    const int ix0 = geo[0], jy0 = geo[1], kz0 = geo[2], ex = geo[3], ey = geo[4], ez = geo[5];
    for (int r = wave; r < ey * ez; r += kGWaves) {
        const int k = r / ey, j = r - k * ey;
        const float *row = coef + ((size_t)dmod(kz0 + k + oz, n, nmask) * n + dmod(jy0 + j + oy, n, nmask)) * n;
        for (int i = lane; i < ex; i += 64) bb[r * ex + i] = row[dmod(ix0 + i + ox, n, nmask)];
    }
}

// A lane's 4 samples in a band's 4-column window: the window's first box column, and per sample q the window's weights.
struct XWin {
    int col;
    float w[4][4], d[4][4];
};

// px: the 4 samples' coordinates; ix0: the box's first cell (geo[0]).
__device__ __forceinline__ void brick_x_window(const float px[4], float qmul, int ix0, XWin &xw)
{
    int m[4];
    float w[4][3], d[4][3];
#pragma unroll
    for (int q = 0; q < 4; ++q) bspline_grad(px[q] * qmul, m[q], w[q], d[q]);
    xw.col = m[0] - 1 - ix0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const bool sh = m[q] != m[0]; // then m[q] == m[0] + 1 (the planner's two_mids)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            xw.w[q][c] = sh ? (c == 0 ? 0.0f : w[q][c - 1]) : (c == 3 ? 0.0f : w[q][c]);
            xw.d[q][c] = sh ? (c == 0 ? 0.0f : d[q][c - 1]) : (c == 3 ? 0.0f : d[q][c]);
        }
    }
}

// ---- the column contractions of the separable kernels, dense grids and brick lists alike: the one statement of their
// arithmetic.  Under a lane's 4 samples lie 4 box columns; a column's z tap k, y tap j lies (k * ey + j) * ex floats behind
// its first tap.  Per column
//     z:  Z_j = sum_k wz_k C[k][j],  Z'_j = sum_k dz_k C[k][j]
//     y:  A = sum_j wy_j Z_j,  B = sum_j dy_j Z_j,  D = sum_j wy_j Z'_j
// and per sample, with its x weights placed in the window (XWin: Wx, Dx, zero outside its three taps),
//     x:  value = sum_i Wx_i A_i,  d/dx = sum_i Dx_i A_i,  d/dy = sum_i Wx_i B_i,  d/dz = sum_i Wx_i D_i.
// Every sum runs in this order, fused: a sample's bits are the same in every kernel that calls these, which is what the
// brick lists promise of the dense default-tier grids and the bounded curl bricks of the gradient bricks' channel 0.
//
// The value (A and the sum over Wx) has one kernel, bricks_sep_kernel, which writes it out from tap3.  The column steps of
// the gradient (z, y -> A, B, D) and of the curl stay written out, from tap3, in their kernels; only their x steps (grad_x,
// curl_x) are functions.  The gradient's, as a function of one column, takes either
// grad3d_grid_sep_kernel<1> from 80 to 81 VGPRs (indexed as here; 95 with the whole 4-column loop inside), 6 waves per SIMD
// to 5, or, indexed k * (ex * ey) + j * ex (78 VGPRs), the brick lists of five bands 3 % of their time.  The curl's, as one
// function of the 4-column loop, keeps every kernel's waves but costs curl_bricks_sep_kernel 4 to 6 VGPRs and timed 0.1 to
// 0.8 % over the parent on the curl and bounded curl brick lists, outside the bound the parent's own two runs allow
// (profiles/sep_contraction_refactor.txt).

// One tap triple: w_2 c2 + (w_1 c1 + w_0 c0).
__device__ __forceinline__ float tap3(const float *w, float c0, float c1, float c2)
{
    return __builtin_fmaf(w[2], c2, __builtin_fmaf(w[1], c1, w[0] * c0));
}

// The gradient: a sample's four channels from its Wx (w) and Dx (d) and the columns' A, B and D.
struct GradSample {
    float v, gx, gy, gz;
};

__device__ __forceinline__ GradSample grad_x(const float *w, const float *d, const float *A, const float *B, const float *D)
{
    GradSample s{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        s.v = __builtin_fmaf(w[c], A[c], s.v);
        s.gx = __builtin_fmaf(d[c], A[c], s.gx);
        s.gy = __builtin_fmaf(w[c], B[c], s.gy);
        s.gz = __builtin_fmaf(w[c], D[c], s.gz);
    }
    return s;
}

// The curl of the potentials psi0, psi1, psi2 (one box each, of one geometry).  v = (d psi2/dy - d psi1/dz,
// d psi0/dz - d psi2/dx, d psi1/dx - d psi0/dy) needs two of the three column contractions per potential:
//     psi0: B, D      psi1: A, D      psi2: A, B  (no Z' at all)
//     vx = sum_i Wx_i (B2 - D1),  vy = sum_i (Wx_i D0 - Dx_i A2),  vz = sum_i (Dx_i A1 - Wx_i B0)
// the components accumulated with signs.  P = B2 - D1.  The kernels fill a CurlColumns column by column, one
// sched_barrier per column (wn_wavelet_curl.hip has its measured numbers); curl_x is the x step.
struct CurlColumns {
    float P[4], D0[4], A2[4], A1[4], B0[4];
};

// acc[component][q] += fg * v_component of sample q (w, d: its Wx, Dx).
__device__ __forceinline__ void curl_x(const float *w, const float *d, const CurlColumns &cols, float fg, float (&acc)[3][4], int q)
{
    float vx = 0.0f, vy = 0.0f, vz = 0.0f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        vx = __builtin_fmaf(w[c], cols.P[c], vx);
        vy = __builtin_fmaf(w[c], cols.D0[c], vy);
        vy = __builtin_fmaf(-d[c], cols.A2[c], vy);
        vz = __builtin_fmaf(d[c], cols.A1[c], vz);
        vz = __builtin_fmaf(-w[c], cols.B0[c], vz);
    }
    acc[0][q] = __builtin_fmaf(fg, vx, acc[0][q]);
    acc[1][q] = __builtin_fmaf(fg, vy, acc[1][q]);
    acc[2][q] = __builtin_fmaf(fg, vz, acc[2][q]);
}

// Stores a lane's 4 samples of CH channel volumes (vol floats apart) at dst, the first sample's address in channel 0:
// one float4 per channel, or scalars where rows are not 16-byte aligned (vec4_ok == 0) or the row ends inside the 4.
template <int CH>
__device__ __forceinline__ void brick_store_row(float *dst, size_t vol, int vec4_ok, int x0, int nx, const float (&acc)[CH][4])
{
    if (vec4_ok && x0 + 3 < nx) {
#pragma unroll
        for (int ch = 0; ch < CH; ++ch)
            *reinterpret_cast<v4f *>(dst + ch * vol) = v4f{acc[ch][0], acc[ch][1], acc[ch][2], acc[ch][3]};
    } else {
#pragma unroll
        for (int ch = 0; ch < CH; ++ch)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (x0 + q < nx) dst[ch * vol + q] = acc[ch][q];
    }
}
#endif

} // namespace wn
