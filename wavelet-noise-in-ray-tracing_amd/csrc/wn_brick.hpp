// wn_brick.hpp -- the frame of the separable brick kernels of the derivative grids: grad3d_grid_sep_kernel<NB>
// (wn_wavelet_grad.hip) and curl3d_grid_sep_kernel<NB> (wn_wavelet_curl.hip).
//
// A workgroup (4 waves) owns a brick of 256 x 8 x 8 samples.  For every band it stages `boxes` coefficient boxes (gradient 1;
// curl 3, one per potential, of one geometry) in LDS once, periodic wrap resolved, x fastest.  A lane owns 4 consecutive x
// samples, a wave rows (y, z) of the brick; 4 consecutive samples span at most two mids, so their taps lie in the 4 box
// columns m0 - 1 .. m0 + 2, and each sample's x weights are placed in that window (zero outside its three taps).  The
// kernels keep what differs: the column contraction between "z, y" and "x", their factors and the channel count.  The frame
// sums nothing: a sample's bits depend on its own weights and coefficients only, not on its place in a brick or z-slab.
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
