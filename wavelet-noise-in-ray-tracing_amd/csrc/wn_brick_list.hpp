// wn_brick_list.hpp -- what the brick-list kernels share: the value bricks of wn_wavelet_bricks.hip (include/wnoise_bricks.h),
// the gradient and curl bricks of wn_wavelet_brick_fields.hip (include/wnoise_brick_fields.h) and the bounded curl bricks of
// wn_wavelet_bounded_bricks.hip (include/wnoise_bounded_bricks.h).
//
// A brick is 8 x 8 x 8 samples of the lattice a wn_grid describes, named by a device triple (bx, by, bz); the volume's extents
// say which bricks are in range.  Here: the entry points' checks after their tile and bands, the volume in bricks and the
// lattice rounded up to whole bricks (what the separable kernels' regime is checked on), and on the device the in-range
// decision, a sample's coordinate and the geometry of a band's coefficient box under a brick; and the separable kernels'
// one argument struct with its regime check and setup, and their frame (pair_brick, fill_box, store_slots).  Their
// arithmetic between staging and store is wn_brick.hpp's column contractions.  Each file still states its own box and
// launch caps (kBoxCap, k*BlockCap) and passes its kBoxCap to brick_sep_args.
#pragma once

#include "wn_brick.hpp"
#include "wnoise_bricks.h"

#include <climits>
#include <cstdint>

namespace wn {

constexpr int kBrickEdge = WN_BRICK, kBrickSamples = kBrickEdge * kBrickEdge * kBrickEdge;

// The bricks of the volume: 0 <= bx < nbx, 0 <= by < nby, bz0 <= bz < bz1.
struct BrickRange {
    int nbx, nby, bz0, bz1;
};

inline long long floor_div8(long long v) { return v >= 0 ? v / kBrickEdge : -((-v + kBrickEdge - 1) / kBrickEdge); }

// What a brick-list call launches on.
struct BrickListPlan {
    GridArgs g;      // the lattice with z0 == nz == 0: the kernels form z coordinates from absolute indices
    BrickRange range;
    GridArgs gr;     // the lattice rounded up to whole bricks (what an in-range brick can reach), when `roundable`
    bool roundable;
};

// The checks of a brick-list entry point after its tile (and bands), for `ch` channel arrays of n slots; then the plan.
// *launch is false when the call is done without a launch: a refusal (the status says so), n == 0, or an empty volume.
inline int brick_list_plan(const wn_grid *grid, const int32_t *bricks_dev, size_t n, int ch, const float *out_dev,
                           BrickListPlan *p, bool *launch)
{
    *launch = false;
    GridArgs g;
    const int rc = check_grid(grid, true, &g);
    if (rc) return rc;
    if (grid->z_mode == WN_Z_CONST)
        return fail(WN_ERR_INVALID, "wn_grid.z_mode must be WN_Z_LATTICE: bricks are three-dimensional");
    if (n == 0) return WN_OK;
    if (!bricks_dev) return fail(WN_ERR_INVALID, "bricks_dev is NULL");
    if (!out_dev) return fail(WN_ERR_INVALID, "out_dev is NULL");
    if (n > SIZE_MAX / kBrickSamples / (size_t)ch)
        return ch == 1 ? fail(WN_ERR_INVALID, "n * 512 overflows size_t") : fail(WN_ERR_INVALID, "%d * n * 512 overflows size_t", ch);
    if (g.nx == 0 || g.ny == 0 || g.nz == 0) return WN_OK; // an empty volume: no brick is in range

    const long long bz0 = floor_div8(g.z0), bz1 = -floor_div8(-((long long)g.z0 + g.nz));
    p->range = BrickRange{(int)(((long long)g.nx + kBrickEdge - 1) / kBrickEdge), (int)(((long long)g.ny + kBrickEdge - 1) / kBrickEdge),
                          (int)bz0, (int)bz1};
    const long long rx = (long long)p->range.nbx * kBrickEdge, ry = (long long)p->range.nby * kBrickEdge;
    p->roundable = rx <= INT_MAX && ry <= INT_MAX && bz0 * kBrickEdge >= INT_MIN && bz1 * kBrickEdge <= INT_MAX;
    g.z0 = 0;
    g.nz = 0;
    p->g = g;
    p->gr = g;
    if (p->roundable) {
        p->gr.nx = (int)rx;
        p->gr.ny = (int)ry;
        p->gr.z0 = (int)(bz0 * kBrickEdge);
        p->gr.nz = (int)((bz1 - bz0) * kBrickEdge);
    }
    *launch = true;
    return WN_OK;
}

// ---- the separable kernels of the three files: value, gradient, curl and bounded curl bricks
struct FieldBand : BrickBand {
    float fv, fg; // factors of the band's value and of its derivatives (wn::band_factors)
};

// What a separable kernel launches on; the bounded curl bricks add their obstacles.
struct BrickSepArgs {
    const float *coef; // linear tile
    int n, nmask;
    int off[9]; // curl: (x, y, z) of psi0, psi1, psi2, each in [0, n); else 0
    GridArgs g; // z0 == 0
    float inv_den;
    BrickRange range;
    const int32_t *bricks;
    size_t count;
    float *out;
    int vec4_ok; // out is 16-byte aligned, and with it every slot of every channel
    FieldBand band[kMaxBands];
};

// The regime of the separable kernels, checked on the lattice rounded up to whole bricks (plan.gr), and their arguments: a
// tile that is not empty, and in every band a step >= 0 below 1/3 cell (LatticeStep::two_mids) with coordinates inside the
// planners' gate; the box of 8 samples then has at most 6 cells per axis and always fits box_cap (the file's kBoxCap).
// false: outside the regime, *a is not to be launched on.  A band keeps `boxes` boxes (the curl: one per potential, shifted
// by off9).
inline bool brick_sep_args(const wn_tile *tile, const BrickListPlan &plan, const int *off9, int boxes, int box_cap,
                           const BandFactors &f, const int32_t *bricks, size_t n, float *out_dev, BrickSepArgs *a)
{
    if (tile->n == 0 || !plan.roundable || f.nbands < 1 || f.nbands > kMaxBands) return false;
    for (int b = 0; b < f.nbands; ++b) {
        LatticeStep ls;
        if (!lattice_step(plan.gr, plan.g.octave_scale * f.qmul[b], false, false, 0.0, &ls) || !ls.two_mids()) return false;
        if ((ls.extent(kBrickEdge) + 1) * ls.extent(kBrickEdge) * ls.extent(kBrickEdge) > box_cap) return false; // never inside two_mids
        a->band[b].qmul = f.qmul[b];
        a->band[b].box_off = b * box_cap * boxes;
        a->band[b].box_cap = box_cap;
        a->band[b].fv = f.fv[b];
        a->band[b].fg = f.fg[b];
    }
    a->coef = tile->dev;
    a->n = tile->n;
    a->nmask = pow2_mask(tile->n);
    for (int i = 0; i < 9; ++i) a->off[i] = off9 ? off9[i] : 0;
    a->g = plan.g;
    a->inv_den = inv_den_of(plan.g.den);
    a->range = plan.range;
    a->bricks = bricks;
    a->count = n;
    a->out = out_dev;
    a->vec4_ok = (reinterpret_cast<uintptr_t>(out_dev) & 15) == 0;
    return true;
}

#if defined(__HIPCC__)
__device__ __forceinline__ bool brick_in_range(const BrickRange &r, int bx, int by, int bz)
{
    return bx >= 0 && bx < r.nbx && by >= 0 && by < r.nby && bz >= r.bz0 && bz < r.bz1;
}

// The coordinate of lattice index i (x, y and z alike: z indices are absolute), wn::lattice_coord's bits: the division is an
// exact multiply when den is a power of two (inv_den = wn::inv_den_of(den), else 0).
__device__ __forceinline__ float brick_coord(const GridArgs &g, float den, float inv_den, int i)
{
    return lattice_coord_fast(i, den, inv_den, g.base_range, g.octave_scale, g.post_scale);
}

// One axis of a band's box under the 8 samples from index `first`: coordinates are monotone in the index, so the mids of the
// first and the last sample bound all of them; one cell of support on either side.
__device__ __forceinline__ void box_axis(const GridArgs &g, float den, float inv_den, int first, float qmul, int &lo, int &ext)
{
    int m0, m1;
    float w0, w1, w2;
    bspline(brick_coord(g, den, inv_den, first) * qmul, m0, w0, w1, w2);
    bspline(brick_coord(g, den, inv_den, first + kBrickEdge - 1) * qmul, m1, w0, w1, w2);
    lo = min(m0, m1) - 1;
    ext = abs(m1 - m0) + 3;
}

// geo = (ix0, jy0, kz0, ex, ey, ez) of wn::brick_fill; x carries the window's fourth column (zero weight, finite values).
__device__ __forceinline__ void box_geometry(const GridArgs &g, float den, float inv_den, int bx, int by, int bz, float qmul,
                                             int geo[6])
{
    box_axis(g, den, inv_den, kBrickEdge * bx, qmul, geo[0], geo[3]);
    box_axis(g, den, inv_den, kBrickEdge * by, qmul, geo[1], geo[4]);
    box_axis(g, den, inv_den, kBrickEdge * bz, qmul, geo[2], geo[5]);
    geo[3] += 1;
}

// ---- the frame of the separable kernels: 256 lanes, two bricks per workgroup, 128 lanes per brick.
// Brick i of the list, read with the same address in every lane of a wave: false when the list has ended or the brick is
// out of range.
__device__ __forceinline__ bool pair_brick(const BrickSepArgs &a, size_t i, int &bx, int &by, int &bz)
{
    bx = by = bz = 0;
    if (i >= a.count) return false;
    bx = __builtin_amdgcn_readfirstlane(a.bricks[3 * i]);
    by = __builtin_amdgcn_readfirstlane(a.bricks[3 * i + 1]);
    bz = __builtin_amdgcn_readfirstlane(a.bricks[3 * i + 2]);
    return brick_in_range(a.range, bx, by, bz);
}

// bb[k][j][i] = coef[Mod(kz0+k+oz)][Mod(jy0+j+oy)][Mod(ix0+i+ox)]: wn::brick_fill's box, the brick's 128 lanes over the flat
// box (rows are at most 7 cells: brick_fill's row per wave would leave 57 of 64 lanes idle).
__device__ __forceinline__ void fill_box(float *bb, const BrickSepArgs &a, const int geo[6], int ox, int oy, int oz, int l)
{
    const int ex = geo[3], exy = geo[3] * geo[4], cells = exy * geo[5];
    for (int c = l; c < cells; c += 128) {
        const int k = c / exy, r = c - k * exy;
        const int j = r / ex, ii = r - j * ex;
        bb[c] = a.coef[((size_t)dmod(geo[2] + k + oz, a.n, a.nmask) * a.n + dmod(geo[1] + j + oy, a.n, a.nmask)) * a.n +
                       dmod(geo[0] + ii + ox, a.n, a.nmask)];
    }
}

// A lane's 4 samples of CH channel arrays (chan floats apart) at dst, its first sample's address in channel 0.
template <int CH>
__device__ __forceinline__ void store_slots(float *dst, size_t chan, int vec4_ok, const float (&acc)[CH][4])
{
    if (vec4_ok) {
#pragma unroll
        for (int ch = 0; ch < CH; ++ch) *reinterpret_cast<v4f *>(dst + ch * chan) = v4f{acc[ch][0], acc[ch][1], acc[ch][2], acc[ch][3]};
    } else {
#pragma unroll
        for (int ch = 0; ch < CH; ++ch)
#pragma unroll
            for (int q = 0; q < 4; ++q) dst[ch * chan + q] = acc[ch][q];
    }
}
#endif

} // namespace wn
