// wn_brick_list.hpp -- what the brick-list kernels share: the value bricks of wn_wavelet_bricks.hip (include/wnoise_bricks.h)
// and the gradient and curl bricks of wn_wavelet_brick_fields.hip (include/wnoise_brick_fields.h).
//
// A brick is 8 x 8 x 8 samples of the lattice a wn_grid describes, named by a device triple (bx, by, bz); the volume's extents
// say which bricks are in range.  Here: the entry points' checks after their tile and bands, the volume in bricks and the
// lattice rounded up to whole bricks (what the separable kernels' regime is checked on), and on the device the in-range
// decision, a sample's coordinate and the geometry of a band's coefficient box under a brick.
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
#endif

} // namespace wn
