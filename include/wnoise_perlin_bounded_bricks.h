/* wnoise_perlin_bounded_bricks.h -- C ABI of the curl noise of Perlin noise potentials with solid boundaries on sparse brick
 * lists: the lattice, list and slots of wn_perlin_curl_bricks (wnoise_perlin_bricks.h) with the obstacles and the field
 * v = A (curl Psi) + grad A x Psi of wnoise_perlin_bounded.h, exported by libwnoise_hip.so; absent from the reference.  The
 * Perlin twin of wnoise_bounded_bricks.h.  This header includes wnoise_perlin_bricks.h and wnoise_perlin_bounded.h.
 * Conventions as in wnoise.h.
 *
 * Unchanged from wn_perlin_curl_bricks, exactly as wnoise_perlin_bricks.h states them: the brick list, the lattice and its
 * coordinates (the z index is absolute: 8 bz + lz), which bricks are IN RANGE and written whole, duplicates, that the slots
 * of out-of-range bricks are left untouched in all three channels, that the list is only read; the layout
 *     out_dev[(ch * n + i) * 512 + lx + 8 * (ly + 8 * lz)],  ch = 0, 1, 2 for vx, vy, vz;
 * that any float-aligned out_dev is accepted and a 16-byte aligned one is written with float4 stores; that the 3 * n * 512
 * floats are the only bytes a call may touch; that g->flags is accepted and ignored; and that the call only enqueues on
 * `stream`: no allocation, no synchronisation, no launch on the null stream, no host read of the list.  It can be captured
 * into a graph and replayed on other lists in the same buffers.
 *
 * Obstacles: wnoise_bounded.h's wn_obstacle list, in the coordinate that noise() / turb() / fractal_noise() receives -- the
 * sample's float lattice coordinate.  obstacles_host and offsets9_host are read before the call returns.
 *
 * Bits.  Every sample of every component is (float) of the matching record of wn_perlin_curl_bounded_points_f32 at the
 * sample's float coordinates, times out_scale, for all three kinds and every depth >= 0 (the kernel tabulates one octave at
 * a time and has no depth cap).  INSIDE samples are (float)0.0 * out_scale; FAR samples carry the bits of
 * wn_perlin_curl_bricks; NEAR samples compose A, G, the curl and the potential values as wnoise_perlin_bounded.h states, in
 * fp64, unfused.  A sample's bits depend on its own lattice index, the lattice, the table, kind, depth, the offsets and the
 * obstacle list only: not on its brick's place in the list, the list's length, duplicates, where the output lies, or the
 * volume's extent inside boundary bricks.
 *
 * nobs == 0: the call is wn_perlin_curl_bricks, with that call's checks; a NULL obstacle list is valid.
 *
 * Argument checks, in this order.  Those of wn_perlin_curl_bricks on kind, depth, perm, g and offsets9_host == NULL, with its
 * messages; then the obstacle checks of wnoise_bounded.h, each WN_ERR_INVALID, also with n == 0; then wnoise_bricks.h's, each
 * WN_ERR_INVALID: z_mode == WN_Z_CONST; after that n == 0 is WN_OK; bricks_dev or out_dev NULL; 3 * n * 512 overflowing
 * size_t; then an empty volume is WN_OK without a launch.  Without a HIP device: WN_ERR_NO_DEVICE, before any of these
 * checks.  A refused call writes nothing.
 *
 * Not provided: potential-value bricks; gradient or value bricks with obstacles; moving obstacles; dense bounded grids.
 */
#ifndef WNOISE_PERLIN_BOUNDED_BRICKS_H
#define WNOISE_PERLIN_BOUNDED_BRICKS_H

#include "wnoise_perlin_bricks.h"
#include "wnoise_perlin_bounded.h"

#ifdef __cplusplus
extern "C" {
#endif

WN_API int wn_perlin_curl_bounded_bricks(const wn_perm *perm, const wn_grid *g, int kind, int depth,
                                         const int32_t *offsets9_host, const wn_obstacle *obstacles_host, int nobs,
                                         const int32_t *bricks_dev, size_t n, float *out_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* WNOISE_PERLIN_BOUNDED_BRICKS_H */
