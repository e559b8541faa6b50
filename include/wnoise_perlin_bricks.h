/* wnoise_perlin_bricks.h -- C ABI of sparse brick lists of Perlin improved noise: perlin::noise, RTOW turb and
 * perlin::fractal_noise, their analytic gradients {value, d/dx, d/dy, d/dz} and the curl {vx, vy, vz} of three shifted
 * potentials on a list of 8 x 8 x 8 leaves of a dense lattice, exported by libwnoise_hip.so; absent from the reference.
 * This header includes wnoise_bricks.h (WN_BRICK and the list conventions) and wnoise_perlin_curl.h (the kinds
 * WN_PERLIN_CURL_* and the offsets).  Conventions as in wnoise.h.
 *
 * One entry point per dense Perlin grid entry point, with (bricks_dev, n) before the output:
 *     wn_perlin_bricks              wn_perlin_grid               1 channel
 *     wn_perlin_turb_bricks         wn_perlin_turb_grid          1
 *     wn_perlin_fractal_bricks      wn_perlin_fractal_grid       1
 *     wn_perlin_grad_bricks         wn_perlin_grad_grid          4  value, d/dx, d/dy, d/dz
 *     wn_perlin_turb_grad_bricks    wn_perlin_turb_grad_grid     4
 *     wn_perlin_fractal_grad_bricks wn_perlin_fractal_grad_grid  4
 *     wn_perlin_curl_bricks         wn_perlin_curl_grid          3  vx, vy, vz
 * A call evaluates the lattice its dense entry point evaluates from the same perm, g, kind, depth and offsets9_host, on the
 * listed bricks only.
 *
 * Brick list, lattice, coordinates (the z index is absolute: 8 bz + lz, not relative to z0), which bricks are IN RANGE --
 * from g->nx, g->ny and [g->z0, g->z1) -- and written whole, also past nx, ny, z1 and below z0 inside a boundary brick;
 * duplicates; that the slots of out-of-range bricks are left untouched in every channel; that the list is only read; and
 * that the in-range decision is uniform per wave: exactly as wnoise_bricks.h states them for wn_eval3d_bricks.
 *
 * Output layout, as in wnoise_brick_fields.h: CH consecutive slot arrays of n slots; sample (lx, ly, lz) of brick i,
 * channel ch, is
 *     out_dev[(ch * n + i) * 512 + lx + 8 * (ly + 8 * lz)].
 * out_dev needs only a float's alignment; a 16-byte aligned out_dev (every slot of every channel is then aligned too) is
 * written with float4 stores, others with scalar stores, and the bits do not depend on where the output lies.  The
 * CH * n * 512 floats are the only bytes a call may touch.
 *
 * One tier: g->flags is accepted and ignored, as in wn_perlin_curl_grid.
 *
 * Bits.  Every sample of every channel has the bits of the same lattice index in the matching dense entry point with
 * z_mode == WN_Z_LATTICE: that is (float) of the matching point entry (wn_perlin_points_vec3, wn_perlin_turb_points,
 * wn_perlin_fractal_points, wn_perlin_grad_points_vec3, wn_perlin_turb_grad_points, wn_perlin_fractal_grad_points,
 * wn_perlin_curl_points_vec3) at the lattice's float coordinates, times out_scale.  This holds for every depth >= 0 (turb at
 * depth 0 is 0 in every channel; the kernel tabulates one octave at a time and has no depth cap), and a sample's bits depend
 * on its own lattice index, the lattice, the table, kind, depth and offsets only: not on its brick's place in the list, the
 * list's length, its neighbours, or how a volume is cut into calls.  The gradient is taken with respect to the coordinate
 * passed to noise() / turb() / fractal_noise(); turb's sign rule, fractal_noise's division, the curl's potentials and its one
 * fp64 subtraction per component are those of wnoise.h and wnoise_perlin_curl.h.
 *
 * Argument checks, in this order.  Those of the matching dense entry point on kind and depth (wn_perlin_curl_bricks: kind in
 * 0..2, and depth >= 0 for WN_PERLIN_CURL_TURB; the turb calls: depth >= 0), on perm and on g, with their messages;
 * wn_perlin_curl_bricks then refuses offsets9_host == NULL (the nine offsets are read before the call returns).  Then
 * wnoise_bricks.h's, each WN_ERR_INVALID: z_mode == WN_Z_CONST (bricks are three-dimensional); after that n == 0 is WN_OK;
 * bricks_dev or out_dev NULL; CH * n * 512 overflowing size_t; then an empty volume is WN_OK without a launch.  Without a
 * HIP device: WN_ERR_NO_DEVICE.  A refused call writes nothing.
 *
 * The calls only enqueue on `stream`: no allocation, no synchronisation, no launch on the null stream, no host read of the
 * list.  They can be captured into a graph and replayed on other lists in the same buffers.
 *
 * Not provided: solid boundaries on the curl bricks (wnoise_perlin_bounded.h's obstacles) in this header: they are
 * wnoise_perlin_bounded_bricks.h's wn_perlin_curl_bounded_bricks; footprints; brick edges other than 8.
 */
#ifndef WNOISE_PERLIN_BRICKS_H
#define WNOISE_PERLIN_BRICKS_H

#include "wnoise_bricks.h"
#include "wnoise_perlin_curl.h"

#ifdef __cplusplus
extern "C" {
#endif

WN_API int wn_perlin_bricks(const wn_perm *perm, const wn_grid *g, const int32_t *bricks_dev, size_t n, float *out_dev,
                            void *stream);
WN_API int wn_perlin_turb_bricks(const wn_perm *perm, const wn_grid *g, int depth, const int32_t *bricks_dev, size_t n,
                                 float *out_dev, void *stream);
WN_API int wn_perlin_fractal_bricks(const wn_perm *perm, const wn_grid *g, const int32_t *bricks_dev, size_t n,
                                    float *out_dev, void *stream);
WN_API int wn_perlin_grad_bricks(const wn_perm *perm, const wn_grid *g, const int32_t *bricks_dev, size_t n, float *out_dev,
                                 void *stream);
WN_API int wn_perlin_turb_grad_bricks(const wn_perm *perm, const wn_grid *g, int depth, const int32_t *bricks_dev, size_t n,
                                      float *out_dev, void *stream);
WN_API int wn_perlin_fractal_grad_bricks(const wn_perm *perm, const wn_grid *g, const int32_t *bricks_dev, size_t n,
                                         float *out_dev, void *stream);
WN_API int wn_perlin_curl_bricks(const wn_perm *perm, const wn_grid *g, int kind, int depth, const int32_t *offsets9_host,
                                 const int32_t *bricks_dev, size_t n, float *out_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* WNOISE_PERLIN_BRICKS_H */
