/* wnoise_brick_fields.h -- C ABI of the derivative fields on sparse brick lists of the 3-D wavelet volume: the analytic
 * gradient {value, d/dx, d/dy, d/dz} and the divergence-free curl velocity {vx, vy, vz} of evaluate3D and WMultibandNoise
 * on a list of 8 x 8 x 8 leaves of a dense lattice, exported by libwnoise_hip.so beside the value bricks of
 * wnoise_bricks.h, which this header includes; absent from the reference.  Conventions as in wnoise.h.
 *
 * A displacement shell needs normals and a narrow-band smoke solver a velocity, both only in the occupied bricks.  These
 * calls evaluate the lattice of wn_eval3d_grad_grid / wn_multiband3d_grad_grid, or of wn_eval3d_curl_grid /
 * wn_multiband3d_curl_grid (wnoise.h), on the listed bricks only.
 *
 * Brick list, lattice, coordinates (the z index is absolute), which bricks are IN RANGE and written, duplicates, and that the
 * slots of out-of-range bricks are left untouched: exactly as wnoise_bricks.h states them for wn_eval3d_bricks /
 * wn_multiband3d_bricks.  So are the argument checks with their messages (WN_Z_CONST is refused; n == 0 is WN_OK after
 * that; WN_ERR_NO_DEVICE without a HIP device), and that the calls only enqueue on `stream` -- no allocation, no
 * synchronisation -- and can be captured into a graph.  What differs is stated here.
 *
 * Channels.  CH = 4 for the gradient calls (value, d/dx, d/dy, d/dz) and CH = 3 for the curl calls (vx, vy, vz).
 * Derivatives are taken with respect to the sample's noise-space coordinate (the value passed to evaluate3D; multiband: the
 * lattice coordinate p), and out_scale multiplies every channel last.  The multiband conventions, offsets9_host (the
 * whole-cell offsets of the three potentials, read before the call returns) and their checks are those of
 * wn_eval3d_grad_grid / wn_eval3d_curl_grid and their multiband forms; the curl calls refuse offsets9_host == NULL.
 *
 * Output layout.  CH consecutive slot arrays, each in wn_eval3d_bricks' layout: sample (lx, ly, lz) of brick i, channel ch, is
 *     out_dev[(ch * n + i) * 512 + lx + 8 * (ly + 8 * lz)].
 * out_dev needs only a float's alignment; a 16-byte aligned out_dev (every channel array is then aligned too) is written
 * with float4 stores, others with scalar stores, and a kernel's bits do not depend on where the output lies.  The CH * n * 512
 * floats are the only bytes a call may touch; CH * n * 512 overflowing size_t is WN_ERR_INVALID.
 *
 * Tiers, through g->flags.
 *   WN_GRID_EXACT    every channel has the bits of wn_eval3d_grad_points / wn_multiband3d_grad_points (curl calls:
 *                    wn_eval3d_curl_points / wn_multiband3d_curl_points) at the sample's float coordinates, times
 *                    out_scale: also the bits of the same sample of the derivative grids under WN_GRID_EXACT.  Channel 0
 *                    of the gradient calls has the bits of wn_eval3d_bricks / wn_multiband3d_bricks under WN_GRID_EXACT.
 *   WN_GRID_DEFAULT  a separable kernel, in the regime wnoise_bricks.h gives its default tier (outside it, an empty tile
 *                    and no active band included, the exact kernel serves the lattice): per brick and band a coefficient
 *                    box in LDS (curl: one per potential), contracted over z, then y, then x with fused multiply-adds.
 *                    Every channel stays within the tolerance wnoise.h gives the dense default tier:
 *                    G = 1e-5 * |out_scale| (multiband: * sum_b |w_b| 2^(first_band+b+1) / out_div) for the gradient calls,
 *                    2 G for the curl calls.  A sample's bits depend only on its lattice index, the lattice, the tile, the
 *                    bands and the offsets.  Two consequences are part of the contract: channel 0 of the gradient calls has
 *                    the bits of the default-tier wn_eval3d_bricks / wn_multiband3d_bricks; and whenever the dense
 *                    wn_*_grad_grid / wn_*_curl_grid call over the same lattice also runs its separable brick kernel,
 *                    the sample has that dense sample's bits.
 *
 * Not provided: projected bricks; bounded curl bricks (wnoise_bounded.h's obstacles: they are wnoise_bounded_bricks.h's
 * wn_eval3d_curl_bounded_bricks / wn_multiband3d_curl_bounded_bricks); brick edges other than 8.
 */
#ifndef WNOISE_BRICK_FIELDS_H
#define WNOISE_BRICK_FIELDS_H

#include "wnoise_bricks.h"

#ifdef __cplusplus
extern "C" {
#endif

WN_API int wn_eval3d_grad_bricks(const wn_tile *tile3d, const wn_grid *g, const int32_t *bricks_dev, size_t n,
                                 float *out_dev, void *stream);
WN_API int wn_multiband3d_grad_bricks(const wn_tile *tile3d, const wn_grid *g, const int32_t *bricks_dev, size_t n,
                                      float s, int first_band, int nbands, const float *w_host, float var_per_band,
                                      float *out_dev, void *stream);
WN_API int wn_eval3d_curl_bricks(const wn_tile *tile3d, const wn_grid *g, const int32_t *bricks_dev, size_t n,
                                 const int32_t *offsets9_host, float *out_dev, void *stream);
WN_API int wn_multiband3d_curl_bricks(const wn_tile *tile3d, const wn_grid *g, const int32_t *bricks_dev, size_t n,
                                      const int32_t *offsets9_host, float s, int first_band, int nbands,
                                      const float *w_host, float var_per_band, float *out_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* WNOISE_BRICK_FIELDS_H */
