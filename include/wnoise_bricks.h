/* wnoise_bricks.h -- C ABI of sparse brick lists of the 3-D wavelet volume: evaluate3D and WMultibandNoise on a list of
 * 8 x 8 x 8 leaves of a dense lattice, exported by libwnoise_hip.so beside the entry points of wnoise.h, which this header
 * includes; absent from the reference.  Conventions (status codes, *_dev / *_host pointers, `stream`, handles) as in
 * wnoise.h.
 *
 * A sparse volume (smoke, clouds, a displacement shell) keeps its voxels in bricks and needs the noise only in the occupied
 * ones.  A brick is a tiny dense lattice: the call evaluates the lattice that `g` describes -- wn_eval3d_grid's, or
 * wn_multiband3d_grid's -- on the listed bricks only, each into a 2 KiB slot of its own.
 *
 * Brick list and lattice.  bricks_dev holds n packed int32 triples (bx, by, bz) on the device (int32 alignment only).
 * Brick i covers the lattice indices [8 bx, 8 bx + 8) x [8 by, 8 by + 8) x [8 bz, 8 bz + 8).  Index i_a of axis a has the
 * coordinate of wnoise.h,
 *     c_a = (((float)i_a / (float)den) * base_range) * octave_scale * post_scale,
 * evaluated in float in this order, z included (the z index is absolute: 8 bz + lz, not relative to z0); out_scale
 * multiplies the result last.  The multiband form follows wn_multiband3d_grid: p is that coordinate (use
 * octave_scale = post_scale = 1), band b runs while s + first_band + b < 0 at q = 2 * p * 2^(first_band+b) with weight
 * w_host[b], and the sum is divided by sqrt(sum_b w[b]^2 * var_per_band) over ALL nbands when that is not zero.
 *
 * Output layout.  Sample (lx, ly, lz) of brick i is out_dev[512 * i + lx + 8 * (ly + 8 * lz)]; out_dev needs only a float's
 * alignment (16-byte aligned slots are written with float4 stores, others with scalar stores), and a kernel's bits do not
 * depend on where the output lies.
 *
 * Which bricks are written.  The list is device data and the call does not synchronise to look at it, so g->nx, g->ny and
 * [g->z0, g->z1) bound the volume: a brick is IN RANGE iff 0 <= bx < ceil(nx / 8), 0 <= by < ceil(ny / 8) and
 * floor(z0 / 8) <= bz < ceil(z1 / 8) (an empty volume -- nx, ny or z1 - z0 zero -- has no brick in range).  All 512 samples
 * of an in-range brick are written, those whose index reaches past nx, ny or z1 (or lies below z0) inside a boundary brick
 * included: the formula defines them.  The 512 floats of an out-of-range brick are left untouched; negative bx and by are
 * out of range.  Nothing else is written: the n * 512 floats are the only bytes the call may touch, and the list itself is
 * only read.  Duplicates are allowed, each fills its own slot with the same bits.  The kernels decide in-range per brick,
 * uniformly for a wave.
 *
 * Tiers, through g->flags as for the dense grids.
 *   WN_GRID_EXACT    every sample has the bits of wn_eval3d_points / wn_multiband3d_points at the sample's float
 *                    coordinates, times out_scale: also the bits of the same sample of wn_eval3d_grid /
 *                    wn_multiband3d_grid under WN_GRID_EXACT.
 *   WN_GRID_DEFAULT  the separable kernel: per brick and band a coefficient box in LDS, contracted over z, then y, then x
 *                    with fused multiply-adds; every sample within 1e-5 of the reference (the default tier's tolerance of
 *                    wnoise.h).  A sample's bits depend on its own lattice index, the lattice, the tile and the bands only:
 *                    not on its brick's place in the list, the list's length, its neighbours, or how a volume is cut into
 *                    calls.  A lattice outside that kernel's regime -- a step of 1/3 cell or more in some band, coordinates
 *                    past 1e6 cells, a negative step, or no active band -- is served by the exact kernel; the regime is
 *                    checked on the extents rounded up to whole bricks.
 * An empty tile writes zeros (times out_scale) to the in-range bricks.
 *
 * Argument checks: those of wn_eval3d_grid / wn_multiband3d_grid on the tile, g and the bands, with their messages.  Then,
 * each WN_ERR_INVALID: z_mode == WN_Z_CONST (bricks are three-dimensional); after that n == 0 is WN_OK; bricks_dev or out_dev
 * NULL; n * 512 overflowing size_t.  Without a HIP device: WN_ERR_NO_DEVICE.
 *
 * The calls only enqueue on `stream`: no allocation, no synchronisation, no launch on the null stream, no host read after
 * they return.  They can be captured into a graph and replayed on other lists in the same buffers.
 *
 * Not provided: gradient, curl and projected bricks (gradient and curl bricks: wnoise_brick_fields.h, which includes this
 * header); brick edges other than 8; building a brick list from a mask or a level set (the caller's sparse structure
 * already has it).
 */
#ifndef WNOISE_BRICKS_H
#define WNOISE_BRICKS_H

#include "wnoise.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WN_BRICK 8                      /* samples per brick edge; 512 samples, 2048 bytes per brick */

WN_API int wn_eval3d_bricks(const wn_tile *tile3d, const wn_grid *g, const int32_t *bricks_dev, size_t n,
                            float *out_dev, void *stream);
WN_API int wn_multiband3d_bricks(const wn_tile *tile3d, const wn_grid *g, const int32_t *bricks_dev, size_t n,
                                 float s, int first_band, int nbands, const float *w_host, float var_per_band,
                                 float *out_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* WNOISE_BRICKS_H */
