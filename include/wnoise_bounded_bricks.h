/* wnoise_bounded_bricks.h -- C ABI of solid boundaries on the curl brick lists of the 3-D wavelet volume: the divergence-free
 * velocity {vx, vy, vz} of wnoise_brick_fields.h's curl bricks with the potential faded to zero towards the obstacles of
 * wnoise_bounded.h, v = curl(A Psi) = A (curl Psi) + grad A x Psi, on a list of 8 x 8 x 8 leaves of a dense lattice; exported
 * by libwnoise_hip.so; absent from the reference.  This header includes wnoise_brick_fields.h and wnoise_bounded.h.
 *
 * A narrow-band smoke solver has walls, a floor and bodies in the flow: these calls give it the bounded velocity in the
 * occupied bricks only, without expanding every brick into a point list for wn_eval3d_curl_bounded_points.
 *
 * Exactly as in wn_eval3d_curl_bricks / wn_multiband3d_curl_bricks, with CH = 3: the brick list, the lattice, coordinates
 * (the z index is absolute), which bricks are IN RANGE and written, that the slots of out-of-range bricks are left
 * untouched, duplicates; the output layout, sample (lx, ly, lz) of brick i, component ch, at
 *     out_dev[(ch * n + i) * 512 + lx + 8 * (ly + 8 * lz)],
 * from any float-aligned out_dev, with float4 stores when it is 16-byte aligned; the argument checks with their messages and
 * order (WN_Z_CONST is refused; n == 0 is WN_OK after that; NULL pointers; 3 * n * 512 overflowing size_t is
 * WN_ERR_INVALID; offsets9_host == NULL is refused; WN_ERR_NO_DEVICE without a HIP device); and that the calls only enqueue on
 * `stream` -- no allocation, no synchronisation -- and can be captured into a graph.
 *
 * New.  The obstacle checks of wnoise_bounded.h, with its messages, run after the tile, offset and band checks and before
 * the brick-list checks.  A refused call writes nothing.  The obstacle list is read before the call returns.  Obstacles live
 * in the coordinate the derivative is taken in: the sample's noise-space coordinate c_a of wnoise_bricks.h for
 * wn_eval3d_curl_bounded_bricks, the lattice coordinate p for wn_multiband3d_curl_bounded_bricks.
 *
 * Arithmetic, which is the contract.  For a sample at float coordinates p, `where` (inside, far, near), A and G are the ramp
 * of wnoise_bounded.h at p: float32, unfused, the same function and so the same bits in both tiers.
 *   nobs == 0        both tiers give the bits of wn_eval3d_curl_bricks / wn_multiband3d_curl_bricks: the call is routed to
 *                    that code and launches no kernel of its own.
 *   WN_GRID_EXACT    and every lattice the separable regime declines (the regime wnoise_bricks.h gives its default tier; an
 *                    empty tile and no active band included): every component has the bits of
 *                    wn_eval3d_curl_bounded_points / wn_multiband3d_curl_bounded_points at the sample's float coordinates,
 *                    times out_scale.  Inside samples are 0.0f * out_scale.
 *   WN_GRID_DEFAULT  in the regime, a separable kernel.  All operations below are separately rounded float32; a = (k+1) % 3
 *                    and b = (k+2) % 3.
 *                      inside  0.0f * out_scale in all three components.
 *                      far     the bits of the default-tier wn_eval3d_curl_bricks / wn_multiband3d_curl_bricks sample, c.
 *                      near    v_k = A*c_k + (G_a*Psi_b - G_b*Psi_a), where c is that same default-tier unbounded sample
 *                              (out_scale and the band factors are already inside it) and Psi_k has the bits of channel 0
 *                              of the default-tier wn_eval3d_grad_bricks / wn_multiband3d_grad_bricks on the tile rolled by
 *                              potential k's offset: by wnoise_brick_fields.h's contract the bits of the default-tier
 *                              wn_eval3d_bricks / wn_multiband3d_bricks on that rolled tile.
 *                    A sample's bits depend only on its lattice index, the lattice, the tile, the bands, the offsets and
 *                    the obstacle list: not on the brick's place in the list, its pair partner, the list length, the
 *                    output alignment or the volume's extent inside boundary bricks.
 *   Tolerance of the default tier against the exact tier and against float64, per component:
 *       A T + V (|G_a| + |G_b|) + dA |c_k| + dG (|Psi_a| + |Psi_b|) + 8 2^-24 (A |c_k| + |G_a Psi_b| + |G_b Psi_a|)
 *   with T the curl bricks' tolerance, 2 G of wnoise_brick_fields.h, V the default-tier value bricks' bound (1e-5 absolute on
 *   every sample, as wnoise_bricks.h gives its default tier), and dA, dG the float32 rounding bounds of the ramp
 *   (zero against the exact tier, whose ramp has the same bits): the derivation of the host twin's float64 comparison
 *   (tests/test_bounded_host.py) with the default tier's T and V in place of the exact evaluators' bounds.
 *
 * Not provided: gradient or value bricks with obstacles; moving obstacles; projected bricks; dense bounded grids; brick edges
 * other than 8.
 */
#ifndef WNOISE_BOUNDED_BRICKS_H
#define WNOISE_BOUNDED_BRICKS_H

#include "wnoise_brick_fields.h"
#include "wnoise_bounded.h"

#ifdef __cplusplus
extern "C" {
#endif

WN_API int wn_eval3d_curl_bounded_bricks(const wn_tile *tile3d, const wn_grid *g, const int32_t *bricks_dev, size_t n,
                                         const int32_t *offsets9_host, const wn_obstacle *obstacles_host, int nobs,
                                         float *out_dev, void *stream);
WN_API int wn_multiband3d_curl_bounded_bricks(const wn_tile *tile3d, const wn_grid *g, const int32_t *bricks_dev, size_t n,
                                              const int32_t *offsets9_host, float s, int first_band, int nbands,
                                              const float *w_host, float var_per_band,
                                              const wn_obstacle *obstacles_host, int nobs, float *out_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* WNOISE_BOUNDED_BRICKS_H */
