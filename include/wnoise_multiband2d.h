/* wnoise_multiband2d.h -- C ABI of WMultibandNoise (Cook & DeRose, "Wavelet Noise", Appendix 2) on a 2-D tile: fused band
 * sums on dense grids and point lists, their analytic gradients, and the band limit taken from a footprint per point;
 * exported by libwnoise_hip.so beside the entry points of wnoise.h; absent from the reference.  Conventions as in
 * wnoise.h, which this header includes.
 *
 * For a 2-D point p, a footprint s and band b in 0 .. nbands-1 (nbands in 0 .. 8):
 *   t_b = (s + (float)first_band) + (float)b, in float and in this association.
 *   Band b is active iff t_b < 0 and every earlier band is active (the paper's loop).  A NaN or +inf s makes no band
 *         active, -inf all of them.
 *   fade == 0 (and every uniform-s entry point): the paper's hard cut, f_b = 1.0f.
 *   fade != 0: f_b = fminf(1.0f, -t_b): the finest surviving band fades in linearly over one octave of footprint.
 *   With the one float product wb = w[b] * f_b the value adds wb * evaluate2D(q_b) and the gradient with respect to p
 *         (wb * (2.0f * 2^(first_band+b))) * grad evaluate2D(q_b), q_b = {2.0f * p[0] * 2^(first_band+b),
 *         2.0f * p[1] * 2^(first_band+b)}.
 *   Band order and the unfused float arithmetic are those of wn_multiband3d_footprint_points:
 *         out_div = sqrtf(sum over ALL nbands of w^2 * var_per_band), weights unfaded, applied when that sum is non-zero.
 *   No active band gives 0 in every channel; so does an empty tile.
 * var_per_band comes from the caller; the reference's 2-D constant is 0.19686 (experient/main.cpp:16, texture.h:98).
 * The uniform-s entry points are the footprint function at the call's s with fade 0: a footprint point whose active bands
 * all have f_b == 1 has the bits of the uniform call at its s.  Every channel of every entry point has the bits of the
 * host evaluator wnhost_multiband2d_footprint (host/scalar_eval.h); a result depends neither on the other samples of the
 * call nor on their number.
 *
 * Grids follow wn_multiband3d_grid: p is the lattice coordinate ((i / den) * base_range) * octave_scale * post_scale of
 * sample (x, y) on both axes (callers use octave_scale = post_scale = 1); out_scale multiplies every channel last; z0, z1,
 * z_mode and z_const are ignored; flags is accepted and ignored (one tier, bit-exact).  wn_multiband2d_grid writes one
 * plane of nx * ny floats in wn_eval2d_grid's layout, wn_multiband2d_grad_grid three consecutive planes: value, d/dx, d/dy.
 * The point entry points write n floats, their _grad_ twins n records {value, d/dx, d/dy} of 3 floats, as
 * wn_eval2d_grad_points.  xy_dev: n interleaved (x, y) pairs; s_dev: n floats.
 *
 * Placement as in wnoise.h: pointers need only a float's alignment, exactly the output is written, and results do not
 * depend on alignment.
 *
 * Argument checks as wn_multiband3d_points: a NULL tile, points, s, out (w_host with nbands > 0) pointer and nbands
 * outside 0..8 are WN_ERR_INVALID; n == 0 (an empty lattice) is WN_OK; a 3-D tile is refused; a tile is used on its own
 * device; without a GPU WN_ERR_NO_DEVICE.
 */
#ifndef WNOISE_MULTIBAND2D_H
#define WNOISE_MULTIBAND2D_H

#include "wnoise.h"

#ifdef __cplusplus
extern "C" {
#endif

WN_API int wn_multiband2d_grid(const wn_tile *tile2d, const wn_grid *g, float s, int first_band, int nbands,
                               const float *w_host, float var_per_band, float *out_dev, void *stream);
WN_API int wn_multiband2d_grad_grid(const wn_tile *tile2d, const wn_grid *g, float s, int first_band, int nbands,
                                    const float *w_host, float var_per_band, float *out_dev, void *stream);
WN_API int wn_multiband2d_points(const wn_tile *tile2d, const float *xy_dev, size_t n, float s, int first_band, int nbands,
                                 const float *w_host, float var_per_band, float *out_dev, void *stream);
WN_API int wn_multiband2d_grad_points(const wn_tile *tile2d, const float *xy_dev, size_t n, float s, int first_band,
                                      int nbands, const float *w_host, float var_per_band, float *out3_dev, void *stream);
WN_API int wn_multiband2d_footprint_points(const wn_tile *tile2d, const float *xy_dev, const float *s_dev, size_t n,
                                           int first_band, int nbands, const float *w_host, float var_per_band, int fade,
                                           float *out_dev, void *stream);
WN_API int wn_multiband2d_footprint_grad_points(const wn_tile *tile2d, const float *xy_dev, const float *s_dev, size_t n,
                                                int first_band, int nbands, const float *w_host, float var_per_band,
                                                int fade, float *out3_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* WNOISE_MULTIBAND2D_H */
