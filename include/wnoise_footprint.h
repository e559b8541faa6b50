/* wnoise_footprint.h -- C ABI of WMultibandNoise (Cook & DeRose, "Wavelet Noise", Appendix 2) with the band limit taken
 * from a footprint PER SAMPLE, exported by libwnoise_hip.so beside the entry points of wnoise.h; absent from the reference.
 * Conventions as in wnoise.h, which this header includes.
 *
 * The paper's WMultibandNoise(p, s, normal, firstBand, nbands, w) stops at the first band with s + firstBand + b >= 0,
 * s = log2 of the sample's footprint: a renderer drops the bands a sample cannot carry.  wn_multiband3d_points and its
 * twins take one s for the whole call; the entry points below take `s_dev`, n floats on the device (a float's
 * alignment), one per point.
 *
 * For point i with footprint s_i and band b in 0 .. nbands-1:
 *   t_b = (s_i + (float)first_band) + (float)b, in float and in this association (the expression the uniform entry
 *         points evaluate for their s).
 *   Band b is active iff t_b < 0 and every earlier band is active (the paper's loop).  A NaN or +inf s_i makes no band
 *         active, -inf all of them.
 *   fade == 0: the paper's hard cut, f_b = 1.0f.
 *   fade != 0: f_b = fminf(1.0f, -t_b): the finest surviving band fades in linearly over one octave of footprint instead
 *         of popping.
 *   With the one float product wb = w[b] * f_b the value adds wb * e_b and the gradient
 *         (wb * (2.0f * 2^(first_band+b))) * grad e_b, e_b = evaluate3D (the projected entry points: evaluate3DProjected)
 *         at q_b = 2 * p * 2^(first_band+b).  The fade does not depend on p: the gradient is that of the faded sum.
 *   Band order, the unfused float arithmetic and the division are those of wn_multiband3d_points:
 *         out_div = sqrtf(sum over ALL nbands of w^2 * var_per_band), weights unfaded, applied when that sum is non-zero.
 *   No active band gives 0 in every channel.
 * So where f_b == 1 for every active band -- every point with fade == 0; with fade, integer-valued s_i -- a point has the
 * bits of the uniform call with s = s_i.  A result depends neither on the other points of the list nor on its length.
 * Every channel has the bits of the host evaluator wnhost_multiband3d_footprint (host/scalar_eval.h).
 *
 * The gradient entry points write float4 records {value, d/dx, d/dy, d/dz}; out4_dev must be 16-byte aligned, else
 * WN_ERR_INVALID.  `one_normal` != 0: normals_dev holds ONE normal for all points, else one per point.
 *
 * wn_wavelet_multiband_texture_points: per axis pos = (float)((double)p * scale) (texture.h:71-75 without the octave
 * multiply); n = WMultibandNoise(pos, s_i, ...) as above, promoted to double; grey = 0.5 * (1 + clamp(n / 4, -1, 1)), the
 * grey level of wn_wavelet_texture_points.  s_dev is taken as given: the footprint in noise space, after `scale`.
 * active_dev as in wn_wavelet_texture_points: NULL, or one byte per point; inactive points are neither evaluated nor
 * written.  An empty tile gives 0.5.
 *
 * Argument checks as wn_multiband3d_points: a NULL tile, points, s, out (normals; w_host with nbands > 0) pointer and
 * nbands outside 0..8 are WN_ERR_INVALID; n == 0 is WN_OK; a 2-D tile is refused; an empty tile gives 0; a tile is used
 * on its own device; without a GPU WN_ERR_NO_DEVICE.  Exactly the n records (with a mask: the active ones) are written.
 */
#ifndef WNOISE_FOOTPRINT_H
#define WNOISE_FOOTPRINT_H

#include "wnoise.h"

#ifdef __cplusplus
extern "C" {
#endif

WN_API int wn_multiband3d_footprint_points(const wn_tile *tile3d, const float *xyz_dev, const float *s_dev, size_t n,
                                           int first_band, int nbands, const float *w_host, float var_per_band,
                                           int fade, float *out_dev, void *stream);
WN_API int wn_multiband3d_projected_footprint_points(const wn_tile *tile3d, const float *xyz_dev,
                                                     const float *normals_dev, int one_normal, const float *s_dev,
                                                     size_t n, int first_band, int nbands, const float *w_host,
                                                     float var_per_band, int fade, float *out_dev, void *stream);
WN_API int wn_multiband3d_footprint_grad_points(const wn_tile *tile3d, const float *xyz_dev, const float *s_dev, size_t n,
                                                int first_band, int nbands, const float *w_host, float var_per_band,
                                                int fade, float *out4_dev, void *stream);
WN_API int wn_multiband3d_projected_footprint_grad_points(const wn_tile *tile3d, const float *xyz_dev,
                                                          const float *normals_dev, int one_normal, const float *s_dev,
                                                          size_t n, int first_band, int nbands, const float *w_host,
                                                          float var_per_band, int fade, float *out4_dev, void *stream);
WN_API int wn_wavelet_multiband_texture_points(const wn_tile *tile3d, double scale, int first_band, int nbands,
                                               const float *w_host, float var_per_band, int fade, const float *xyz_dev,
                                               const float *s_dev, const uint8_t *active_dev, size_t n, float *grey_dev,
                                               void *stream);

#ifdef __cplusplus
}
#endif
#endif /* WNOISE_FOOTPRINT_H */
