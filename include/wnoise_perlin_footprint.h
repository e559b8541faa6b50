/* wnoise_perlin_footprint.h -- C ABI of Perlin turb and fractal_noise with the octave limit taken from a footprint PER
 * SAMPLE, exported by libwnoise_hip.so beside the entry points of wnoise.h; absent from the reference.  The Perlin twin of
 * wnoise_footprint.h: clamping the octave sum by the filter width is the classical way to antialias Perlin noise, and what
 * Cook & DeRose compare wavelet noise against.  Conventions as in wnoise.h, which this header includes.
 *
 * `s_dev` holds n floats on the device (a float's alignment), one per point: s_i = log2 of the sample's footprint in the
 * noise space of p.  For point i and octave j in 0 .. octaves-1 (turb: depth-1):
 *   t_j = (s_i + bias) + (float)j, in float and in this association.
 *   Octave j is active iff t_j < 0; t_j does not decrease with j, so the first octave that fails ends the loop.  A NaN or
 *         +inf s_i makes no octave active, -inf all of them.
 *   fade == 0: a hard cut, f_j = 1.0f.
 *   fade != 0: f_j = fminf(1.0f, -t_j): the finest surviving octave fades in linearly over one octave of footprint.
 *   Octave j has cells of size 2^-j.  bias = 0 cuts an octave when the footprint reaches one cell, bias = -1 at two cells:
 *         the rule wn_multiband3d_footprint_points (wnoise_footprint.h) applies to its bands.
 *
 * turb (wn_perlin_turb_points' arithmetic: the float point doubles per octave, weight halves):
 *         accum += (weight * (double)f_j) * noise(p_j); value = fabs(accum).
 *         Gradient: g += (double)f_j * grad noise(p_j) in octave order, times -1 where the value's own accum is negative
 *         (wn_perlin_turb_grad_points' sign rule).  No active octave: +0 in all four channels.
 * fractal (wn_perlin_fractal_points' arithmetic, float point times double frequency, for `octaves` octaves):
 *         result += noise(p * frequency) * (amplitude * (double)f_j); value = result / max_value, where max_value is the
 *         sum of the amplitudes of ALL `octaves` octaves, however many run: dropping an octave drops its energy, nothing is
 *         renormalised.  Gradient: (sum_j f_j * grad noise) / max_value.  octaves == 0: 0 in every channel, no division.
 * The fade does not depend on p: the gradients are those of the faded sums.
 *
 * Where f_j == 1 for every active octave -- every sample with fade == 0; with fade, every integer-valued s_i + bias -- the
 * products with f_j are exact: a turb sample with k active octaves has the bits of wn_perlin_turb_points /
 * wn_perlin_turb_grad_points at depth = k, and a fractal sample with octaves = 6 and all six active those of
 * wn_perlin_fractal_points / wn_perlin_fractal_grad_points.  A result depends neither on the other points of the list nor
 * on its length.  Every channel has the bits of the host evaluators wnhost_perlin_turb_footprint /
 * wnhost_perlin_fractal_footprint / wnhost_noise_multiband_texture_value (host/scalar_eval.h).
 *
 * The value entry points write one double per point (a double's alignment).  The gradient entry points write records of
 * four doubles {value, d/dx, d/dy, d/dz}; out4_dev must be 16-byte aligned as for wn_perlin_turb_grad_points, else
 * WN_ERR_INVALID.
 *
 * wn_noise_multiband_texture_points: per axis pos = (float)scale * p in float (noise_texture::value's scaling without its
 * octave factor); n = the fractal form above at pos and s_i; grey = (float)(0.5 * (1.0 + n)).  s_dev is taken as given:
 * the footprint in noise space, after `scale`.  active_dev as in wn_noise_texture_points: NULL, or one byte per point;
 * inactive points are neither evaluated nor written.
 *
 * Argument checks as the Perlin point entry points: a NULL perm is WN_ERR_INVALID and a perm is used on its own device;
 * depth / octaves outside 0..16 is WN_ERR_INVALID; n == 0 is WN_OK; a NULL points, s_dev or out pointer is
 * WN_ERR_INVALID; without a GPU WN_ERR_NO_DEVICE.  Exactly the n records (with a mask: the active ones) are written.
 */
#ifndef WNOISE_PERLIN_FOOTPRINT_H
#define WNOISE_PERLIN_FOOTPRINT_H

#include "wnoise.h"

#ifdef __cplusplus
extern "C" {
#endif

WN_API int wn_perlin_turb_footprint_points(const wn_perm *perm, const float *xyz_dev, const float *s_dev, size_t n,
                                           int depth, float bias, int fade, double *out_dev, void *stream);
WN_API int wn_perlin_fractal_footprint_points(const wn_perm *perm, const float *xyz_dev, const float *s_dev, size_t n,
                                              int octaves, float bias, int fade, double *out_dev, void *stream);
WN_API int wn_perlin_turb_footprint_grad_points(const wn_perm *perm, const float *xyz_dev, const float *s_dev, size_t n,
                                                int depth, float bias, int fade, double *out4_dev, void *stream);
WN_API int wn_perlin_fractal_footprint_grad_points(const wn_perm *perm, const float *xyz_dev, const float *s_dev, size_t n,
                                                   int octaves, float bias, int fade, double *out4_dev, void *stream);
WN_API int wn_noise_multiband_texture_points(const wn_perm *perm, double scale, int octaves, float bias, int fade,
                                             const float *xyz_dev, const float *s_dev, const uint8_t *active_dev, size_t n,
                                             float *grey_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* WNOISE_PERLIN_FOOTPRINT_H */
