/* wnoise_perlin_curl.h -- C ABI of the divergence-free curl noise from Perlin noise potentials (Bridson, Houriham and
 * Nordenstam, "Curl-Noise for Procedural Fluid Flow", 2007), exported by libwnoise_hip.so beside the entry points of
 * wnoise.h; absent from the reference.  Conventions as in wnoise.h, which this header includes.
 *
 * The vector potential is Psi = (psi0, psi1, psi2); psi_k is the Perlin potential evaluated with the LATTICE INDEX
 * shifted by a whole-cell offset o_k = (ox, oy, oz)_k: where perlin::noise forms X = (int)floor(x) & 255 (likewise Y, Z),
 * psi_k hashes the cell ((X + ox_k) & 255, (Y + oy_k) & 255, (Z + oz_k) & 255).  The fractional parts, fade and fade' are
 * unchanged, so in exact arithmetic psi_k(p) = noise(p + o_k).
 * `offsets9_host`: nine int32 on the host, the (x, y, z) triples of psi0, psi1, psi2; any integers (negative ones and
 * ones >= 256 included), reduced mod 256 (two's complement & 255); equal offsets are allowed.  The velocity is
 *     v = (d psi2/dy - d psi1/dz,  d psi0/dz - d psi2/dx,  d psi1/dx - d psi0/dy)
 * Inside a cell every psi_k is a polynomial, so its mixed partials commute and div v = 0; v is continuous across cell
 * faces because the gradient is.
 *
 * Kinds (the numbers the kernels use):
 *   WN_PERLIN_CURL_NOISE    psi_k = perlin::noise on the shifted cells.
 *   WN_PERLIN_CURL_TURB     psi_k = sum_{i<depth} 2^-i noise_k(2^i p) on the float point that doubles per octave: turb's
 *                           accumulated sum BEFORE fabs (|.| is not differentiable, and the curl of |S| is not
 *                           divergence-free where S = 0).  The offsets act on every octave's own cell index and are the
 *                           same in every octave.  Each partial is the plain sum of the octaves' noise partials in octave
 *                           order (the chain factor 2^-i * 2^i is exactly 1).  depth == 0: 0 in all three components.
 *   WN_PERLIN_CURL_FRACTAL  psi_k = fractal_noise on the shifted cells (six octaves, float point times a double
 *                           frequency); each partial is (sum_i partial_i) / max_value.
 * `depth` is read by TURB only.
 *
 * Arithmetic (fp64, unfused): floor, the fractional parts, fade and fade' are formed once per point and octave, the
 * hashes once per potential.  Each of the six partials that enter v is the sum that the gradient entry points of wnoise.h
 * form for that channel (wn_perlin_grad_points; wn_perlin_turb_grad_points without its sign; wn_perlin_fractal_grad_points)
 * -- corner vectors blended over z, then y, then x, plus fade' times the value's own differences -- evaluated at the
 * shifted hashes; each component is then ONE fp64 subtraction.  For NOISE a component therefore has the bits of the
 * subtraction of two channels of wn_perlin_grad_points run at p + o_k, wherever that addition is exact.  The value and the
 * unused third partial of each potential are not computed.
 *
 * Points: `n` packed records {vx, vy, vz} of three doubles (24 bytes; no alignment beyond a double's); every component has
 * the bits of the host evaluators (wnhost_perlin_curl, wnhost_perlin_turb_curl, wnhost_perlin_fractal_curl).
 * Grids: three consecutive float volumes -- vx, vy, vz -- each in wn_perlin_grid's layout; every sample is
 * (float)component * out_scale; derivatives are taken with respect to the sample's noise-space coordinate; under
 * WN_Z_CONST the z-derivatives are taken at z_const.  One tier: `flags` is accepted and ignored.  A sample has the bits of
 * (float) of the point entry point at the lattice's float coordinates, times out_scale; they do not depend on how the
 * volume is cut into z-slabs.
 * Argument checks as the Perlin gradient entry points: `kind` outside 0..2 and depth < 0 with TURB are WN_ERR_INVALID; a
 * perm is used on its own device; n == 0 or an empty lattice is WN_OK; NULL perm, points, out or offsets9_host is
 * WN_ERR_INVALID; without a GPU WN_ERR_NO_DEVICE.
 */
#ifndef WNOISE_PERLIN_CURL_H
#define WNOISE_PERLIN_CURL_H

#include "wnoise.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WN_PERLIN_CURL_NOISE   0
#define WN_PERLIN_CURL_TURB    1
#define WN_PERLIN_CURL_FRACTAL 2

WN_API int wn_perlin_curl_points(const wn_perm *perm, const double *xyz_dev, size_t n,
                                 const int32_t *offsets9_host, double *out3_dev, void *stream);      /* noise(double,double,double) */
WN_API int wn_perlin_curl_points_vec3(const wn_perm *perm, const float *xyz_dev, size_t n, int kind, int depth,
                                      const int32_t *offsets9_host, double *out3_dev, void *stream); /* float vec3 points */
WN_API int wn_perlin_curl_grid(const wn_perm *perm, const wn_grid *g, int kind, int depth,
                               const int32_t *offsets9_host, float *out_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* WNOISE_PERLIN_CURL_H */
