// scalar_eval.h -- host evaluators of the reference's SCALAR members only (one sample per call).
//
// "Scalar class methods stay on the CPU path".  A caller that asks for one sample and needs it before its
// next instruction (the reference's ray tracer: material.h:72 -> texture.h:37-43 / 67-107, 29.6 M calls a render) cannot
// be served by a device faster than the PCIe round trip (1.9 us measured, profiles/r03_scalar_latency.json); the
// reference's own call takes ~0.1 us.  These functions are that call: the reference's arithmetic in the reference's order
// (file:line beside each), compiled with -ffp-contract=off into libwnoise_host.so.  scalar_eval.cpp states none of it
// itself: each function calls the evaluator of csrc/wn_eval.hpp that the HIP kernels call, so host and device share one
// source and return the same bits, those of the reference (tests/test_host_scalar.py, tools/scalar_api_check).  This
// header includes nothing from csrc/ and can be copied next to the reference's sources on its own.
//
// They are not a fallback: nothing that takes more than one sample (points lists, textures' values(), dense grids, tile
// generation) has a host form, and the host classes still throw without a HIP device.  WN_SCALAR_ON_DEVICE=1 in the
// environment sends the scalar members through the resident scalar kernel instead (wn_scalar_*, csrc/wn_mailbox.hip).
#ifndef WN_HOST_SCALAR_EVAL_H
#define WN_HOST_SCALAR_EVAL_H

#include <stddef.h>

#if defined(__GNUC__)
#define WNHOST_API __attribute__((visibility("default")))
#else
#define WNHOST_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

// `coef`: the tile's n^2 / n^3 coefficients, x fastest (WaveletNoise::getNoiseCoefficients()); n == 0 or coef == NULL -> 0.0f
WNHOST_API float wnhost_eval2d(const float *coef, int n, const float p[2]);                                  // WaveletNoise.cpp:111-140
// evaluate2D and its gradient (absent from the reference): returns the value (the bits of wnhost_eval2d), writes d/dx,
// d/dy to grad -- tap weights d_x*w_y, w_x*d_y in evaluate2D's order, unfused: the bits of wn_eval2d_grad_points.
// n == 0 or coef == NULL -> 0 in all three.
WNHOST_API float wnhost_eval2d_grad(const float *coef, int n, const float p[2], float grad[2]);
WNHOST_API float wnhost_eval3d(const float *coef, int n, const float p[3]);                                  // WaveletNoise.cpp:185-215
// evaluate3D and its gradient (absent from the reference): returns the value (the bits of wnhost_eval3d), writes
// d/dx, d/dy, d/dz to grad -- tap weights (d_x*w_y)*w_z, (w_x*d_y)*w_z, (w_x*w_y)*d_z in evaluate3D's order, unfused:
// the bits of wn_eval3d_grad_points.  n == 0 or coef == NULL -> 0 in all four.
WNHOST_API float wnhost_eval3d_grad(const float *coef, int n, const float p[3], float grad[3]);
// The curl of the vector potential (psi0, psi1, psi2), psi_k = evaluate3D of the tile shifted by the whole-cell offset
// offsets9[3k .. 3k+2] = (ox, oy, oz)_k (any integers; include/wnoise.h), absent from the reference: writes
// v = (d psi2/dy - d psi1/dz, d psi0/dz - d psi2/dx, d psi1/dx - d psi0/dy) -- six of wnhost_eval3d_grad's derivative sums
// over the offset coefficients and one subtraction per component: the bits of wn_eval3d_curl_points.
// n == 0 or coef == NULL -> 0 in all three.
WNHOST_API void wnhost_eval3d_curl(const float *coef, int n, const float p[3], const int offsets9[9], float v[3]);
// One particle traced through that curl field (include/wnoise_advect.h, whose wn_advect `a` is: method, steps, h, gain, drift,
// traj_every): p_out receives the position after a->steps steps of wn::advect_step, the step the device kernel runs, around
// wnhost_eval3d_curl -- the bits of wn_eval3d_curl_advect_points.  traj (read only when a->traj_every >= 1; may then not
// be NULL): a->steps / a->traj_every + 1 packed triples, the positions after steps 0, e, 2e, ...  p_out may be p_in.
// n == 0 or coef == NULL: v = 0, pure drift.  Returns 0, or 1 and writes nothing when `a` is one that entry point refuses.
struct wn_advect;
WNHOST_API int wnhost_eval3d_curl_advect(const float *coef, int n, const float p_in[3], const int offsets9[9],
                                         const struct wn_advect *a, float p_out[3], float *traj);
// That curl with solid boundaries (include/wnoise_bounded.h, whose wn_obstacle the list holds; absent from the reference):
// v = A curl Psi + grad A x Psi with the ramp product A of the obstacles near p -- wn::eval3d_curl_bounded_exact, the
// evaluator the device kernels run: the bits of wn_eval3d_curl_bounded_points.  nobs == 0 and a point far from every
// obstacle: the bits of wnhost_eval3d_curl; a point inside one: 0.  n == 0 or coef == NULL: 0 in all three.  Returns 0, or 1
// and writes nothing when the list is one that entry point refuses.  The advect form traces one particle through it as
// wnhost_eval3d_curl_advect does through the unbounded field: the bits of wn_eval3d_curl_bounded_advect_points.
struct wn_obstacle;
WNHOST_API int wnhost_eval3d_curl_bounded(const float *coef, int n, const float p[3], const int offsets9[9],
                                          const struct wn_obstacle *obstacles, int nobs, float v[3]);
WNHOST_API int wnhost_eval3d_curl_bounded_advect(const float *coef, int n, const float p_in[3], const int offsets9[9],
                                                 const struct wn_obstacle *obstacles, int nobs, const struct wn_advect *a,
                                                 float p_out[3], float *traj);
WNHOST_API float wnhost_eval3d_projected(const float *coef, int n, const float p[3], const float normal[3]); // WaveletNoise.cpp:218-265
// evaluate3DProjected and its gradient with respect to p, the normal held fixed (absent from the reference): returns the
// value (the bits of wnhost_eval3d_projected, its 1e-6 cut included), writes the gradient of the uncut sum over the same
// box to grad (include/wnoise.h): the bits of wn_eval3d_projected_grad_points.  n == 0 or coef == NULL -> 0 in all four.
WNHOST_API float wnhost_eval3d_projected_grad(const float *coef, int n, const float p[3], const float normal[3],
                                              float grad[3]);
// WMultibandNoise (Cook & DeRose Appendix 2) at ONE footprint s (absent from the reference; include/wnoise_footprint.h):
// band b runs while t_b = (s + first_band) + b < 0 and enters with the weight w[b] * f_b, f_b = 1 (fade == 0: the paper's
// hard cut) or fminf(1, -t_b) (fade != 0); normal_or_null != NULL makes every band evaluate3DProjected; the sum is
// divided by sqrtf(sum over all nbands of w^2 * var_per_band) when that sum is non-zero.  Returns the value;
// grad_or_null != NULL also receives the gradient with respect to p (the value's bits do not change).  The first host
// evaluator of a multiband function: the bits of wn_multiband3d_footprint_points and its twins, and -- where every
// f_b == 1 -- of wn_multiband3d_points at s.  n == 0, coef == NULL or nbands outside 0..8 -> 0 in every channel.
WNHOST_API float wnhost_multiband3d_footprint(const float *coef, int n, const float p[3], const float *normal_or_null,
                                              float s, int fade, int first_band, int nbands, const float *w,
                                              float var_per_band, float *grad_or_null);
// 2-D WMultibandNoise at ONE footprint s (absent from the reference; include/wnoise_multiband2d.h): the function above on
// a 2-D tile -- bands are evaluate2D at q_b = 2 * p * 2^(first_band+b), the gradient has two components.  The bit
// reference of wn_multiband2d_footprint_points and its _grad_ twin and -- at the call's s with fade == 0 -- of the
// uniform wn_multiband2d_* entry points.  `coef`: n^2 coefficients.  n == 0, coef == NULL or nbands outside 0..8 -> 0 in
// every channel.
WNHOST_API float wnhost_multiband2d_footprint(const float *coef, int n, const float p[2], float s, int fade, int first_band,
                                              int nbands, const float *w, float var_per_band, float *grad_or_null);
// Curl noise on the 2-D tile (absent from the reference; include/wnoise_curl2d.h): v = (d psi/dy, -d psi/dx) of the stream
// function psi = the function above at footprint s with fade == 0 -- v[0] has the bits of its d/dy channel, v[1] those of its
// d/dx channel with the sign flipped: the bits of wn_multiband2d_curl_points.  n == 0, coef == NULL or nbands outside
// 0..8 -> 0 in both.
WNHOST_API void wnhost_multiband2d_curl(const float *coef, int n, const float p[2], float s, int first_band, int nbands,
                                        const float *w, float var_per_band, float v[2]);
// One particle traced through that field (include/wnoise_curl2d.h, whose wn_advect2d `a` is wn_advect with a drift of two
// components): p_out receives the position after a->steps steps of wn::advect_step<., 2>, the step the device kernel runs,
// around wnhost_multiband2d_curl -- the bits of wn_multiband2d_curl_advect_points.  traj (read only when a->traj_every >= 1;
// may then not be NULL): a->steps / a->traj_every + 1 packed pairs, the positions after steps 0, e, 2e, ...  p_out may be
// p_in.  n == 0 or coef == NULL: v = 0, pure drift.  Returns 0, or 1 and writes nothing when nbands or `a` is one that
// entry point refuses.
struct wn_advect2d;
WNHOST_API int wnhost_multiband2d_curl_advect(const float *coef, int n, const float p_in[2], float s, int first_band,
                                              int nbands, const float *w, float var_per_band, const struct wn_advect2d *a,
                                              float p_out[2], float *traj);
// That field with solid boundaries and a background stream (absent from the reference; include/wnoise_bounded2d.h, whose
// wn_obstacle2d the list holds): the ramp of the obstacles fades the stream function psi_t = psi + (ux * py - uy * px)
// (flow = {ux, uy}; NULL: psi alone), v = (d(A psi_t)/dy, -d(A psi_t)/dx) -- zero inside a solid, and without a stream the
// bits of wnhost_multiband2d_curl far from all of them and with nobs == 0: the bits of wn_multiband2d_curl_bounded_points.
// wnhost_multiband2d_curl_bounded_advect traces one particle through it as wnhost_multiband2d_curl_advect does through the
// unbounded field: the bits of wn_multiband2d_curl_bounded_advect_points.  Both return 0, or 1 and write nothing for an
// obstacle list, a stream, nbands or `a` that the entry point refuses.
struct wn_obstacle2d;
WNHOST_API int wnhost_multiband2d_curl_bounded(const float *coef, int n, const float p[2], float s, int first_band, int nbands,
                                               const float *w, float var_per_band, const struct wn_obstacle2d *obstacles,
                                               int nobs, const float *flow2, float v[2]);
WNHOST_API int wnhost_multiband2d_curl_bounded_advect(const float *coef, int n, const float p_in[2], float s, int first_band,
                                                      int nbands, const float *w, float var_per_band,
                                                      const struct wn_obstacle2d *obstacles, int nobs, const float *flow2,
                                                      const struct wn_advect2d *a, float p_out[2], float *traj);
// grey level of wavelet_multiband_texture::value (texture.h; wn_wavelet_multiband_texture_points): the function above
// (normal == NULL) at (float)((double)xyz * scale) and footprint s, through wavelet_texture's grey; coef == NULL: 0.5
WNHOST_API float wnhost_wavelet_multiband_texture_value(const float *coef, int n, double scale, int first_band, int nbands,
                                                        const float *w, float var_per_band, int fade, const float xyz[3],
                                                        float s);
// `perm`: the 512-entry table (perlin.h:34-39)
WNHOST_API double wnhost_perlin(const int *perm, double x, double y, double z);      // perlin.h:42-62
WNHOST_API double wnhost_perlin_fractal(const int *perm, const float q[3]);           // perlin.h:75-90
WNHOST_API double wnhost_perlin_turb(const int *perm, const float q[3], int depth);   // RTOW turb (absent from the reference)
// noise / fractal_noise / turb and their gradients (absent from the reference): each returns the value (the bits of the
// function above) and writes d/dx, d/dy, d/dz to grad -- corner vectors blended over z, then y, then x, plus fade' times the
// value's own differences (include/wnoise.h): the bits of wn_perlin_grad_points / _fractal_grad_points / _turb_grad_points.
// turb: the sign of the accumulated sum multiplies the gradient (+1 where the sum is 0: not differentiable there);
// depth == 0 -> 0 in all four.
WNHOST_API double wnhost_perlin_grad(const int *perm, double x, double y, double z, double grad[3]);
WNHOST_API double wnhost_perlin_fractal_grad(const int *perm, const float q[3], double grad[3]);
WNHOST_API double wnhost_perlin_turb_grad(const int *perm, const float q[3], int depth, double grad[3]);
// turb and fractal_noise with the octave limit taken from ONE footprint s (absent from the reference;
// include/wnoise_perlin_footprint.h): octave i runs while t_i = (s + bias) + i < 0 and enters with the factor f_i = 1
// (fade == 0: a hard cut) or fminf(1, -t_i) (fade != 0).  turb: accum += (2^-i * f_i) * noise, the value fabs(accum), the
// gradient sum_i f_i * grad noise times wnhost_perlin_turb_grad's sign.  fractal: result += noise * (2^-i * f_i) over
// `octaves` octaves, divided -- like sum_i f_i * grad noise -- by the amplitudes of ALL `octaves` octaves.  Each returns the
// value; grad_or_null != NULL also receives the gradient (the value's bits do not change).  The bits of
// wn_perlin_*_footprint_points and their _grad_ twins and -- where every f_i == 1 -- of wnhost_perlin_turb at the sample's
// octave count / of wnhost_perlin_fractal at six of six octaves.  depth / octaves outside 0..16, or no active octave -> 0 in
// every channel.
WNHOST_API double wnhost_perlin_turb_footprint(const int *perm, const float q[3], int depth, float s, float bias, int fade,
                                               double *grad_or_null);
WNHOST_API double wnhost_perlin_fractal_footprint(const int *perm, const float q[3], int octaves, float s, float bias,
                                                  int fade, double *grad_or_null);
// grey level of noise_multiband_texture::value (texture.h; wn_noise_multiband_texture_points): the fractal form above at
// (float)scale * xyz per axis and footprint s, through 0.5 * (1 + n); octaves outside 0..16: 0.5
WNHOST_API float wnhost_noise_multiband_texture_value(const int *perm, double scale, int octaves, float bias, int fade,
                                                      const float xyz[3], float s);
// The curl of three Perlin potentials (absent from the reference; include/wnoise_perlin_curl.h): psi_k is noise / the signed
// turb sum (no fabs) / fractal_noise with the cell index shifted by offsets9[3k .. 3k+2] = (ox, oy, oz)_k (any integers, taken
// & 255); writes v = (d psi2/dy - d psi1/dz, d psi0/dz - d psi2/dx, d psi1/dx - d psi0/dy) -- six of the partial sums the
// gradient functions above form, at the shifted hashes, and one subtraction per component: the bits of
// wn_perlin_curl_points / _points_vec3.  turb: depth == 0 -> 0 in all three.
WNHOST_API void wnhost_perlin_curl(const int *perm, double x, double y, double z, const int offsets9[9], double v[3]);
WNHOST_API void wnhost_perlin_turb_curl(const int *perm, const float q[3], int depth, const int offsets9[9], double v[3]);
WNHOST_API void wnhost_perlin_fractal_curl(const int *perm, const float q[3], const int offsets9[9], double v[3]);
// One particle traced through one of those curl fields (include/wnoise_perlin_advect.h; `kind`: WN_PERLIN_CURL_NOISE / _TURB /
// _FRACTAL of include/wnoise_perlin_curl.h, `depth` read by TURB only): p_out receives the position after a->steps steps of
// wn::advect_step in double, the step the device kernel runs, around wnhost_perlin_curl at the double stage point (NOISE) or
// wnhost_perlin_turb_curl / _fractal_curl at the stage point rounded to float (TURB, FRACTAL) -- the bits of
// wn_perlin_curl_advect_points.  traj (read only when a->traj_every >= 1; may then not be NULL): a->steps / a->traj_every + 1
// packed triples [snapshot][3], the positions after steps 0, e, 2e, ...  p_out may be p_in.  Returns 0, or 1 (WN_ERR_INVALID)
// and writes nothing when kind, depth or `a` is one that entry point refuses.
WNHOST_API int wnhost_perlin_curl_advect(const int *perm, int kind, int depth, const double p_in[3], const int offsets9[9],
                                         const struct wn_advect *a, double p_out[3], double *traj);
// Those curl fields with solid boundaries (absent from the reference; include/wnoise_perlin_bounded.h, whose wn_obstacle list
// is wnoise_bounded.h's).  The potential values Psi = (psi0, psi1, psi2) on the shifted cells: noise / turb's accumulated sum
// before its fabs / fractal_noise -- with all nine offsets 0 the bits of wnhost_perlin, (up to the sign) wnhost_perlin_turb
// and wnhost_perlin_fractal: the bits of wn_perlin_curl_potential_points_f64 / _points_vec3.
WNHOST_API void wnhost_perlin_curl_potential(const int *perm, double x, double y, double z, const int offsets9[9], double psi[3]);
WNHOST_API void wnhost_perlin_turb_curl_potential(const int *perm, const float q[3], int depth, const int offsets9[9],
                                                  double psi[3]);
WNHOST_API void wnhost_perlin_fractal_curl_potential(const int *perm, const float q[3], const int offsets9[9], double psi[3]);
// The bounded velocity v = A curl Psi + grad A x Psi at p: NOISE evaluates the ramp and the field at the double point p, TURB
// and FRACTAL at (float)p (the ramp at that float widened to double) -- zero inside a solid, the bits of wnhost_perlin_curl /
// _turb_curl / _fractal_curl far from all of them and with nobs == 0: the bits of wn_perlin_curl_bounded_points_f64 /
// _points_vec3.  wnhost_perlin_curl_bounded_advect traces one particle through it as wnhost_perlin_curl_advect does through
// the unbounded field: the bits of wn_perlin_curl_bounded_advect_points_f64.  Both return 0, or 1 and write nothing for a kind,
// depth, obstacle list or `a` that the entry point refuses.
WNHOST_API int wnhost_perlin_curl_bounded(const int *perm, int kind, int depth, const double p[3], const int offsets9[9],
                                          const struct wn_obstacle *obstacles, int nobs, double v[3]);
WNHOST_API int wnhost_perlin_curl_bounded_advect(const int *perm, int kind, int depth, const double p_in[3],
                                                 const int offsets9[9], const struct wn_obstacle *obstacles, int nobs,
                                                 const struct wn_advect *a, double p_out[3], double *traj);
// grey level of texture::value (texture.h); use_3d = 0: the 2-D tile and branch; coef == NULL: the no-tile grey
WNHOST_API float wnhost_wavelet_texture_value(const float *coef, int n, int use_3d, double scale, int octave,
                                              const float xyz[3]);                    // texture.h:67-107
WNHOST_API float wnhost_noise_texture_value(const int *perm, double scale, int octave, const float xyz[3]); // texture.h:37-43
// 1 when WN_SCALAR_ON_DEVICE is set (read once): the classes' scalar members then use the resident scalar kernel
WNHOST_API int wnhost_scalar_on_device(void);

#ifdef __cplusplus
}
#endif
#endif
