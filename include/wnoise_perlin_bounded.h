/* wnoise_perlin_bounded.h -- C ABI of solid boundaries for the curl noise of Perlin noise potentials and for particles moved
 * through it (Bridson, Houriham and Nordenstam, "Curl-Noise for Procedural Fluid Flow", 2007, section 2.4), exported by
 * libwnoise_hip.so beside the entry points of wnoise.h; absent from the reference.  The Perlin twin of wnoise_bounded.h, whose
 * wn_obstacle, WN_OBSTACLE_* and WN_MAX_OBSTACLES it uses, around the fields of wnoise_perlin_curl.h and the time step of
 * wnoise_perlin_advect.h, both of which it includes.  Conventions as in wnoise.h.
 *
 * The vector potential Psi = (psi0, psi1, psi2) of wn_perlin_curl_points / _points_vec3 is faded to zero towards every
 * obstacle by a smooth ramp A of the distance to it, and the velocity is the curl of the faded potential,
 *     v = curl(A Psi) = A (curl Psi) + grad A x Psi:
 * exactly divergence-free, with no normal component on an obstacle's surface.  Obstacles are spheres, containers and
 * half-spaces in the noise-space coordinates of the points; overlapping ramps multiply.  INSIDE, FAR and NEAR are defined as
 * in wnoise_bounded.h.
 *
 * Arithmetic, which is the contract.  Everything is fp64 and unfused: every product, sum, division and square root is
 * rounded on its own.
 *   Potential values, on the shifted cells (offsets9_host as in wnoise_perlin_curl.h).
 *       WN_PERLIN_CURL_NOISE    psi_k has the bits of perlin::noise evaluated with potential k's shifted hashes (where
 *                               p + o_k is exact, the bits of wn_perlin_points at p + o_k).
 *       WN_PERLIN_CURL_TURB     psi_k is turb's accumulated sum, accum += weight * noise_k, weight halving and the float
 *                               point doubling per octave, BEFORE the fabs, the offsets applied in every octave.
 *                               depth == 0: psi = 0.
 *       WN_PERLIN_CURL_FRACTAL  psi_k is fractal_noise's result / max_value, result += noise_k * amplitude over six octaves.
 *     With all nine offsets 0 the three are equal, and equal noise / (up to the sign) turb / fractal_noise.
 *   Ramp.  wnoise_bounded.h's, line by line, with every operation in double: an obstacle's c, r and d0 are widened from
 *     float, which is exact; sqrt and / are IEEE double; the constants 1.875, -1.25 and 0.375 are exact; the obstacle order,
 *     the d <= 0 (INSIDE), d >= d0 (skipped; all skipped: FAR) rules, G = G * alpha + (A * dalpha) * nrm and A = A * alpha are
 *     unchanged.  The ramp is evaluated at the point the evaluator receives: the double point
 *     (wn_perlin_curl_bounded_points_f64), the float point widened to double (_points_f32), and under advection the double stage point q (NOISE) or (float)q
 *     widened (TURB, FRACTAL) -- the rule wnoise_perlin_advect.h states for the field itself.
 *   Velocity.  INSIDE: (0, 0, 0).  FAR, or nobs == 0: exactly the bits of wn_perlin_curl_points / _points_vec3; Psi is not
 *     needed.  NEAR: with c the bits of wn_perlin_curl_points / _points_vec3 and psi those of the potential entry points,
 *         v0 = A*c0 + (G1*psi2 - G2*psi1),  v1 = A*c1 + (G2*psi0 - G0*psi2),  v2 = A*c2 + (G0*psi1 - G1*psi0).
 *   Advection.  The step, the snapshots, the in-place rule, the argument order, the chaining of launches and "exactly those
 *     doubles are written, from any double-aligned pointer" are wnoise_perlin_advect.h's, with the stage velocity
 *     k(q) = gain * v(q) + drift of this bounded v: the result is the composition of wn_perlin_curl_bounded_points_f64
 *     (NOISE, at q) / _points_f32 (TURB, FRACTAL, at q.astype(float32)) with that header's separately rounded float64 operations.  A
 *     particle inside a solid moves by drift alone.  The bits do not depend on how a call is cut into launches;
 *     wn_perlin_bounded_advect_launch_steps() is the cap.
 * A result has the bits of the host's wnhost_perlin_*curl_potential / wnhost_perlin_curl_bounded / _bounded_advect.
 *
 * Argument checks: first those of the unbounded entry point (wn_perlin_curl_points, _points_vec3, wn_perlin_curl_advect_points)
 * on kind, depth and perm, in its order; then the obstacle checks of wnoise_bounded.h, each WN_ERR_INVALID, also with n == 0
 * (nobs == 0 with a NULL list is valid); then the rest of the unbounded entry point's (`a`; n == 0 is WN_OK; the pointers).
 *
 * Names: the suffix says what the points are, _f64 for packed doubles (NOISE potentials only, as wn_perlin_curl_points) and
 * _f32 for packed floats with `kind` and `depth` (as wn_perlin_curl_points_vec3).
 *
 * Not provided: dense grids (brick lists: wnoise_perlin_bounded_bricks.h); a background stream; moving obstacles and potentials that change with time;
 * Bridson's variant that keeps the normal component of Psi.
 */
#ifndef WNOISE_PERLIN_BOUNDED_H
#define WNOISE_PERLIN_BOUNDED_H

#include "wnoise_bounded.h"
#include "wnoise_perlin_advect.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the potential values Psi = (psi0, psi1, psi2): n packed records of three doubles */
WN_API int wn_perlin_curl_potential_points_f64(const wn_perm *perm, const double *xyz_dev, size_t n,
                                               const int32_t *offsets9_host, double *out3_dev, void *stream);
WN_API int wn_perlin_curl_potential_points_f32(const wn_perm *perm, const float *xyz_dev, size_t n, int kind, int depth,
                                               const int32_t *offsets9_host, double *out3_dev, void *stream);
/* the bounded velocity: n packed records {vx, vy, vz} of doubles */
WN_API int wn_perlin_curl_bounded_points_f64(const wn_perm *perm, const double *xyz_dev, size_t n, const int32_t *offsets9_host,
                                             const wn_obstacle *obstacles_host, int nobs, double *out3_dev, void *stream);
WN_API int wn_perlin_curl_bounded_points_f32(const wn_perm *perm, const float *xyz_dev, size_t n, int kind, int depth,
                                             const int32_t *offsets9_host, const wn_obstacle *obstacles_host, int nobs,
                                             double *out3_dev, void *stream);
WN_API int wn_perlin_curl_bounded_advect_points_f64(const wn_perm *perm, const double *xyz_in_dev, size_t n, int kind,
                                                    int depth, const int32_t *offsets9_host,
                                                    const wn_obstacle *obstacles_host, int nobs, const wn_advect *a,
                                                    double *xyz_out_dev, double *traj_dev, void *stream);
/* The most steps one kernel launch integrates, >= 1.  The budget of wn_perlin_advect_launch_steps counts obstacles too:
 * budget / (stages * (octaves + ceil(kappa * nobs))), kappa the cost of one obstacle's ramp in octave evaluations
 * (csrc/wn_perlin_bounded.hip).  nobs == 0: wn_perlin_advect_launch_steps(kind, depth, method); an nobs outside
 * 0..WN_MAX_OBSTACLES is counted as WN_MAX_OBSTACLES. */
WN_API int wn_perlin_bounded_advect_launch_steps(int kind, int depth, int method, int nobs);

#ifdef __cplusplus
}
#endif
#endif /* WNOISE_PERLIN_BOUNDED_H */
