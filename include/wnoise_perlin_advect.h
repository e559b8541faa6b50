/* wnoise_perlin_advect.h -- C ABI of fused particle advection through the divergence-free curl noise of Perlin noise
 * potentials (Bridson, Houriham and Nordenstam, "Curl-Noise for Procedural Fluid Flow", 2007), exported by libwnoise_hip.so
 * beside the entry points of wnoise.h; absent from the reference.  The Perlin twin of wnoise_advect.h, whose wn_advect and
 * WN_ADVECT_* it uses, around the velocity fields of wnoise_perlin_curl.h, whose kinds, `depth` and offsets9_host it takes.
 * Conventions as in wnoise.h.
 *
 * A particle is a packed record of three doubles (24 bytes; no alignment beyond a double's) in noise-space coordinates.
 * Positions in, positions out and the trajectory are doubles.  The velocity v(q) at a stage point q is
 *   WN_PERLIN_CURL_NOISE     exactly what wn_perlin_curl_points returns at the double point q;
 *   WN_PERLIN_CURL_TURB,
 *   WN_PERLIN_CURL_FRACTAL   exactly what wn_perlin_curl_points_vec3 returns at (float)q: each component of q is rounded
 *                            to nearest once, on entry to the evaluator -- float points are the only ones those two
 *                            potentials are defined on.  The position itself stays a double.
 * `depth` is read by TURB only; depth == 0 gives v = 0.  One call moves every particle `steps` explicit time steps of size
 * h through the stage velocity
 *     k(q) = gain * v(q) + drift
 * inside ONE kernel launch per wn_perlin_advect_launch_steps(kind, depth, method) steps (csrc/wn_perlin_advect.hip;
 * launches are chained on `stream`): the position and the stage sums stay in registers between steps.  The field does
 * not depend on time and has no boundaries.
 *
 * Arithmetic, which is the contract.  The step is fp64; every product and every sum is rounded on its own (unfused).  The
 * floats of wn_advect are widened to double, which is exact.  Per component:
 *     k(q) = gain * v(q) + drift                one multiply, then one add
 *     h2 = 0.5 * (double)h,  h6 = (double)h / 6.0      both formed once, on the host
 *     WN_ADVECT_EULER     p' = p + h * k(p)
 *     WN_ADVECT_MIDPOINT  k1 = k(p);  p' = p + h * k(p + h2 * k1)
 *     WN_ADVECT_RK4       k1 = k(p), k2 = k(p + h2 * k1), k3 = k(p + h2 * k2), k4 = k(p + h * k3);
 *                         p' = p + h6 * (((k1 + 2.0 * k2) + 2.0 * k3) + k4)
 * A result therefore has the bits of composing wn_perlin_curl_points (NOISE) / wn_perlin_curl_points_vec3 at
 * q.astype(float32) (TURB, FRACTAL) with these operations written out as separately rounded float64 operations (numpy
 * float64 arrays, one operation per statement), and of the host's wnhost_perlin_curl_advect.  The bits do not depend on
 * how the steps are cut into launches.  No position gets special handling: the domain is that of the point entry
 * points, and the same composition defines what follows a non-finite position.
 *
 * Outputs.  xyz_out_dev receives the n positions after `steps` steps, whether or not that step is a snapshot.  It may be
 * xyz_in_dev itself (in place); any other overlap of the two ranges of 3 n doubles is WN_ERR_INVALID.  traj_dev is read
 * only when traj_every >= 1 and must then be non-NULL: steps / traj_every + 1 snapshots, time-major [snapshot][n][3], so
 * that a wave's store of a snapshot is contiguous and every snapshot is itself a point list for wn_perlin_curl_points;
 * snapshot 0 is the input.  Exactly those doubles are written, from any double-aligned pointer.  steps == 0 copies the
 * input.
 * Argument checks, in this order: those of wn_perlin_curl_points_vec3 on kind and depth (`kind` outside 0..2, depth < 0
 * with TURB: WN_ERR_INVALID) and on the perm (NULL, or one of another device); then those of the wavelet call on `a`, with
 * the same messages (WN_ERR_INVALID for a NULL `a`, a method outside 0..2, steps < 0, traj_every < 0, a non-finite h, gain
 * or drift); n == 0 is then WN_OK; then NULL xyz_in_dev or xyz_out_dev, NULL offsets9_host, NULL traj_dev with
 * traj_every >= 1, and the overlap above are WN_ERR_INVALID.  Without a GPU WN_ERR_NO_DEVICE.
 */
#ifndef WNOISE_PERLIN_ADVECT_H
#define WNOISE_PERLIN_ADVECT_H

#include "wnoise_advect.h"
#include "wnoise_perlin_curl.h"

#ifdef __cplusplus
extern "C" {
#endif

WN_API int wn_perlin_curl_advect_points(const wn_perm *perm, const double *xyz_in_dev, size_t n, int kind, int depth,
                                        const int32_t *offsets9_host, const wn_advect *a, double *xyz_out_dev,
                                        double *traj_dev, void *stream);
/* The most steps one kernel launch integrates, >= 1: a call of more steps is a chain of launches.  A launch is bounded by a
 * budget of octave evaluations (kPerlinAdvectOctaveBudget): budget / (stages * octaves), stages 1, 2 or 4 by method,
 * octaves 1 (NOISE), max(depth, 1) (TURB) or 6 (FRACTAL).  An unknown kind or method is counted as the costliest. */
WN_API int wn_perlin_advect_launch_steps(int kind, int depth, int method);

#ifdef __cplusplus
}
#endif
#endif /* WNOISE_PERLIN_ADVECT_H */
