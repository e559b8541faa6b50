/* wnoise_advect.h -- C ABI of fused particle advection through the divergence-free curl noise of 3-D wavelet noise
 * potentials (Bridson, Houriham and Nordenstam, "Curl-Noise for Procedural Fluid Flow", 2007), exported by libwnoise_hip.so
 * beside the entry points of wnoise.h; absent from the reference.  Conventions as in wnoise.h, which this header includes.
 *
 * A particle is a packed float triple (no alignment beyond a float's) in noise-space coordinates: the values
 * wn_eval3d_curl_points takes, or the lattice coordinate p of wn_multiband3d_curl_points.  The velocity v(q) is exactly what
 * that entry point returns at q -- tile, offsets9_host and bands are handled the same way; an empty tile, or no active
 * band, gives v = 0.  One call moves every particle `steps` explicit time steps of size h through the stage velocity
 *     k(q) = gain * v(q) + drift
 * inside ONE kernel launch per kAdvectLaunchSteps steps (csrc/wn_wavelet_advect.hip; launches are chained on `stream`):
 * the position and the stage sums stay in registers between steps.  The field does not depend on time; solid
 * boundaries (Bridson's distance ramp) are served by wnoise_bounded.h, Perlin potentials by wnoise_perlin_advect.h.
 *
 * Arithmetic, which is the contract.  Everything is float32; every product and every sum is rounded on its own (unfused).
 * Per component:
 *     k(q) = gain * v(q) + drift                one multiply, then one add
 *     h2 = 0.5f * h,  h6 = h / 6.0f             both formed once, on the host
 *     WN_ADVECT_EULER     p' = p + h * k(p)
 *     WN_ADVECT_MIDPOINT  k1 = k(p);  p' = p + h * k(p + h2 * k1)
 *     WN_ADVECT_RK4       k1 = k(p), k2 = k(p + h2 * k1), k3 = k(p + h2 * k2), k4 = k(p + h * k3);
 *                         p' = p + h6 * (((k1 + 2.0f * k2) + 2.0f * k3) + k4)
 * A result therefore has the bits of composing wn_eval3d_curl_points / wn_multiband3d_curl_points with these operations
 * written out as separately rounded float32 operations (numpy float32 arrays, one operation per statement), and of the
 * host's wnhost_eval3d_curl_advect.  The bits do not depend on how the steps are cut into launches.  A particle that
 * reaches a non-finite position gets no special handling: the same composition defines what follows.
 *
 * wn_advect (8 x 4 bytes):
 *   method       WN_ADVECT_EULER, WN_ADVECT_MIDPOINT or WN_ADVECT_RK4
 *   steps        >= 0; 0 copies the input
 *   h            the step, any finite value; a negative one traces backwards
 *   gain, drift  finite
 *   traj_every   0: no trajectory.  e >= 1: a snapshot of every position after steps 0, e, 2e, ... <= steps.
 *
 * Outputs.  xyz_out_dev receives the n positions after `steps` steps, whether or not that step is a snapshot.  It may be
 * xyz_in_dev itself (in place); any other overlap of the two ranges of 3 n floats is WN_ERR_INVALID.  traj_dev is read
 * only when traj_every >= 1 and must then be non-NULL: steps / traj_every + 1 snapshots, time-major [snapshot][n][3], so
 * that a wave's store of a snapshot is contiguous and every snapshot is itself a point list for any other entry point;
 * snapshot 0 is the input.  Exactly those floats are written, from any float-aligned pointer.
 * Argument checks as the curl point entry points (a NULL tile, a 2-D tile, a tile of another device, NULL offsets9_host,
 * the multiband entry point's band checks; NULL xyz_in_dev or xyz_out_dev with n > 0), and WN_ERR_INVALID for a NULL `a`,
 * a method outside 0..2, steps < 0, traj_every < 0, a non-finite h, gain or drift.  n == 0 is WN_OK.
 */
#ifndef WNOISE_ADVECT_H
#define WNOISE_ADVECT_H

#include "wnoise.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WN_ADVECT_EULER    0
#define WN_ADVECT_MIDPOINT 1
#define WN_ADVECT_RK4      2

typedef struct wn_advect {      /* 8 x 4 bytes */
    int32_t method;             /* one of the three above */
    int32_t steps;              /* >= 0 */
    float   h;                  /* step, any finite value; negative traces backwards */
    float   gain;               /* multiplies the curl */
    float   drift[3];           /* constant velocity added to it */
    int32_t traj_every;         /* 0: no trajectory; e >= 1: snapshot after steps 0, e, 2e, ... <= steps */
} wn_advect;

WN_API int wn_eval3d_curl_advect_points(const wn_tile *tile3d, const float *xyz_in_dev, size_t n,
                                        const int32_t *offsets9_host, const wn_advect *a, float *xyz_out_dev,
                                        float *traj_dev, void *stream);
WN_API int wn_multiband3d_curl_advect_points(const wn_tile *tile3d, const float *xyz_in_dev, size_t n,
                                             const int32_t *offsets9_host, float s, int first_band, int nbands,
                                             const float *w_host, float var_per_band, const wn_advect *a,
                                             float *xyz_out_dev, float *traj_dev, void *stream);
/* The most steps one kernel launch integrates (kAdvectLaunchSteps): a call of more steps is a chain of launches. */
WN_API int wn_advect_launch_steps(void);

#ifdef __cplusplus
}
#endif
#endif /* WNOISE_ADVECT_H */
