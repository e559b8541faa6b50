/* wnoise_bounded2d.h -- C ABI of solid boundaries and a background stream for curl noise on a 2-D tile and for particles
 * moved through it (Bridson, Houriham and Nordenstam, "Curl-Noise for Procedural Fluid Flow", 2007, sections 2.3 and 2.4),
 * exported by libwnoise_hip.so beside the entry points of wnoise_curl2d.h and wnoise_bounded.h, which this header includes;
 * absent from the reference.  Conventions as in those two headers.
 *
 * The stream function psi of wn_multiband2d_curl_points is faded to zero towards every obstacle by the smooth ramp A of
 * wnoise_bounded.h, and the velocity is the curl of the faded stream function,
 *     v = (d(A psi)/dy, -d(A psi)/dx) = A (d psi/dy, -d psi/dx) + psi (dA/dy, -dA/dx).
 * It is still exactly divergence-free, and on an obstacle's surface A -> 0 while grad A is parallel to the normal, so the
 * normal component of v vanishes there.  The obstacle kinds and WN_MAX_OBSTACLES are those of wnoise_bounded.h; in the plane
 * WN_OBSTACLE_SPHERE is a disc, WN_OBSTACLE_CONTAINER a hollow disc and WN_OBSTACLE_HALFSPACE a half-plane.  Obstacles live
 * in the coordinate p of the unbounded entry points: the points passed in, the particles' positions, or the lattice's p of
 * wn_multiband2d_curl_grid (out_scale multiplies last).
 *
 * The background stream.  The constant `drift` of wn_advect2d is added after the ramp: a drifting particle sails straight
 * through a solid.  A uniform stream (ux, uy) that is to flow AROUND the solids belongs into the potential instead,
 *     psi_bg(p) = ux * py - uy * px,   whose curl is (ux, uy),
 * where the ramp bends it with the noise.  flow2_host == NULL: no stream.  flow2_host = {ux, uy}: psi_bg is added, and its
 * terms below are applied even when both are zero.
 *
 * Everything about tiles, bands, the footprint s, wn_advect2d, trajectories, in-place output, launch chaining
 * (wn_advect2d_launch_steps() is the cap, unchanged) and "exactly those floats are written, from any float-aligned pointer"
 * is as in wnoise_curl2d.h.  Argument checks: those of the unbounded entry point come first, in their order.  Then, each
 * WN_ERR_INVALID and whatever n is: nobs outside 0..WN_MAX_OBSTACLES; a NULL list with nobs > 0; a kind outside 0..2; any
 * non-finite field; d0 <= 0; a disc or container with r <= 0; a half-plane with a zero normal; a non-zero reserved field.
 * Then a non-finite ux or uy.  nobs == 0 is valid.
 *
 * Arithmetic, which is the contract.  Float32, unfused: every product, sum, division and square root is rounded on its own.
 *   Distance and ramp are wnoise_bounded.h's with the third component dropped.  Disc kinds: dx = x - c per component,
 *   l2 = dx0*dx0 + dx1*dx1, l = sqrt(l2), m = dx / l per component (m = 0 when l == 0).
 *       WN_OBSTACLE_SPHERE      d = l - r,  nrm = m
 *       WN_OBSTACLE_CONTAINER   d = r - l,  nrm = -m
 *       WN_OBSTACLE_HALFSPACE   d = (n0*x0 + n1*x1) - o,  nrm = n as given (not normalised)
 *   Ramp of obstacle j:
 *       r = d / d0,  r2 = r*r,  alpha = r * (1.875f + r2 * (-1.25f + r2 * 0.375f)),
 *       q = 1.0f - r2,  dalpha = (1.875f * (q*q)) / d0.
 *   A point is INSIDE when some obstacle has d <= 0, FAR when every obstacle has d >= d0, NEAR otherwise.  At a NEAR point
 *   start with A = 1, G = (0, 0), walk the obstacles in list order, skip those with d >= d0, and per component
 *       G = G * alpha + (A * dalpha) * nrm,   then   A = A * alpha.
 *   Stream function.  psi, gx, gy are exactly the three channels {value, d/dx, d/dy} of wn_multiband2d_grad_points at the
 *   call's s.  With flow2_host = {ux, uy}:
 *       psi_t = psi + (ux*py - uy*px),   gx_t = gx - uy,   gy_t = gy + ux;
 *   with flow2_host == NULL psi_t, gx_t, gy_t are psi, gx, gy themselves.
 *   Velocity.
 *       INSIDE  v = (0, 0); under advection such a particle moves by drift alone
 *       FAR     v = (gy_t, -gx_t)
 *       NEAR    v0 = A*gy_t + G1*psi_t,   v1 = -(A*gx_t + G0*psi_t)
 *   With nobs == 0 and flow2_host == NULL every result has the bits of the unbounded entry point, and so has every FAR point
 *   of a call with flow2_host == NULL.
 *   Advection: the stage velocity is k(q) = gain * v(q) + drift with this v, inside the time step of wnoise_curl2d.h.
 * A result has the bits of the host's wnhost_multiband2d_curl_bounded / wnhost_multiband2d_curl_bounded_advect.
 *
 * wn_multiband2d_curl_bounded_points writes n records {vx, vy}; wn_multiband2d_curl_bounded_grid two planes of nx * ny
 * floats, vx then vy, each multiplied by out_scale last.
 *
 * Not provided: Bridson's variant that keeps the normal component; obstacles other than these three kinds; moving
 * obstacles and potentials that change with time; the Perlin field.
 */
#ifndef WNOISE_BOUNDED2D_H
#define WNOISE_BOUNDED2D_H

#include "wnoise_bounded.h"
#include "wnoise_curl2d.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct wn_obstacle2d {     /* 8 x 4 bytes */
    int32_t kind;                  /* WN_OBSTACLE_SPHERE (disc), _CONTAINER (hollow disc) or _HALFSPACE (half-plane) */
    float   c[2];                  /* centre, or the half-plane's normal (any non-zero length) */
    float   r;                     /* radius (> 0), or the half-plane's offset */
    float   d0;                    /* ramp width, > 0: the field is unchanged at distance >= d0 */
    int32_t reserved[3];           /* 0 */
} wn_obstacle2d;

WN_API int wn_multiband2d_curl_bounded_points(const wn_tile *tile2d, const float *xy_dev, size_t n, float s, int first_band,
                                              int nbands, const float *w_host, float var_per_band,
                                              const wn_obstacle2d *obstacles_host, int nobs, const float *flow2_host,
                                              float *out2_dev, void *stream);
WN_API int wn_multiband2d_curl_bounded_grid(const wn_tile *tile2d, const wn_grid *g, float s, int first_band, int nbands,
                                            const float *w_host, float var_per_band, const wn_obstacle2d *obstacles_host,
                                            int nobs, const float *flow2_host, float *out_dev, void *stream);
WN_API int wn_multiband2d_curl_bounded_advect_points(const wn_tile *tile2d, const float *xy_in_dev, size_t n, float s,
                                                     int first_band, int nbands, const float *w_host, float var_per_band,
                                                     const wn_obstacle2d *obstacles_host, int nobs, const float *flow2_host,
                                                     const wn_advect2d *a, float *xy_out_dev, float *traj_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* WNOISE_BOUNDED2D_H */
