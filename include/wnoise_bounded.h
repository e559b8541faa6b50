/* wnoise_bounded.h -- C ABI of solid boundaries for the curl noise of 3-D wavelet noise potentials and for particles moved
 * through it (Bridson, Houriham and Nordenstam, "Curl-Noise for Procedural Fluid Flow", 2007, section 2.4), exported by
 * libwnoise_hip.so beside the entry points of wnoise.h and wnoise_advect.h; absent from the reference.  Conventions as in
 * wnoise_advect.h, which this header includes.
 *
 * The vector potential Psi of wn_eval3d_curl_points / wn_multiband3d_curl_points is faded to zero towards every obstacle by
 * a smooth ramp A of the distance to it, and the velocity is the curl of the faded potential,
 *     v = curl(A Psi) = A (curl Psi) + grad A x Psi.
 * It is still exactly divergence-free, and on an obstacle's surface A -> 0 while grad A is parallel to the normal, so the
 * normal component of v vanishes there: particles flow around a solid, not through it.  Obstacles live in the coordinate
 * the particles live in: the noise-space point passed to wn_eval3d_curl_points, or the lattice coordinate p of the
 * multiband form.  Overlapping ramps multiply, which keeps both properties and keeps the field C1 across d = d0.
 *
 * Everything about tiles, offsets9_host, bands, wn_advect, trajectories, in-place output, launch chaining
 * (wn_advect_launch_steps() is the cap) and "exactly those floats are written, from any float-aligned pointer" is as in the
 * unbounded entry points, and so are their argument checks.  New checks, each WN_ERR_INVALID: nobs outside
 * 0..WN_MAX_OBSTACLES; a NULL list with nobs > 0; a kind outside 0..2; any non-finite field; d0 <= 0; a sphere or container
 * with r <= 0; a half-space with a zero normal; a non-zero reserved field.  nobs == 0 is valid and gives the unbounded bits.
 *
 * Arithmetic, which is the contract.  Float32, unfused: every product, sum, division and square root is rounded on its own
 * (IEEE / and sqrtf).
 *   Distance of obstacle j at x.  Sphere kinds: dx = x - c per component, l2 = (dx0*dx0 + dx1*dx1) + dx2*dx2, l = sqrt(l2),
 *   m = dx / l per component (m = 0 when l == 0).
 *       WN_OBSTACLE_SPHERE      d = l - r,  nrm = m
 *       WN_OBSTACLE_CONTAINER   d = r - l,  nrm = -m
 *       WN_OBSTACLE_HALFSPACE   d = ((n0*x0 + n1*x1) + n2*x2) - o,  nrm = n as given.  The normal is not normalised: d is
 *                               then a linear function whose exact gradient is n, consistent for any length.
 *   Ramp of obstacle j (Bridson's quintic; its derivative is 15/8 (1 - r^2)^2):
 *       r = d / d0,  r2 = r*r,  alpha = r * (1.875f + r2 * (-1.25f + r2 * 0.375f)),
 *       q = 1.0f - r2,  dalpha = (1.875f * (q*q)) / d0.
 *   A point is INSIDE when some obstacle has d <= 0: v = (0, 0, 0); under advection such a particle moves by drift alone.
 *   A point is FAR when every obstacle has d >= d0: v is exactly the unbounded entry point's result, the same bits, and the
 *   potential values are not evaluated.  Every other point is NEAR: start with A = 1, G = (0, 0, 0), walk the obstacles in
 *   list order, skip those with d >= d0, and per component
 *       G = G * alpha + (A * dalpha) * nrm,   then   A = A * alpha.
 *   With c the curl with exactly the bits of wn_eval3d_curl_points / wn_multiband3d_curl_points and Psi_k the potential
 *   values with exactly the bits of wn_eval3d_points / wn_multiband3d_points (normal == NULL) on the rolled tile T_k,
 *       v = A*c + (G x Psi),   e.g.  v0 = A*c0 + (G1*Psi2 - G2*Psi1).
 *   Advection: the stage velocity is k(q) = gain * v(q) + drift with this v, inside the time step of wnoise_advect.h.
 * A result has the bits of the host's wnhost_eval3d_curl_bounded / wnhost_eval3d_curl_bounded_advect.
 *
 * Not provided: Bridson's variant that keeps the normal component of Psi; obstacles other than these three kinds; moving
 * obstacles and potentials that change with time; dense grids.  The Perlin and 2-D fields have their boundaries in headers
 * of their own: wnoise_perlin_bounded.h (fp64, with this header's wn_obstacle) and wnoise_bounded2d.h.  Lattices are served
 * on sparse lists of 8 x 8 x 8 bricks, by wnoise_bounded_bricks.h.
 */
#ifndef WNOISE_BOUNDED_H
#define WNOISE_BOUNDED_H

#include "wnoise_advect.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WN_OBSTACLE_SPHERE     0   /* solid ball: fluid where |x - c| > r */
#define WN_OBSTACLE_CONTAINER  1   /* hollow ball: fluid where |x - c| < r */
#define WN_OBSTACLE_HALFSPACE  2   /* c is a normal n (any non-zero length), r an offset o: fluid where n.x > o */
#define WN_MAX_OBSTACLES      16

typedef struct wn_obstacle {       /* 8 x 4 bytes */
    int32_t kind;                  /* one of the three above */
    float   c[3];                  /* centre, or the half-space's normal */
    float   r;                     /* radius (> 0), or the half-space's offset */
    float   d0;                    /* ramp width, > 0: the field is unchanged at distance >= d0 */
    int32_t reserved[2];           /* 0 */
} wn_obstacle;

WN_API int wn_eval3d_curl_bounded_points(const wn_tile *tile3d, const float *xyz_dev, size_t n, const int32_t *offsets9_host,
                                         const wn_obstacle *obstacles_host, int nobs, float *out3_dev, void *stream);
WN_API int wn_multiband3d_curl_bounded_points(const wn_tile *tile3d, const float *xyz_dev, size_t n,
                                              const int32_t *offsets9_host, float s, int first_band, int nbands,
                                              const float *w_host, float var_per_band, const wn_obstacle *obstacles_host,
                                              int nobs, float *out3_dev, void *stream);
WN_API int wn_eval3d_curl_bounded_advect_points(const wn_tile *tile3d, const float *xyz_in_dev, size_t n,
                                                const int32_t *offsets9_host, const wn_obstacle *obstacles_host, int nobs,
                                                const wn_advect *a, float *xyz_out_dev, float *traj_dev, void *stream);
WN_API int wn_multiband3d_curl_bounded_advect_points(const wn_tile *tile3d, const float *xyz_in_dev, size_t n,
                                                     const int32_t *offsets9_host, float s, int first_band, int nbands,
                                                     const float *w_host, float var_per_band,
                                                     const wn_obstacle *obstacles_host, int nobs, const wn_advect *a,
                                                     float *xyz_out_dev, float *traj_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* WNOISE_BOUNDED_H */
