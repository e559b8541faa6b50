/* wnoise_curl2d.h -- C ABI of divergence-free curl noise on a 2-D tile and of fused particle advection through it (Bridson,
 * Houriham and Nordenstam, "Curl-Noise for Procedural Fluid Flow", 2007), exported by libwnoise_hip.so beside the entry
 * points of wnoise.h; absent from the reference.  Conventions as in wnoise.h, which this header includes through
 * wnoise_multiband2d.h; the WN_ADVECT_* method constants are those of wnoise_advect.h.
 *
 * The field.  The stream function psi(p) is WMultibandNoise on the 2-D tile (wnoise_multiband2d.h) at ONE footprint s for
 * the whole call, with the hard cut (fade 0): the function behind wn_multiband2d_grad_points.  The velocity is
 *     v(p) = (d psi/dy, -d psi/dx):
 *   vx  has the bits of that entry point's d/dy channel;
 *   vy  has the bits of its d/dx channel with the sign flipped (an exact operation; a zero becomes -0.0f).
 * div v = 0 wherever psi is twice differentiable.  An empty tile, no active band, or all-zero weights give v = 0.
 * first_band = -1, nbands = 1, w = {1}, var_per_band = 1 gives the curl of plain evaluate2D(p): q = 2 * p * 2^-1 = p
 * exactly, and the division is by sqrtf(1 * 1) = 1.  There is no separate single-band entry point.
 * Every channel has the bits of the host evaluator wnhost_multiband2d_curl (host/scalar_eval.h); a result depends neither
 * on the other samples of the call nor on their number.
 *
 * wn_multiband2d_curl_points writes n records {vx, vy}.  wn_multiband2d_curl_grid writes two consecutive planes of
 * nx * ny floats, vx then vy, on the lattice of wn_multiband2d_grad_grid: p = ((i / den) * base_range) * octave_scale *
 * post_scale on both axes; out_scale multiplies both channels last; z0, z1, z_mode, z_const and flags are ignored.
 *
 * Advection.  A particle is a packed float pair in the coordinates of p.  One call of wn_multiband2d_curl_advect_points
 * moves every particle `steps` explicit time steps of size h through the stage velocity
 *     k(q) = gain * v(q) + drift
 * with the arithmetic of wnoise_advect.h in two dimensions, which is the contract: everything is float32; every product
 * and every sum is rounded on its own (unfused); per component
 *     k(q) = gain * v(q) + drift                one multiply, then one add
 *     h2 = 0.5f * h,  h6 = h / 6.0f             both formed once, on the host
 *     WN_ADVECT_EULER     p' = p + h * k(p)
 *     WN_ADVECT_MIDPOINT  k1 = k(p);  p' = p + h * k(p + h2 * k1)
 *     WN_ADVECT_RK4       k1 = k(p), k2 = k(p + h2 * k1), k3 = k(p + h2 * k2), k4 = k(p + h * k3);
 *                         p' = p + h6 * (((k1 + 2.0f * k2) + 2.0f * k3) + k4)
 * A result therefore has the bits of composing wn_multiband2d_curl_points with these operations written out as separately
 * rounded float32 operations, and of the host's wnhost_multiband2d_curl_advect.  The steps run inside the kernel
 * (csrc/wn_wavelet_curl2d.hip): position, stage point and RK4's running sum stay in registers, and a tile that fits is
 * read from LDS, so the particle order does not matter.  A call of more than wn_advect2d_launch_steps(method, nbands) steps
 * is a chain of launches on `stream`; the bits do not depend on where the launch boundaries fall.  A particle that reaches a
 * non-finite position gets no special handling: the same composition defines what follows.
 *
 * wn_advect2d (7 x 4 bytes): wn_advect with a drift of two components.
 *   method       WN_ADVECT_EULER, WN_ADVECT_MIDPOINT or WN_ADVECT_RK4
 *   steps        >= 0; 0 copies the input
 *   h            the step, any finite value; a negative one traces backwards
 *   gain, drift  finite
 *   traj_every   0: no trajectory.  e >= 1: a snapshot of every position after steps 0, e, 2e, ... <= steps.
 *
 * Outputs.  xy_out_dev receives the n positions after `steps` steps, whether or not that step is a snapshot.  It may be
 * xy_in_dev itself (in place); any other overlap of the two ranges of 2 n floats is WN_ERR_INVALID.  traj_dev is read only
 * when traj_every >= 1 and must then be non-NULL: steps / traj_every + 1 snapshots, time-major [snapshot][n][2]; snapshot 0
 * is the input.  Placement as in wnoise.h: pointers need only a float's alignment, exactly the output is written, and
 * results do not depend on alignment.
 *
 * Argument checks.  Tile, bands, points and grid as wn_multiband2d_grad_points / _grad_grid, in their order (a NULL tile, a
 * 3-D tile, a tile of another device; nbands outside 0..8, NULL w_host with nbands > 0; NULL points or out with n > 0; the
 * grid's own checks).  Then, for the advection call, WN_ERR_INVALID for a NULL `a`, a method outside 0..2, steps < 0,
 * traj_every < 0, a non-finite h, gain or drift -- whatever n is; n == 0 is WN_OK.
 */
#ifndef WNOISE_CURL2D_H
#define WNOISE_CURL2D_H

#include "wnoise_advect.h"
#include "wnoise_multiband2d.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct wn_advect2d {    /* 7 x 4 bytes */
    int32_t method;             /* WN_ADVECT_EULER, WN_ADVECT_MIDPOINT or WN_ADVECT_RK4 */
    int32_t steps;              /* >= 0 */
    float   h;                  /* step, any finite value; negative traces backwards */
    float   gain;               /* multiplies the curl */
    float   drift[2];           /* constant velocity added to it */
    int32_t traj_every;         /* 0: no trajectory; e >= 1: snapshot after steps 0, e, 2e, ... <= steps */
} wn_advect2d;

WN_API int wn_multiband2d_curl_points(const wn_tile *tile2d, const float *xy_dev, size_t n, float s, int first_band,
                                      int nbands, const float *w_host, float var_per_band, float *out2_dev, void *stream);
WN_API int wn_multiband2d_curl_grid(const wn_tile *tile2d, const wn_grid *g, float s, int first_band, int nbands,
                                    const float *w_host, float var_per_band, float *out_dev, void *stream);
WN_API int wn_multiband2d_curl_advect_points(const wn_tile *tile2d, const float *xy_in_dev, size_t n, float s,
                                             int first_band, int nbands, const float *w_host, float var_per_band,
                                             const wn_advect2d *a, float *xy_out_dev, float *traj_dev, void *stream);
/* The steps one kernel launch integrates for that method and band count (at least 1): a call of more steps is a chain of
 * launches.  A method outside 0..2 counts as RK4, nbands outside 0..8 is clamped. */
WN_API int wn_advect2d_launch_steps(int method, int nbands);

#ifdef __cplusplus
}
#endif
#endif /* WNOISE_CURL2D_H */
