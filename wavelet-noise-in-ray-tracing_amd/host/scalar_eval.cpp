// scalar_eval.cpp -- the reference's scalar members on the host, one sample per call (see scalar_eval.h).  Every function is
// a call of the evaluator that the HIP kernels use (csrc/wn_eval.hpp: one statement of each loop, the reference's file:line
// beside it), built with -ffp-contract=off like them: every product and sum rounds once, as on the reference's baseline
// x86-64 build.
#include "scalar_eval.h"

#include <cmath>
#include <cstdlib>

#include "wn_advect.hpp"
#include "wn_eval.hpp"
#include "wnoise_advect.h"
#include "wnoise_bounded.h"
#include "wnoise_bounded2d.h"
#include "wnoise_curl2d.h"
#include "wnoise_perlin_bounded.h"
#include "wnoise_perlin_curl.h"

namespace {

struct WaveletTexture { // what wn::wavelet_texture_value reads
    const float *coef;
    int n, nmask, mode;
    double scale;
    float octave_mul, inv_stddev;
};

struct Footprint : wn::FootprintBands { // what wn::multiband_footprint_exact and the texture adaptor read
    const float *coef;
    int n, nmask;
    double scale;
};

// false: nothing to evaluate (nbands out of range)
bool footprint_setup(Footprint &a, const float *coef, int n, int first_band, int nbands, const float *w, float var_per_band,
                     int fade)
{
    if (nbands < 0 || nbands > wn::kFootprintMaxBands || (nbands && !w)) return false;
    wn::footprint_bands_fill(first_band, nbands, w, var_per_band, fade, &a);
    a.coef = coef;
    a.n = (coef && n > 0) ? n : 0;
    a.nmask = wn::pow2_mask(a.n);
    a.scale = 1.0;
    return true;
}

// false: a wn_advect / wn_advect2d that no trace can follow, or one that asks for a trajectory without a buffer for it
template <typename A>
bool advect_ok(const A *a, const void *traj)
{
    if (!a || a->method < WN_ADVECT_EULER || a->method > WN_ADVECT_RK4 || a->steps < 0 || a->traj_every < 0) return false;
    bool finite = std::isfinite(a->h) && std::isfinite(a->gain);
    for (const float d : a->drift) finite = finite && std::isfinite(d);
    return finite && (!a->traj_every || traj);
}

// One particle's whole trace: the chain of wn_advect.hpp with a single launch of all the steps, on a list of one.
template <typename T, int D, typename A, typename V>
void advect_one(const A &a, const T *p_in, T *p_out, T *traj, const V &velocity)
{
    wn::advect_chain(wn::advect_trace_fill<T, D>(a, 1), p_in, p_out, traj, a.steps, a.steps, [&](const wn::AdvectTrace<T, D> &t) {
        T p[D];
        for (int c = 0; c < D; ++c) p[c] = t.in[c];
        wn::with_advect_method(a.method, [&](auto method) {
            wn::advect_trace<decltype(method)::value>(t, p, 0, velocity, [&](T *dst) {
                for (int c = 0; c < D; ++c) dst[c] = p[c];
            });
        });
        return 0;
    });
}

} // namespace

extern "C" {

float wnhost_eval2d(const float *coef, int n, const float p[2])
{
    if (!coef || n <= 0) return 0.0f;
    return wn::eval2d_exact(coef, n, wn::pow2_mask(n), p[0], p[1]);
}

float wnhost_eval3d(const float *coef, int n, const float p[3])
{
    if (!coef || n <= 0) return 0.0f;
    return wn::eval3d_exact(coef, n, wn::pow2_mask(n), p[0], p[1], p[2]);
}

float wnhost_eval2d_grad(const float *coef, int n, const float p[2], float grad[2])
{
    grad[0] = grad[1] = 0.0f;
    if (!coef || n <= 0) return 0.0f;
    return wn::eval2d_exact<true>(coef, n, wn::pow2_mask(n), p[0], p[1], grad);
}

float wnhost_eval3d_grad(const float *coef, int n, const float p[3], float grad[3])
{
    grad[0] = grad[1] = grad[2] = 0.0f;
    if (!coef || n <= 0) return 0.0f;
    return wn::eval3d_grad_exact(coef, n, wn::pow2_mask(n), p[0], p[1], p[2], grad);
}

void wnhost_eval3d_curl(const float *coef, int n, const float p[3], const int offsets9[9], float v[3])
{
    v[0] = v[1] = v[2] = 0.0f;
    if (!coef || n <= 0) return;
    const int nmask = wn::pow2_mask(n);
    int off[9];
    for (int i = 0; i < 9; ++i) off[i] = wn::dmod(offsets9[i], n, nmask);
    wn::eval3d_curl_exact(coef, n, nmask, off, p[0], p[1], p[2], v);
}

int wnhost_eval3d_curl_advect(const float *coef, int n, const float p_in[3], const int offsets9[9], const wn_advect *a,
                              float p_out[3], float *traj)
{
    return wnhost_eval3d_curl_bounded_advect(coef, n, p_in, offsets9, nullptr, 0, a, p_out, traj); // no obstacle: the same bits
}

int wnhost_eval3d_curl_bounded(const float *coef, int n, const float p[3], const int offsets9[9], const wn_obstacle *obstacles,
                               int nobs, float v[3])
{
    if (wn::obstacle_fault(obstacles, nobs)) return 1;
    if (!coef || n <= 0) n = 0;
    const int nmask = wn::pow2_mask(n);
    int off[9];
    for (int i = 0; i < 9; ++i) off[i] = n ? wn::dmod(offsets9[i], n, nmask) : 0;
    wn::eval3d_curl_bounded_exact(coef, n, nmask, off, obstacles, nobs, p, v);
    return 0;
}

int wnhost_eval3d_curl_bounded_advect(const float *coef, int n, const float p_in[3], const int offsets9[9],
                                      const wn_obstacle *obstacles, int nobs, const wn_advect *a, float p_out[3], float *traj)
{
    if (wn::obstacle_fault(obstacles, nobs)) return 1;
    if (!advect_ok(a, traj)) return 1;
    if (!coef || n <= 0) n = 0;
    const int nmask = wn::pow2_mask(n);
    int off[9];
    for (int i = 0; i < 9; ++i) off[i] = n ? wn::dmod(offsets9[i], n, nmask) : 0;
    const auto velocity = [&](const float q[3], float v[3]) {
        wn::eval3d_curl_bounded_exact(coef, n, nmask, off, obstacles, nobs, q, v);
    };
    advect_one<float, 3>(*a, p_in, p_out, traj, velocity);
    return 0;
}

float wnhost_eval3d_projected(const float *coef, int n, const float p[3], const float nrm[3])
{
    if (!coef || n <= 0) return 0.0f;
    return wn::projected_exact(coef, n, wn::pow2_mask(n), p, nrm);
}

float wnhost_eval3d_projected_grad(const float *coef, int n, const float p[3], const float nrm[3], float grad[3])
{
    grad[0] = grad[1] = grad[2] = 0.0f;
    if (!coef || n <= 0) return 0.0f;
    return wn::projected_grad_exact(coef, n, wn::pow2_mask(n), p, nrm, grad);
}

float wnhost_multiband3d_footprint(const float *coef, int n, const float p[3], const float *normal, float s, int fade,
                                   int first_band, int nbands, const float *w, float var_per_band, float *grad)
{
    if (grad) grad[0] = grad[1] = grad[2] = 0.0f;
    Footprint a;
    if (!footprint_setup(a, coef, n, first_band, nbands, w, var_per_band, fade)) return 0.0f;
    if (normal)
        return grad ? wn::multiband_footprint_exact<false, true, true>(a, p, normal, s, grad)
                    : wn::multiband_footprint_exact<false, true, false>(a, p, normal, s, nullptr);
    return grad ? wn::multiband_footprint_exact<false, false, true>(a, p, nullptr, s, grad)
                : wn::multiband_footprint_exact<false, false, false>(a, p, nullptr, s, nullptr);
}

float wnhost_multiband2d_footprint(const float *coef, int n, const float p[2], float s, int fade, int first_band, int nbands,
                                   const float *w, float var_per_band, float *grad)
{
    if (grad) grad[0] = grad[1] = 0.0f;
    Footprint a;
    if (!footprint_setup(a, coef, n, first_band, nbands, w, var_per_band, fade)) return 0.0f;
    return grad ? wn::multiband2d_footprint_exact<true>(a, a.coef, p, s, grad)
                : wn::multiband2d_footprint_exact<false>(a, a.coef, p, s, nullptr);
}

void wnhost_multiband2d_curl(const float *coef, int n, const float p[2], float s, int first_band, int nbands, const float *w,
                             float var_per_band, float v[2])
{
    v[0] = v[1] = 0.0f;
    Footprint a;
    if (!footprint_setup(a, coef, n, first_band, nbands, w, var_per_band, 0)) return;
    wn::multiband2d_curl_exact(a, a.coef, p, s, v);
}

int wnhost_multiband2d_curl_advect(const float *coef, int n, const float p_in[2], float s, int first_band, int nbands,
                                   const float *w, float var_per_band, const wn_advect2d *a, float p_out[2], float *traj)
{
    // no obstacle and no stream: the same bits
    return wnhost_multiband2d_curl_bounded_advect(coef, n, p_in, s, first_band, nbands, w, var_per_band, nullptr, 0, nullptr, a,
                                                  p_out, traj);
}

int wnhost_multiband2d_curl_bounded(const float *coef, int n, const float p[2], float s, int first_band, int nbands,
                                    const float *w, float var_per_band, const wn_obstacle2d *obstacles, int nobs,
                                    const float *flow2, float v[2])
{
    if (wn::obstacle_fault<2>(obstacles, nobs)) return 1;
    if (flow2 && !(std::isfinite(flow2[0]) && std::isfinite(flow2[1]))) return 1;
    Footprint f;
    if (!footprint_setup(f, coef, n, first_band, nbands, w, var_per_band, 0)) return 1;
    wn::multiband2d_curl_bounded_exact(f, f.coef, obstacles, nobs, flow2, p, s, v);
    return 0;
}

int wnhost_multiband2d_curl_bounded_advect(const float *coef, int n, const float p_in[2], float s, int first_band, int nbands,
                                           const float *w, float var_per_band, const wn_obstacle2d *obstacles, int nobs,
                                           const float *flow2, const wn_advect2d *a, float p_out[2], float *traj)
{
    if (!advect_ok(a, traj)) return 1;
    if (wn::obstacle_fault<2>(obstacles, nobs)) return 1;
    if (flow2 && !(std::isfinite(flow2[0]) && std::isfinite(flow2[1]))) return 1;
    Footprint f;
    if (!footprint_setup(f, coef, n, first_band, nbands, w, var_per_band, 0)) return 1;
    const auto velocity = [&](const float q[2], float v[2]) {
        wn::multiband2d_curl_bounded_exact(f, f.coef, obstacles, nobs, flow2, q, s, v);
    };
    advect_one<float, 2>(*a, p_in, p_out, traj, velocity);
    return 0;
}

float wnhost_wavelet_multiband_texture_value(const float *coef, int n, double scale, int first_band, int nbands,
                                             const float *w, float var_per_band, int fade, const float xyz[3], float s)
{
    Footprint a;
    if (!footprint_setup(a, coef, n, first_band, nbands, w, var_per_band, fade)) return wn::wavelet_texture_grey(0.0);
    a.scale = scale;
    return wn::wavelet_multiband_texture_value<false>(a, xyz[0], xyz[1], xyz[2], s);
}

double wnhost_perlin(const int *perm, double x, double y, double z) { return wn::perlin_exact(perm, x, y, z); }

double wnhost_perlin_fractal(const int *perm, const float q[3]) { return wn::perlin_fractal(perm, q[0], q[1], q[2]); }

double wnhost_perlin_turb(const int *perm, const float q[3], int depth)
{
    return wn::perlin_turb(perm, q[0], q[1], q[2], depth);
}

double wnhost_perlin_grad(const int *perm, double x, double y, double z, double grad[3])
{
    return wn::perlin_grad_exact(perm, x, y, z, grad);
}

double wnhost_perlin_fractal_grad(const int *perm, const float q[3], double grad[3])
{
    return wn::perlin_fractal_grad(perm, q[0], q[1], q[2], grad);
}

double wnhost_perlin_turb_grad(const int *perm, const float q[3], int depth, double grad[3])
{
    return wn::perlin_turb_grad(perm, q[0], q[1], q[2], depth, grad);
}

double wnhost_perlin_turb_footprint(const int *perm, const float q[3], int depth, float s, float bias, int fade, double *grad)
{
    if (grad) grad[0] = grad[1] = grad[2] = 0.0;
    if (depth < 0 || depth > wn::kPerlinFootprintMaxOctaves) return 0.0;
    return grad ? wn::perlin_turb_footprint<true>(perm, q[0], q[1], q[2], depth, s, bias, fade, grad)
                : wn::perlin_turb_footprint<false>(perm, q[0], q[1], q[2], depth, s, bias, fade, nullptr);
}

double wnhost_perlin_fractal_footprint(const int *perm, const float q[3], int octaves, float s, float bias, int fade,
                                       double *grad)
{
    if (grad) grad[0] = grad[1] = grad[2] = 0.0;
    if (octaves < 0 || octaves > wn::kPerlinFootprintMaxOctaves) return 0.0;
    return grad ? wn::perlin_fractal_footprint<true>(perm, q[0], q[1], q[2], octaves, s, bias, fade, grad)
                : wn::perlin_fractal_footprint<false>(perm, q[0], q[1], q[2], octaves, s, bias, fade, nullptr);
}

float wnhost_noise_multiband_texture_value(const int *perm, double scale, int octaves, float bias, int fade,
                                           const float xyz[3], float s)
{
    if (octaves < 0 || octaves > wn::kPerlinFootprintMaxOctaves) return 0.5f;
    return wn::noise_multiband_texture_value(perm, (float)scale, octaves, bias, fade, xyz[0], xyz[1], xyz[2], s);
}

void wnhost_perlin_curl(const int *perm, double x, double y, double z, const int offsets9[9], double v[3])
{
    wn::perlin_curl_exact(perm, x, y, z, offsets9, v);
}

void wnhost_perlin_turb_curl(const int *perm, const float q[3], int depth, const int offsets9[9], double v[3])
{
    wn::perlin_turb_curl(perm, q[0], q[1], q[2], depth, offsets9, v);
}

void wnhost_perlin_fractal_curl(const int *perm, const float q[3], const int offsets9[9], double v[3])
{
    wn::perlin_fractal_curl(perm, q[0], q[1], q[2], offsets9, v);
}

int wnhost_perlin_curl_advect(const int *perm, int kind, int depth, const double p_in[3], const int offsets9[9],
                              const wn_advect *a, double p_out[3], double *traj)
{
    if (kind < WN_PERLIN_CURL_NOISE || kind > WN_PERLIN_CURL_FRACTAL || (kind == WN_PERLIN_CURL_TURB && depth < 0)) return 1;
    if (!advect_ok(a, traj)) return 1;
    const auto velocity = [&](const double q[3], double v[3]) {
        if (kind == WN_PERLIN_CURL_NOISE) wn::perlin_curl_exact(perm, q[0], q[1], q[2], offsets9, v);
        else if (kind == WN_PERLIN_CURL_TURB) wn::perlin_turb_curl(perm, (float)q[0], (float)q[1], (float)q[2], depth, offsets9, v);
        else wn::perlin_fractal_curl(perm, (float)q[0], (float)q[1], (float)q[2], offsets9, v);
    };
    advect_one<double, 3>(*a, p_in, p_out, traj, velocity);
    return 0;
}

void wnhost_perlin_curl_potential(const int *perm, double x, double y, double z, const int offsets9[9], double psi[3])
{
    wn::perlin_curl_potential<WN_PERLIN_CURL_NOISE>(perm, x, y, z, 0, offsets9, psi);
}

void wnhost_perlin_turb_curl_potential(const int *perm, const float q[3], int depth, const int offsets9[9], double psi[3])
{
    wn::perlin_curl_potential<WN_PERLIN_CURL_TURB>(perm, q[0], q[1], q[2], depth, offsets9, psi);
}

void wnhost_perlin_fractal_curl_potential(const int *perm, const float q[3], const int offsets9[9], double psi[3])
{
    wn::perlin_curl_potential<WN_PERLIN_CURL_FRACTAL>(perm, q[0], q[1], q[2], 0, offsets9, psi);
}

int wnhost_perlin_curl_bounded(const int *perm, int kind, int depth, const double p[3], const int offsets9[9],
                               const wn_obstacle *obstacles, int nobs, double v[3])
{
    if (kind < WN_PERLIN_CURL_NOISE || kind > WN_PERLIN_CURL_FRACTAL || (kind == WN_PERLIN_CURL_TURB && depth < 0)) return 1;
    if (wn::obstacle_fault(obstacles, nobs)) return 1;
    if (kind == WN_PERLIN_CURL_NOISE)
        wn::perlin_curl_bounded<WN_PERLIN_CURL_NOISE>(perm, p[0], p[1], p[2], 0, offsets9, obstacles, nobs, v);
    else if (kind == WN_PERLIN_CURL_TURB)
        wn::perlin_curl_bounded<WN_PERLIN_CURL_TURB>(perm, (float)p[0], (float)p[1], (float)p[2], depth, offsets9, obstacles,
                                                     nobs, v);
    else
        wn::perlin_curl_bounded<WN_PERLIN_CURL_FRACTAL>(perm, (float)p[0], (float)p[1], (float)p[2], 0, offsets9, obstacles,
                                                        nobs, v);
    return 0;
}

int wnhost_perlin_curl_bounded_advect(const int *perm, int kind, int depth, const double p_in[3], const int offsets9[9],
                                      const wn_obstacle *obstacles, int nobs, const wn_advect *a, double p_out[3], double *traj)
{
    if (kind < WN_PERLIN_CURL_NOISE || kind > WN_PERLIN_CURL_FRACTAL || (kind == WN_PERLIN_CURL_TURB && depth < 0)) return 1;
    if (wn::obstacle_fault(obstacles, nobs)) return 1;
    if (!advect_ok(a, traj)) return 1;
    const auto velocity = [&](const double q[3], double v[3]) {
        wnhost_perlin_curl_bounded(perm, kind, depth, q, offsets9, obstacles, nobs, v);
    };
    advect_one<double, 3>(*a, p_in, p_out, traj, velocity);
    return 0;
}

float wnhost_wavelet_texture_value(const float *coef, int n, int use_3d, double scale, int octave, const float xyz[3])
{
    const float octave_scale = (float)std::pow(2.0, (double)octave); // std::pow(2.0f, int) is evaluated in double, :77
    WaveletTexture t;
    t.coef = coef;
    t.n = n > 0 ? n : 0;
    t.nmask = wn::pow2_mask(n);
    t.mode = !coef ? 0 : (use_3d ? 3 : 2);
    t.scale = scale;
    t.octave_mul = octave_scale * 2.0f;
    t.inv_stddev = 1.0f / std::sqrt(use_3d ? 0.18402f : 0.19686f); // :84-85, :98-99
    return wn::wavelet_texture_value<false>(t, xyz[0], xyz[1], xyz[2]);
}

float wnhost_noise_texture_value(const int *perm, double scale, int octave, const float xyz[3])
{
    const float octave_scale = (float)std::pow(2.0, (double)octave);
    // vec3 * double narrows the factor (vec3.h:82-84)
    return wn::noise_texture_value(perm, (float)scale, octave_scale, xyz[0], xyz[1], xyz[2]);
}

int wnhost_scalar_on_device(void)
{
    static const int on = [] {
        const char *e = std::getenv("WN_SCALAR_ON_DEVICE");
        return (e && *e && *e != '0') ? 1 : 0;
    }();
    return on;
}

} // extern "C"
