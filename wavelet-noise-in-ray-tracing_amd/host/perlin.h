// perlin.h -- the reference's class perlin (perlin.h:14-91) over the MI355X C ABI.
//
// Same constructor and members; the permutation table is built on the host by the same libstdc++
// calls as the reference (iota + std::shuffle(mt19937(seed)), perlin.h:34-39, via
// wn_perm_create_seeded) and lives on the device as 512 bytes.  The batched forms run as HIP kernels in fp64 with the
// reference's operation order; the scalar members are evaluated on the host from the mirrored table (scalar_eval.h;
// WN_SCALAR_ON_DEVICE=1: by the resident scalar kernel).  Bit-identical either way.
// Additive: turb() (RTOW; absent from the reference), batched overloads, analytic gradients, curl noise
// particles advected through it, and octave limiting by a footprint per sample.
#ifndef PERLIN_H
#define PERLIN_H

#include <cstddef>
#include <random>
#include <vector>

#include "scalar_eval.h"
#include "vec3.h"
#include "wn_host.hpp"
#include "wnoise_perlin_advect.h"
#include "wnoise_perlin_bounded.h"
#include "wnoise_perlin_curl.h"
#include "wnoise_perlin_footprint.h"

using point3 = vec3;

class perlin {
  private:
    std::vector<int> p; // host mirror of the table (perlin.h:16)
    wn_perm *perm_ = nullptr;

    double scalar(const point3 &q, int kind, int depth) const // kind 1: turb, 2: fractal_noise
    {
        const float xyz[3] = {q.x(), q.y(), q.z()};
        if (!wnhost_scalar_on_device()) return kind == 1 ? wnhost_perlin_turb(p.data(), xyz, depth) : wnhost_perlin_fractal(p.data(), xyz);
        double v = 0.0;
        wnhost::check(wn_scalar_perlin_vec3(perm_, xyz, kind, depth, &v), "wn_scalar_perlin_vec3");
        return v;
    }

  public:
    explicit perlin(unsigned int seed = std::mt19937::default_seed) : p(512)
    {
        wnhost::check(wn_perm_create_seeded(seed, &perm_), "wn_perm_create_seeded");
        wnhost::check(wn_perm_download(perm_, p.data()), "wn_perm_download");
    }
    ~perlin() { wn_perm_destroy(perm_); }
    perlin(const perlin &o) : p(o.p) { wnhost::check(wn_perm_create(p.data(), &perm_), "wn_perm_create"); }
    perlin &operator=(const perlin &) = delete;

    // perlin.h:42-62
    double noise(double x, double y, double z) const noexcept(false)
    {
        if (!wnhost_scalar_on_device()) return wnhost_perlin(p.data(), x, y, z);
        double v = 0.0;
        wnhost::check(wn_scalar_perlin(perm_, x, y, z, &v), "wn_scalar_perlin");
        return v;
    }
    double noise(double x, double y) const { return noise(x, y, 0.0); }              // perlin.h:65-67
    double noise(const point3 &q) const { return noise(q.x(), q.y(), q.z()); }        // perlin.h:70-72

    double fractal_noise(const point3 &q) const                                       // perlin.h:75-90
    {
        return scalar(q, 2, 0);
    }
    // RTOW "The Next Week" turb(p, depth); absent from the reference.
    double turb(const point3 &q, int depth = 7) const
    {
        return scalar(q, 1, depth);
    }

    // ---- additive: batched forms (host pointers) and the device-resident table -------------------
    void noise(const double *xyz, size_t n, double *out) const
    {
        if (!n) return;
        wnhost::DeviceBuffer in(3 * n * sizeof(double)), res(n * sizeof(double));
        in.upload(xyz);
        wnhost::check(wn_perlin_points(perm_, in.as<double>(), n, res.as<double>(), nullptr), "wn_perlin_points");
        res.download(out);
    }

    // ---- additive: analytic gradients (absent from the reference; include/wnoise.h) --------------
    // Scalar members: return the value (the bits of noise / turb / fractal_noise) and write d/dx, d/dy, d/dz to grad;
    // evaluated on the host from the mirrored table (scalar_eval.h), bit-identical to the kernels.
    double noise_gradient(double x, double y, double z, double grad[3]) const { return wnhost_perlin_grad(p.data(), x, y, z, grad); }
    double noise_gradient(const point3 &q, double grad[3]) const { return noise_gradient(q.x(), q.y(), q.z(), grad); }
    double turb_gradient(const point3 &q, double grad[3], int depth = 7) const
    {
        const float xyz[3] = {q.x(), q.y(), q.z()};
        return wnhost_perlin_turb_grad(p.data(), xyz, depth, grad);
    }
    double fractal_noise_gradient(const point3 &q, double grad[3]) const
    {
        const float xyz[3] = {q.x(), q.y(), q.z()};
        return wnhost_perlin_fractal_grad(p.data(), xyz, grad);
    }
    // Batched overloads (host pointers, through the GPU): n records {value, d/dx, d/dy, d/dz} of four doubles to out4.
    void noise_gradient(const double *xyz, size_t n, double *out4) const
    {
        if (!n) return;
        wnhost::DeviceBuffer in(3 * n * sizeof(double)), res(4 * n * sizeof(double));
        in.upload(xyz);
        wnhost::check(wn_perlin_grad_points(perm_, in.as<double>(), n, res.as<double>(), nullptr), "wn_perlin_grad_points");
        res.download(out4);
    }
    void noise_gradient(const float *xyz, size_t n, double *out4) const { grad_vec3(xyz, n, 0, 0, out4); }
    void turb_gradient(const float *xyz, size_t n, double *out4, int depth = 7) const { grad_vec3(xyz, n, 1, depth, out4); }
    void fractal_noise_gradient(const float *xyz, size_t n, double *out4) const { grad_vec3(xyz, n, 2, 0, out4); }

    // ---- additive: divergence-free curl noise (absent from the reference; include/wnoise_perlin_curl.h) ----------
    // v = curl of the three potentials noise / the signed turb sum / fractal_noise on cells shifted by offsets9 (the
    // (x, y, z) triples of psi0, psi1, psi2; NULL: default_curl_offsets(), a default only, not a measured
    // decorrelation).  Scalar members: evaluated on the host, bit-identical to the kernels.
    static const int *default_curl_offsets()
    {
        static const int o[9] = {0, 0, 0, 85, 85, 85, 170, 170, 170};
        return o;
    }
    void noise_curl(double x, double y, double z, double v[3], const int *offsets9 = nullptr) const
    {
        wnhost_perlin_curl(p.data(), x, y, z, offsets9 ? offsets9 : default_curl_offsets(), v);
    }
    void noise_curl(const point3 &q, double v[3], const int *offsets9 = nullptr) const { noise_curl(q.x(), q.y(), q.z(), v, offsets9); }
    void turb_curl(const point3 &q, double v[3], int depth = 7, const int *offsets9 = nullptr) const
    {
        const float xyz[3] = {q.x(), q.y(), q.z()};
        wnhost_perlin_turb_curl(p.data(), xyz, depth, offsets9 ? offsets9 : default_curl_offsets(), v);
    }
    void fractal_noise_curl(const point3 &q, double v[3], const int *offsets9 = nullptr) const
    {
        const float xyz[3] = {q.x(), q.y(), q.z()};
        wnhost_perlin_fractal_curl(p.data(), xyz, offsets9 ? offsets9 : default_curl_offsets(), v);
    }
    // Batched overloads (host pointers, through the GPU): n records {vx, vy, vz} of three doubles to out3.
    void noise_curl(const double *xyz, size_t n, double *out3, const int *offsets9 = nullptr) const
    {
        if (!n) return;
        wnhost::DeviceBuffer in(3 * n * sizeof(double)), res(3 * n * sizeof(double));
        in.upload(xyz);
        wnhost::check(wn_perlin_curl_points(perm_, in.as<double>(), n, curl_offsets(offsets9), res.as<double>(), nullptr), "wn_perlin_curl_points");
        res.download(out3);
    }
    void noise_curl(const float *xyz, size_t n, double *out3, const int *offsets9 = nullptr) const { curl_vec3(xyz, n, WN_PERLIN_CURL_NOISE, 0, offsets9, out3); }
    void turb_curl(const float *xyz, size_t n, double *out3, int depth = 7, const int *offsets9 = nullptr) const { curl_vec3(xyz, n, WN_PERLIN_CURL_TURB, depth, offsets9, out3); }
    void fractal_noise_curl(const float *xyz, size_t n, double *out3, const int *offsets9 = nullptr) const { curl_vec3(xyz, n, WN_PERLIN_CURL_FRACTAL, 0, offsets9, out3); }

    // ---- additive: particles moved through that curl field (absent from the reference; include/wnoise_perlin_advect.h,
    // whose wn_advect `a` is: method, steps, h, gain, drift, traj_every).  kind: WN_PERLIN_CURL_NOISE / _TURB / _FRACTAL, depth
    // read by TURB only; positions are doubles, TURB and FRACTAL evaluate at the stage point rounded to float.  With
    // a.traj_every = e >= 1 the positions after steps 0, e, 2e, ... go to traj, a.steps / e + 1 snapshots of n points each
    // ([snapshot][n][3]).  The scalar member is traced on the host (scalar_eval.h), bit-identical to
    // wn_perlin_curl_advect_points, which the batched one calls.
    void advect_curl(const point3 &q, const wn_advect &a, int kind, int depth, const int *offsets9, double p_out[3],
                     double *traj = nullptr) const
    {
        const double xyz[3] = {q.x(), q.y(), q.z()};
        advect_curl(xyz, a, kind, depth, offsets9, p_out, traj);
    }
    void advect_curl(const double xyz[3], const wn_advect &a, int kind, int depth, const int *offsets9, double p_out[3],
                     double *traj = nullptr) const
    {
        if (wnhost_perlin_curl_advect(p.data(), kind, depth, xyz, offsets9 ? offsets9 : default_curl_offsets(), &a, p_out, traj))
            throw std::runtime_error("advect_curl: a kind or method outside 0..2, a negative depth, steps or traj_every, a "
                                     "non-finite h, gain or drift, or a trajectory without a buffer");
    }
    void advect_curl(const double *xyz, size_t n, const wn_advect &a, int kind, int depth, const int *offsets9, double *xyz_out,
                     double *traj = nullptr) const
    {
        wnhost::perlin_advect_batch(perm_, xyz, n, kind, depth, offsets9 ? offsets9 : default_curl_offsets(), a, xyz_out, traj);
    }

    // ---- additive: that curl field with solid boundaries (absent from the reference; include/wnoise_perlin_bounded.h, whose
    // obstacle list is wnoise_bounded.h's: at most 16 spheres, containers and half-spaces in the coordinates of the points).
    // curl_potential: Psi = (psi0, psi1, psi2), the potentials the curl members differentiate.  curl_bounded:
    // v = A curl Psi + grad A x Psi, zero inside a solid, the curl member's bits far from all of them.  advect_curl_bounded:
    // advect_curl through it.  kind, depth and offsets9 as in advect_curl; NOISE evaluates at the double point, TURB and
    // FRACTAL at the point rounded to float.  Scalar members on the host (scalar_eval.h), batched ones (host pointers; double
    // points: NOISE only) through the GPU; bit-identical to each other.
    void curl_potential(const double xyz[3], int kind, int depth, const int *offsets9, double psi[3]) const
    {
        const int *off = offsets9 ? offsets9 : default_curl_offsets();
        const float q[3] = {(float)xyz[0], (float)xyz[1], (float)xyz[2]};
        if (kind == WN_PERLIN_CURL_NOISE) wnhost_perlin_curl_potential(p.data(), xyz[0], xyz[1], xyz[2], off, psi);
        else if (kind == WN_PERLIN_CURL_TURB && depth >= 0) wnhost_perlin_turb_curl_potential(p.data(), q, depth, off, psi);
        else if (kind == WN_PERLIN_CURL_FRACTAL) wnhost_perlin_fractal_curl_potential(p.data(), q, off, psi);
        else throw std::runtime_error("curl_potential: a kind outside 0..2 or a negative depth");
    }
    void curl_potential(const double *xyz, size_t n, const int *offsets9, double *out3) const
    {
        wnhost::perlin_bounded_points_batch(perm_, xyz, n, WN_PERLIN_CURL_NOISE, 0, curl_offsets_int(offsets9), nullptr, -1, out3);
    }
    void curl_potential(const float *xyz, size_t n, int kind, int depth, const int *offsets9, double *out3) const
    {
        wnhost::perlin_bounded_points_batch(perm_, xyz, n, kind, depth, curl_offsets_int(offsets9), nullptr, -1, out3);
    }
    void curl_bounded(const double xyz[3], int kind, int depth, const int *offsets9, const wn_obstacle *obstacles, int nobs,
                      double v[3]) const
    {
        if (wnhost_perlin_curl_bounded(p.data(), kind, depth, xyz, curl_offsets_int(offsets9), obstacles, nobs, v))
            throw std::runtime_error("curl_bounded: a kind outside 0..2, a negative depth, or an obstacle list that "
                                     "include/wnoise_bounded.h refuses");
    }
    void curl_bounded(const double *xyz, size_t n, const int *offsets9, const wn_obstacle *obstacles, int nobs, double *out3) const
    {
        wnhost::perlin_bounded_points_batch(perm_, xyz, n, WN_PERLIN_CURL_NOISE, 0, curl_offsets_int(offsets9), obstacles,
                                            nobs < 0 ? WN_MAX_OBSTACLES + 1 : nobs, out3);
    }
    void curl_bounded(const float *xyz, size_t n, int kind, int depth, const int *offsets9, const wn_obstacle *obstacles, int nobs,
                      double *out3) const
    {
        wnhost::perlin_bounded_points_batch(perm_, xyz, n, kind, depth, curl_offsets_int(offsets9), obstacles,
                                            nobs < 0 ? WN_MAX_OBSTACLES + 1 : nobs, out3);
    }
    void advect_curl_bounded(const double xyz[3], const wn_advect &a, int kind, int depth, const int *offsets9,
                             const wn_obstacle *obstacles, int nobs, double p_out[3], double *traj = nullptr) const
    {
        if (wnhost_perlin_curl_bounded_advect(p.data(), kind, depth, xyz, curl_offsets_int(offsets9), obstacles, nobs, &a, p_out, traj))
            throw std::runtime_error("advect_curl_bounded: what advect_curl or curl_bounded refuses");
    }
    void advect_curl_bounded(const double *xyz, size_t n, const wn_advect &a, int kind, int depth, const int *offsets9,
                             const wn_obstacle *obstacles, int nobs, double *xyz_out, double *traj = nullptr) const
    {
        wnhost::perlin_bounded_advect_batch(perm_, xyz, n, kind, depth, curl_offsets_int(offsets9), obstacles, nobs, a, xyz_out, traj);
    }

    // ---- additive: octave limiting by a footprint per sample (absent from the reference; include/wnoise_perlin_footprint.h)
    // s = log2 of the sample's footprint in the noise space of q: octave i runs while (s + bias) + i < 0; fade: the finest
    // surviving octave enters with min(1, -t_i) instead of popping.  Scalar members: evaluated on the host, bit-identical
    // to the kernels; the gradient forms return the value and write d/dx, d/dy, d/dz to grad.
    double turb_footprint(const point3 &q, float s, int depth = 7, float bias = 0.0f, bool fade = false) const
    {
        const float xyz[3] = {q.x(), q.y(), q.z()};
        return wnhost_perlin_turb_footprint(p.data(), xyz, depth, s, bias, fade ? 1 : 0, nullptr);
    }
    double fractal_noise_footprint(const point3 &q, float s, int octaves = 6, float bias = 0.0f, bool fade = false) const
    {
        const float xyz[3] = {q.x(), q.y(), q.z()};
        return wnhost_perlin_fractal_footprint(p.data(), xyz, octaves, s, bias, fade ? 1 : 0, nullptr);
    }
    double turb_footprint_gradient(const point3 &q, float s, double grad[3], int depth = 7, float bias = 0.0f, bool fade = false) const
    {
        const float xyz[3] = {q.x(), q.y(), q.z()};
        return wnhost_perlin_turb_footprint(p.data(), xyz, depth, s, bias, fade ? 1 : 0, grad);
    }
    double fractal_noise_footprint_gradient(const point3 &q, float s, double grad[3], int octaves = 6, float bias = 0.0f,
                                            bool fade = false) const
    {
        const float xyz[3] = {q.x(), q.y(), q.z()};
        return wnhost_perlin_fractal_footprint(p.data(), xyz, octaves, s, bias, fade ? 1 : 0, grad);
    }
    // Batched overloads (host pointers, through the GPU): one footprint per point; n doubles to out, or n records
    // {value, d/dx, d/dy, d/dz} of four doubles to out4.
    void turb_footprint(const float *xyz, const float *s, size_t n, double *out, int depth = 7, float bias = 0.0f, bool fade = false) const
    {
        footprint_vec3(xyz, s, n, 0, depth, bias, fade, out);
    }
    void fractal_noise_footprint(const float *xyz, const float *s, size_t n, double *out, int octaves = 6, float bias = 0.0f,
                                 bool fade = false) const
    {
        footprint_vec3(xyz, s, n, 1, octaves, bias, fade, out);
    }
    void turb_footprint_gradient(const float *xyz, const float *s, size_t n, double *out4, int depth = 7, float bias = 0.0f,
                                 bool fade = false) const
    {
        footprint_vec3(xyz, s, n, 2, depth, bias, fade, out4);
    }
    void fractal_noise_footprint_gradient(const float *xyz, const float *s, size_t n, double *out4, int octaves = 6,
                                          float bias = 0.0f, bool fade = false) const
    {
        footprint_vec3(xyz, s, n, 3, octaves, bias, fade, out4);
    }

    const std::vector<int> &table() const { return p; }
    const wn_perm *perm() const { return perm_; }

  private:
    void grad_vec3(const float *xyz, size_t n, int kind, int depth, double *out4) const // kind 0: noise, 1: turb, 2: fractal_noise
    {
        if (!n) return;
        wnhost::DeviceBuffer in(3 * n * sizeof(float)), res(4 * n * sizeof(double));
        in.upload(xyz);
        if (kind == 0) wnhost::check(wn_perlin_grad_points_vec3(perm_, in.as<float>(), n, res.as<double>(), nullptr), "wn_perlin_grad_points_vec3");
        else if (kind == 1) wnhost::check(wn_perlin_turb_grad_points(perm_, in.as<float>(), n, depth, res.as<double>(), nullptr), "wn_perlin_turb_grad_points");
        else wnhost::check(wn_perlin_fractal_grad_points(perm_, in.as<float>(), n, res.as<double>(), nullptr), "wn_perlin_fractal_grad_points");
        res.download(out4);
    }
    // kind 0: turb, 1: fractal_noise, 2 / 3: their gradients
    void footprint_vec3(const float *xyz, const float *s, size_t n, int kind, int octaves, float bias, bool fade, double *out) const
    {
        if (!n) return;
        wnhost::DeviceBuffer in(3 * n * sizeof(float)), fp(n * sizeof(float)), res((kind >= 2 ? 4 : 1) * n * sizeof(double));
        in.upload(xyz);
        fp.upload(s);
        const int f = fade ? 1 : 0;
        if (kind == 0) wnhost::check(wn_perlin_turb_footprint_points(perm_, in.as<float>(), fp.as<float>(), n, octaves, bias, f, res.as<double>(), nullptr), "wn_perlin_turb_footprint_points");
        else if (kind == 1) wnhost::check(wn_perlin_fractal_footprint_points(perm_, in.as<float>(), fp.as<float>(), n, octaves, bias, f, res.as<double>(), nullptr), "wn_perlin_fractal_footprint_points");
        else if (kind == 2) wnhost::check(wn_perlin_turb_footprint_grad_points(perm_, in.as<float>(), fp.as<float>(), n, octaves, bias, f, res.as<double>(), nullptr), "wn_perlin_turb_footprint_grad_points");
        else wnhost::check(wn_perlin_fractal_footprint_grad_points(perm_, in.as<float>(), fp.as<float>(), n, octaves, bias, f, res.as<double>(), nullptr), "wn_perlin_fractal_footprint_grad_points");
        res.download(out);
    }
    static const int *curl_offsets_int(const int *offsets9) { return offsets9 ? offsets9 : default_curl_offsets(); }
    static const int32_t *curl_offsets(const int *offsets9)
    {
        static_assert(sizeof(int) == sizeof(int32_t), "offsets are int32");
        return reinterpret_cast<const int32_t *>(offsets9 ? offsets9 : default_curl_offsets());
    }
    void curl_vec3(const float *xyz, size_t n, int kind, int depth, const int *offsets9, double *out3) const
    {
        if (!n) return;
        wnhost::DeviceBuffer in(3 * n * sizeof(float)), res(3 * n * sizeof(double));
        in.upload(xyz);
        wnhost::check(wn_perlin_curl_points_vec3(perm_, in.as<float>(), n, kind, depth, curl_offsets(offsets9), res.as<double>(), nullptr),
                      "wn_perlin_curl_points_vec3");
        res.download(out3);
    }
};

#endif
