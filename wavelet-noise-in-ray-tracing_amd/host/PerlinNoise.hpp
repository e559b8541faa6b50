// PerlinNoise.hpp -- the reference's experient/PerlinNoise.hpp:9-61 (the same improved-noise
// algorithm as perlin.h with an explicit seed and no vec3 overloads) over the MI355X C ABI.
#ifndef PERLINNOISE_HPP
#define PERLINNOISE_HPP

#include <cstddef>
#include <random>
#include <vector>

#include "scalar_eval.h"
#include "wn_host.hpp"
#include "wnoise_perlin_advect.h"
#include "wnoise_perlin_bounded.h"
#include "wnoise_perlin_curl.h"

class PerlinNoise {
  private:
    std::vector<int> p;
    wn_perm *perm_ = nullptr;

  public:
    explicit PerlinNoise(unsigned int seed = std::mt19937::default_seed) : p(512)
    {
        wnhost::check(wn_perm_create_seeded(seed, &perm_), "wn_perm_create_seeded");
        wnhost::check(wn_perm_download(perm_, p.data()), "wn_perm_download");
    }
    ~PerlinNoise() { wn_perm_destroy(perm_); }
    PerlinNoise(const PerlinNoise &) = delete;
    PerlinNoise &operator=(const PerlinNoise &) = delete;

    double noise(double x, double y, double z) const // PerlinNoise.hpp:36-56
    {
        if (!wnhost_scalar_on_device()) return wnhost_perlin(p.data(), x, y, z); // one sample: on the host (scalar_eval.h)
        double v = 0.0;
        wnhost::check(wn_scalar_perlin(perm_, x, y, z, &v), "wn_scalar_perlin");
        return v;
    }
    double noise(double x, double y) const { return noise(x, y, 0.0); } // PerlinNoise.hpp:58-60

    // additive: noise and its analytic gradient (absent from the reference; include/wnoise.h).  The scalar member is
    // evaluated on the host and returns the value, d/dx, d/dy, d/dz to grad; the batched overload writes n records
    // {value, d/dx, d/dy, d/dz} of four doubles through the GPU.  Bit-identical to each other.
    double noise_gradient(double x, double y, double z, double grad[3]) const { return wnhost_perlin_grad(p.data(), x, y, z, grad); }
    void noise_gradient(const double *xyz, size_t n, double *out4) const
    {
        if (!n) return;
        wnhost::DeviceBuffer in(3 * n * sizeof(double)), res(4 * n * sizeof(double));
        in.upload(xyz);
        wnhost::check(wn_perlin_grad_points(perm_, in.as<double>(), n, res.as<double>(), nullptr), "wn_perlin_grad_points");
        res.download(out4);
    }

    // additive: the curl of three noise potentials on cells shifted by offsets9 (include/wnoise_perlin_curl.h; NULL:
    // (0,0,0), (85,85,85), (170,170,170), a default only).  Scalar on the host, batched (n records {vx, vy, vz} of three
    // doubles) through the GPU; bit-identical to each other.
    void noise_curl(double x, double y, double z, double v[3], const int *offsets9 = nullptr) const
    {
        wnhost_perlin_curl(p.data(), x, y, z, curl_offsets(offsets9), v);
    }
    void noise_curl(const double *xyz, size_t n, double *out3, const int *offsets9 = nullptr) const
    {
        if (!n) return;
        wnhost::DeviceBuffer in(3 * n * sizeof(double)), res(3 * n * sizeof(double));
        in.upload(xyz);
        static_assert(sizeof(int) == sizeof(int32_t), "offsets are int32");
        wnhost::check(wn_perlin_curl_points(perm_, in.as<double>(), n, reinterpret_cast<const int32_t *>(curl_offsets(offsets9)),
                                            res.as<double>(), nullptr), "wn_perlin_curl_points");
        res.download(out3);
    }

    // additive: particles moved through that curl field (include/wnoise_perlin_advect.h, whose wn_advect `a` is: method,
    // steps, h, gain, drift, traj_every); this class serves noise_curl only, so the potentials are WN_PERLIN_CURL_NOISE.
    // With a.traj_every = e >= 1 the positions after steps 0, e, 2e, ... go to traj ([snapshot][n][3]).  Scalar traced on
    // the host, batched through the GPU; bit-identical to each other.
    void advect_curl(double x, double y, double z, const wn_advect &a, const int *offsets9, double p_out[3],
                     double *traj = nullptr) const
    {
        const double xyz[3] = {x, y, z};
        if (wnhost_perlin_curl_advect(p.data(), WN_PERLIN_CURL_NOISE, 0, xyz, curl_offsets(offsets9), &a, p_out, traj))
            throw std::runtime_error("advect_curl: a method outside 0..2, negative steps or traj_every, a non-finite h, gain or "
                                     "drift, or a trajectory without a buffer");
    }
    void advect_curl(const double *xyz, size_t n, const wn_advect &a, const int *offsets9, double *xyz_out,
                     double *traj = nullptr) const
    {
        wnhost::perlin_advect_batch(perm_, xyz, n, WN_PERLIN_CURL_NOISE, 0, curl_offsets(offsets9), a, xyz_out, traj);
    }

    // additive: that field with solid boundaries (include/wnoise_perlin_bounded.h; the obstacle list is wnoise_bounded.h's),
    // NOISE potentials only.  curl_potential: Psi; curl_bounded: v = A curl Psi + grad A x Psi; advect_curl_bounded:
    // advect_curl through it.  Scalar on the host, batched through the GPU; bit-identical to each other.
    void curl_potential(double x, double y, double z, double psi[3], const int *offsets9 = nullptr) const
    {
        wnhost_perlin_curl_potential(p.data(), x, y, z, curl_offsets(offsets9), psi);
    }
    void curl_potential(const double *xyz, size_t n, double *out3, const int *offsets9 = nullptr) const
    {
        wnhost::perlin_bounded_points_batch(perm_, xyz, n, WN_PERLIN_CURL_NOISE, 0, curl_offsets(offsets9), nullptr, -1, out3);
    }
    void curl_bounded(double x, double y, double z, const wn_obstacle *obstacles, int nobs, double v[3],
                      const int *offsets9 = nullptr) const
    {
        const double xyz[3] = {x, y, z};
        if (wnhost_perlin_curl_bounded(p.data(), WN_PERLIN_CURL_NOISE, 0, xyz, curl_offsets(offsets9), obstacles, nobs, v))
            throw std::runtime_error("curl_bounded: an obstacle list that include/wnoise_bounded.h refuses");
    }
    void curl_bounded(const double *xyz, size_t n, const wn_obstacle *obstacles, int nobs, double *out3,
                      const int *offsets9 = nullptr) const
    {
        wnhost::perlin_bounded_points_batch(perm_, xyz, n, WN_PERLIN_CURL_NOISE, 0, curl_offsets(offsets9), obstacles,
                                            nobs < 0 ? WN_MAX_OBSTACLES + 1 : nobs, out3);
    }
    void advect_curl_bounded(double x, double y, double z, const wn_advect &a, const int *offsets9, const wn_obstacle *obstacles,
                             int nobs, double p_out[3], double *traj = nullptr) const
    {
        const double xyz[3] = {x, y, z};
        if (wnhost_perlin_curl_bounded_advect(p.data(), WN_PERLIN_CURL_NOISE, 0, xyz, curl_offsets(offsets9), obstacles, nobs, &a,
                                              p_out, traj))
            throw std::runtime_error("advect_curl_bounded: what advect_curl or curl_bounded refuses");
    }
    void advect_curl_bounded(const double *xyz, size_t n, const wn_advect &a, const int *offsets9, const wn_obstacle *obstacles,
                             int nobs, double *xyz_out, double *traj = nullptr) const
    {
        wnhost::perlin_bounded_advect_batch(perm_, xyz, n, WN_PERLIN_CURL_NOISE, 0, curl_offsets(offsets9), obstacles, nobs, a,
                                            xyz_out, traj);
    }

    const std::vector<int> &table() const { return p; }
    const wn_perm *perm() const { return perm_; }

  private:
    static const int *curl_offsets(const int *offsets9)
    {
        static const int o[9] = {0, 0, 0, 85, 85, 85, 170, 170, 170};
        return offsets9 ? offsets9 : o;
    }
};

#endif
