// wn_host.hpp -- glue shared by the host classes: error translation, a per-thread pinned scratch
// (batch-of-one calls for the few members without a wn_scalar_* entry point) and a device buffer.
//
// Everything that takes more than one sample -- point lists, textures' values(), dense grids, tile generation -- runs on
// the GPU through libwnoise_hip.so (include/wnoise.h); a failing ABI call (most commonly: no HIP device) throws
// std::runtime_error with wn_last_error(), nothing falls back to the CPU.  Only the reference's scalar members (one sample
// per call) are evaluated on the host (scalar_eval.h), from the mirrors the classes already keep.
#pragma once

#include <cstddef>
#include <stdexcept>
#include <string>

#include "wnoise.h"
#include "wnoise_perlin_advect.h"
#include "wnoise_perlin_bounded.h"

namespace wnhost {

inline void check(int rc, const char *what)
{
    if (rc != WN_OK) throw std::runtime_error(std::string(what) + ": " + wn_last_error());
}

// Pinned, device-mapped staging for batch-of-one calls (WMultibandNoise): the kernel reads the point from and
// writes the result to host memory, so such a call is launch + sync, with no memcpy calls.  The reference's own
// scalar members (evaluate*, noise, value) are evaluated on the host (scalar_eval.h) or, with WN_SCALAR_ON_DEVICE=1, by the
// resident scalar kernel (wn_scalar_*, include/wnoise.h).
class Scratch {
  public:
    static Scratch &get()
    {
        thread_local Scratch s;
        return s;
    }
    float *in_host() { return reinterpret_cast<float *>(host_); }
    double *in_host64() { return reinterpret_cast<double *>(host_); }
    float *out_host() { return reinterpret_cast<float *>(host_ + kIn); }
    double *out_host64() { return reinterpret_cast<double *>(host_ + kIn); }
    void *in_dev() { return dev_; }
    void *out_dev() { return dev_ + kIn; }
    Scratch(const Scratch &) = delete;
    Scratch &operator=(const Scratch &) = delete;

  private:
    static constexpr size_t kIn = 64, kBytes = 128;
    Scratch()
    {
        void *h = nullptr, *d = nullptr;
        check(wn_host_alloc_mapped(&h, &d, kBytes), "wn_host_alloc_mapped");
        host_ = static_cast<char *>(h);
        dev_ = static_cast<char *>(d);
    }
    ~Scratch() { wn_host_free_mapped(host_); }
    char *host_ = nullptr, *dev_ = nullptr;
};

// Device buffer for the batched host-pointer overloads.
class DeviceBuffer {
  public:
    explicit DeviceBuffer(size_t bytes) : bytes_(bytes) { check(wn_dev_alloc(&p_, bytes), "wn_dev_alloc"); }
    ~DeviceBuffer() { wn_dev_free(p_); }
    void *get() const { return p_; }
    template <typename T> T *as() const { return static_cast<T *>(p_); }
    void upload(const void *src) { check(wn_copy_h2d(p_, src, bytes_, nullptr), "wn_copy_h2d"); }
    void download(void *dst) const
    {
        check(wn_copy_d2h(dst, p_, bytes_, nullptr), "wn_copy_d2h");
        check(wn_stream_sync(nullptr), "wn_stream_sync");
    }
    DeviceBuffer(const DeviceBuffer &) = delete;
    DeviceBuffer &operator=(const DeviceBuffer &) = delete;

  private:
    void *p_ = nullptr;
    size_t bytes_;
};

// The batched advect_curl members of perlin and PerlinNoise (host pointers): one call of wn_perlin_curl_advect_points, in
// place on the device; the trajectory buffer exists only when a.traj_every asks for it and traj is given.
inline void perlin_advect_batch(const wn_perm *perm, const double *xyz, size_t n, int kind, int depth, const int *offsets9,
                                const wn_advect &a, double *xyz_out, double *traj)
{
    static_assert(sizeof(int) == sizeof(int32_t), "offsets are int32");
    if (!n) return;
    const bool snaps = a.traj_every >= 1 && a.steps >= 0 && traj;
    const size_t traj_bytes = snaps ? ((size_t)(a.steps / a.traj_every) + 1) * 3 * n * sizeof(double) : 0;
    DeviceBuffer pos(3 * n * sizeof(double)), path(traj_bytes ? traj_bytes : sizeof(double));
    pos.upload(xyz);
    check(wn_perlin_curl_advect_points(perm, pos.as<double>(), n, kind, depth, reinterpret_cast<const int32_t *>(offsets9), &a,
                                       pos.as<double>(), snaps ? path.as<double>() : nullptr, nullptr),
          "wn_perlin_curl_advect_points");
    if (snaps) check(wn_copy_d2h(traj, path.get(), traj_bytes, nullptr), "wn_copy_d2h");
    pos.download(xyz_out);
}

// The batched advect_curl_bounded members of perlin and PerlinNoise: perlin_advect_batch around
// wn_perlin_curl_bounded_advect_points_f64 (include/wnoise_perlin_bounded.h).
inline void perlin_bounded_advect_batch(const wn_perm *perm, const double *xyz, size_t n, int kind, int depth, const int *offsets9,
                                        const wn_obstacle *obstacles, int nobs, const wn_advect &a, double *xyz_out, double *traj)
{
    if (!n) return;
    const bool snaps = a.traj_every >= 1 && a.steps >= 0 && traj;
    const size_t traj_bytes = snaps ? ((size_t)(a.steps / a.traj_every) + 1) * 3 * n * sizeof(double) : 0;
    DeviceBuffer pos(3 * n * sizeof(double)), path(traj_bytes ? traj_bytes : sizeof(double));
    pos.upload(xyz);
    check(wn_perlin_curl_bounded_advect_points_f64(perm, pos.as<double>(), n, kind, depth, reinterpret_cast<const int32_t *>(offsets9),
                                               obstacles, nobs, &a, pos.as<double>(), snaps ? path.as<double>() : nullptr, nullptr),
          "wn_perlin_curl_bounded_advect_points_f64");
    if (snaps) check(wn_copy_d2h(traj, path.get(), traj_bytes, nullptr), "wn_copy_d2h");
    pos.download(xyz_out);
}

// The batched curl_potential and curl_bounded members (host pointers): n points of three T (double: the NOISE entry points on
// doubles; float: the _vec3 ones) in, n records of three doubles out.  obstacles == nullptr with nobs < 0: the potential
// values; otherwise the bounded velocity.
template <typename T>
inline void perlin_bounded_points_batch(const wn_perm *perm, const T *xyz, size_t n, int kind, int depth, const int *offsets9,
                                        const wn_obstacle *obstacles, int nobs, double *out3)
{
    if (!n) return;
    DeviceBuffer in(3 * n * sizeof(T)), res(3 * n * sizeof(double));
    in.upload(xyz);
    const int32_t *off = reinterpret_cast<const int32_t *>(offsets9);
    if constexpr (sizeof(T) == sizeof(double)) {
        if (nobs < 0) check(wn_perlin_curl_potential_points_f64(perm, in.as<double>(), n, off, res.as<double>(), nullptr), "wn_perlin_curl_potential_points_f64");
        else check(wn_perlin_curl_bounded_points_f64(perm, in.as<double>(), n, off, obstacles, nobs, res.as<double>(), nullptr), "wn_perlin_curl_bounded_points_f64");
    } else {
        if (nobs < 0) check(wn_perlin_curl_potential_points_f32(perm, in.as<float>(), n, kind, depth, off, res.as<double>(), nullptr), "wn_perlin_curl_potential_points_f32");
        else check(wn_perlin_curl_bounded_points_f32(perm, in.as<float>(), n, kind, depth, off, obstacles, nobs, res.as<double>(), nullptr), "wn_perlin_curl_bounded_points_f32");
    }
    res.download(out3);
}

} // namespace wnhost
