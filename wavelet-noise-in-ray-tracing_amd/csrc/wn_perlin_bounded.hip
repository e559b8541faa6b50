// wn_perlin_bounded.hip -- the curl noise of Perlin noise potentials with solid boundaries, on point lists and under particle
// advection, and the potential values themselves (include/wnoise_perlin_bounded.h).
//
// The velocity is wn::perlin_curl_bounded and the values are wn::perlin_curl_potential (wn_eval.hpp), stated once for these
// kernels and for the host's wnhost_perlin_curl_bounded / wnhost_perlin_*curl_potential; a particle's trace through a launch
// and the chain of launches are wn_advect.hpp's (wn::advect_trace, wn::advect_chain).
//
//   perlin_potential_points_kernel               one point per lane in a grid-stride loop, records {psi0, psi1, psi2}.
//   perlin_curl_bounded_points_kernel<KIND>      the same, records {vx, vy, vz}.
//   perlin_curl_bounded_advect_kernel<KIND, M>   perlin_curl_advect_kernel's shape: the position is loaded once, the steps of
//                                                the launch run on registers, a snapshot is three 8-byte stores.
//
// Every kernel stages the permutation table in LDS (512 bytes) and has no private segment.  The obstacle list travels by
// value in the launch arguments (wn_obstacles.hpp; 16 x 32 bytes): it is the same for every lane, so the ramp's loop reads it
// with scalar loads and branches on the kind as a wave.  Per point or stage the ramp comes first; a lane that is inside
// evaluates nothing, every other lane takes ONE walk over the octaves, which gives the curl and Psi together (the value is
// perlin_sample_grad's return, two lerps beside the partials), so a near lane costs what a far lane costs plus the
// composition.  nobs == 0 launches the unbounded kernels through their entry points.
//
// A launch integrates at most launch_steps() steps; a longer trace is a chain of launches on the stream.
#include "wn_obstacles.hpp"
#include "wn_perlin_frame.hpp"
#include "wnoise_perlin_bounded.h"

#include <algorithm>
#include <cmath>

namespace {

using wn::kNoise, wn::kTurb, wn::kFractal;
using wn::Obstacles;
static_assert(WN_PERLIN_CURL_NOISE == kNoise && WN_PERLIN_CURL_TURB == kTurb && WN_PERLIN_CURL_FRACTAL == kFractal,
              "the public kinds are the kernels' kinds");

// A launch on a card that others share must end.  wn_perlin_advect.hip sized its budget of octave evaluations per particle
// and launch (kPerlinAdvectOctaveBudget) to 50 ms on 16 M particles; here a stage also pays the ramp, a double square root
// and several double divisions per obstacle, so a stage counts as octaves + ceil(kappa * nobs) octave evaluations, kappa
// being the cost of one obstacle's ramp in octave evaluations.
// Measured on one MI355X, 16 M particles uniform in a 128-cell box, RK4, 16 steps (profiles/perlin_bounded_kernels.txt):
// particles far from 16 obstacles against particles far from 1 give 0.0435 to 0.045 ms per obstacle and stage, beside
// 0.389 (noise) to 0.416 ms (fractal_noise) per octave evaluation: kappa = 0.107 to 0.112.  1 / 8 is kept: a stage is then
// never counted cheaper than it is, and the longest launch measured with it is recorded in that file.
constexpr double kRampKappa = 0.125;

int launch_steps(int kind, int depth, int method, int nobs)
{
    if (nobs == 0) return wn_perlin_advect_launch_steps(kind, depth, method);
    // the unbounded rule is budget / (stages * octaves): one stage of one octave gives the budget itself
    const long long budget = wn_perlin_advect_launch_steps(WN_PERLIN_CURL_NOISE, 0, WN_ADVECT_EULER);
    const long long octaves = kind == kNoise ? 1 : (kind == kTurb ? std::max(depth, 1) : wn::kFractalOctaves);
    const int counted = (nobs < 0 || nobs > WN_MAX_OBSTACLES) ? WN_MAX_OBSTACLES : nobs;
    const long long ramp = (long long)std::ceil(kRampKappa * counted);
    return (int)std::max(1LL, budget / (wn::advect_stages(method) * (octaves + ramp)));
}

struct Offsets {
    int o[9]; // (x, y, z) of psi0, psi1, psi2, each in 0..255
};

struct PotentialPointsArgs {
    const uint8_t *perm;
    const double *pts64;
    const float *pts32;
    double *out; // n records {psi0, psi1, psi2}
    size_t count;
    Offsets off;
    int kind, depth;
};

struct BoundedPointsArgs {
    const uint8_t *perm;
    const double *pts64; // NOISE only
    const float *pts32;
    double *out; // n records {vx, vy, vz}
    size_t count;
    Offsets off;
    int depth;
    Obstacles o;
};

struct BoundedAdvectArgs {
    const uint8_t *perm;
    Offsets off;
    int depth; // TURB
    Obstacles o;
    wn::AdvectTrace<double, 3> t; // xyz interleaved
};

__global__ __launch_bounds__(256) void perlin_potential_points_kernel(const PotentialPointsArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_perm[512];
    wn::load_perm_lds(s_perm, a.perm);
    const uint8_t *perm = s_perm;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.count; i += (size_t)gridDim.x * blockDim.x) {
        double psi[3];
        if (a.pts64) {
            const double *p = a.pts64 + 3 * i;
            wn::perlin_curl_potential<kNoise>(perm, p[0], p[1], p[2], 0, a.off.o, psi);
        } else {
            const float *p = a.pts32 + 3 * i;
            if (a.kind == kNoise) wn::perlin_curl_potential<kNoise>(perm, p[0], p[1], p[2], 0, a.off.o, psi);
            else if (a.kind == kTurb) wn::perlin_curl_potential<kTurb>(perm, p[0], p[1], p[2], a.depth, a.off.o, psi);
            else wn::perlin_curl_potential<kFractal>(perm, p[0], p[1], p[2], 0, a.off.o, psi);
        }
        double *const rec = a.out + 3 * i;
        rec[0] = psi[0];
        rec[1] = psi[1];
        rec[2] = psi[2];
    }
}

template <int KIND>
__global__ __launch_bounds__(256) void perlin_curl_bounded_points_kernel(const BoundedPointsArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_perm[512];
    wn::load_perm_lds(s_perm, a.perm);
    const uint8_t *perm = s_perm;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.count; i += (size_t)gridDim.x * blockDim.x) {
        double v[3];
        if (KIND == kNoise && a.pts64) {
            const double *p = a.pts64 + 3 * i;
            wn::perlin_curl_bounded<kNoise>(perm, p[0], p[1], p[2], 0, a.off.o, a.o.list, a.o.nobs, v);
        } else {
            const float *p = a.pts32 + 3 * i;
            wn::perlin_curl_bounded<KIND>(perm, p[0], p[1], p[2], a.depth, a.off.o, a.o.list, a.o.nobs, v);
        }
        double *const rec = a.out + 3 * i;
        rec[0] = v[0];
        rec[1] = v[1];
        rec[2] = v[2];
    }
}

// amdgpu_waves_per_eu, from the compiled register counts (gfx950; tests/test_perlin_bounded_register_budget.py prints them,
// profiles/perlin_bounded_kernels.txt records them).  The kernel carries A, G and Psi (10 doubles) across the walk beside what
// perlin_curl_advect_kernel holds.  Held to 4 waves per SIMD (128 VGPRs) as that kernel is, Euler and midpoint fit, 97 to 127
// VGPRs, and so does <noise, RK4> (124); <turb, RK4> and <fractal_noise, RK4> do not: they get a private segment of 48 and 72
// bytes.  Those two are held to 3 waves instead and take 138 and 150 VGPRs with no private segment.
constexpr int advect_waves(int kind, int method) { return (method == WN_ADVECT_RK4 && kind != kNoise) ? 3 : 4; }

template <int KIND, int METHOD>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(advect_waves(KIND, METHOD)))) void perlin_curl_bounded_advect_kernel(const BoundedAdvectArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_perm[512];
    wn::load_perm_lds(s_perm, a.perm);
    const uint8_t *perm = s_perm;
    const auto velocity = [&](const double q[3], double v[3]) {
        if (KIND == kNoise) wn::perlin_curl_bounded<kNoise>(perm, q[0], q[1], q[2], 0, a.off.o, a.o.list, a.o.nobs, v);
        else wn::perlin_curl_bounded<KIND>(perm, (float)q[0], (float)q[1], (float)q[2], a.depth, a.off.o, a.o.list, a.o.nobs, v);
    };
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.t.count; i += (size_t)gridDim.x * blockDim.x) {
        double p[3] = {a.t.in[3 * i], a.t.in[3 * i + 1], a.t.in[3 * i + 2]};
        wn::advect_trace<METHOD>(a.t, p, 3 * i, velocity, [&](double *dst) {
            dst[0] = p[0];
            dst[1] = p[1];
            dst[2] = p[2];
        });
    }
}

// kind and depth as wn_perlin_curl_points_vec3 checks them
int check_kind(int kind, int depth)
{
    if (kind < kNoise || kind > kFractal) return wn::fail(WN_ERR_INVALID, "kind must be 0 (noise), 1 (turb) or 2 (fractal_noise)");
    if (kind == kTurb && depth < 0) return wn::fail(WN_ERR_INVALID, "depth must be >= 0");
    return WN_OK;
}

Offsets reduce_offsets(const int32_t *offsets9_host)
{
    Offsets off;
    for (int i = 0; i < 9; ++i) off.o[i] = offsets9_host[i] & 255;
    return off;
}

int potential_points(const wn_perm *perm, const double *p64, const float *p32, size_t n, int kind, int depth,
                     const int32_t *offsets9_host, double *out3_dev, void *stream)
{
    int rc = check_kind(kind, depth);
    if (rc) return rc;
    rc = wn::check_perm(perm, "perlin curl potential points");
    if (rc || n == 0) return rc;
    if ((!p64 && !p32) || !out3_dev) return wn::fail(WN_ERR_INVALID, "points/out pointer is NULL");
    if (!offsets9_host) return wn::fail(WN_ERR_INVALID, "offsets9_host is NULL");
    const PotentialPointsArgs a{perm->dev, p64, p32, out3_dev, n, reduce_offsets(offsets9_host), kind, depth};
    hipLaunchKernelGGL(perlin_potential_points_kernel, dim3(wn::stride_blocks(n)), dim3(256), 0, wn::as_stream(stream), a);
    WN_LAUNCH_CHECK("perlin_potential_points_kernel");
    return WN_OK;
}

int bounded_points(const wn_perm *perm, bool vec3, const double *p64, const float *p32, size_t n, int kind, int depth,
                   const int32_t *offsets9_host, const wn_obstacle *obstacles_host, int nobs, double *out3_dev, void *stream)
{
    if (nobs == 0) // no list to check: the unbounded kernel through its entry point, with its checks
        return vec3 ? wn_perlin_curl_points_vec3(perm, p32, n, kind, depth, offsets9_host, out3_dev, stream)
                    : wn_perlin_curl_points(perm, p64, n, offsets9_host, out3_dev, stream);
    int rc = check_kind(kind, depth);
    if (rc) return rc;
    rc = wn::check_perm(perm, "perlin curl bounded points");
    if (rc) return rc;
    BoundedPointsArgs a{};
    rc = wn::obstacle_args(obstacles_host, nobs, "perlin curl bounded points", &a.o);
    if (rc || n == 0) return rc;
    if ((!p64 && !p32) || !out3_dev) return wn::fail(WN_ERR_INVALID, "points/out pointer is NULL");
    if (!offsets9_host) return wn::fail(WN_ERR_INVALID, "offsets9_host is NULL");
    a.perm = perm->dev;
    a.pts64 = p64;
    a.pts32 = p32;
    a.out = out3_dev;
    a.count = n;
    a.off = reduce_offsets(offsets9_host);
    a.depth = depth;
    const dim3 grid(wn::stride_blocks(n)), block(256);
    const hipStream_t s = wn::as_stream(stream);
    if (kind == kNoise) hipLaunchKernelGGL(perlin_curl_bounded_points_kernel<kNoise>, grid, block, 0, s, a);
    else if (kind == kTurb) hipLaunchKernelGGL(perlin_curl_bounded_points_kernel<kTurb>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(perlin_curl_bounded_points_kernel<kFractal>, grid, block, 0, s, a);
    WN_LAUNCH_CHECK("perlin_curl_bounded_points_kernel");
    return WN_OK;
}

int bounded_advect_points(const wn_perm *perm, const double *in_dev, size_t n, int kind, int depth,
                          const int32_t *offsets9_host, const wn_obstacle *obstacles_host, int nobs, const wn_advect *adv,
                          double *out_dev, double *traj_dev, void *stream)
{
    if (nobs == 0) // no list to check: the unbounded kernel through its entry point, with its checks
        return wn_perlin_curl_advect_points(perm, in_dev, n, kind, depth, offsets9_host, adv, out_dev, traj_dev, stream);
    int rc = check_kind(kind, depth);
    if (rc) return rc;
    rc = wn::check_perm(perm, "perlin curl bounded advect points");
    if (rc) return rc;
    BoundedAdvectArgs a{};
    rc = wn::obstacle_args(obstacles_host, nobs, "perlin curl bounded advect points", &a.o);
    if (rc) return rc;
    rc = wn::check_advect(adv);
    if (rc || n == 0) return rc;
    if (!offsets9_host) return wn::fail(WN_ERR_INVALID, "offsets9_host is NULL");
    rc = wn::check_advect_buffers<double, 3>(in_dev, out_dev, traj_dev, n, adv->traj_every, "xyz_in_dev", "xyz_out_dev");
    if (rc) return rc;

    a.perm = perm->dev;
    a.off = reduce_offsets(offsets9_host);
    a.depth = depth;
    const dim3 grid = dim3(wn::stride_blocks(n)), block(256);
    const hipStream_t s = wn::as_stream(stream);
    const auto launch_one = [&](const wn::AdvectTrace<double, 3> &t) -> int {
        a.t = t;
        wn::with_advect_method(adv->method, [&](auto method) {
            constexpr int kMethod = decltype(method)::value;
            if (kind == kNoise) hipLaunchKernelGGL((perlin_curl_bounded_advect_kernel<kNoise, kMethod>), grid, block, 0, s, a);
            else if (kind == kTurb) hipLaunchKernelGGL((perlin_curl_bounded_advect_kernel<kTurb, kMethod>), grid, block, 0, s, a);
            else hipLaunchKernelGGL((perlin_curl_bounded_advect_kernel<kFractal, kMethod>), grid, block, 0, s, a);
        });
        WN_LAUNCH_CHECK("perlin_curl_bounded_advect_kernel");
        return WN_OK;
    };
    return wn::advect_chain(wn::advect_trace_fill<double, 3>(*adv, n), in_dev, out_dev, traj_dev, adv->steps,
                            launch_steps(kind, depth, adv->method, nobs), launch_one);
}

} // namespace

extern "C" {

int wn_perlin_curl_potential_points_f64(const wn_perm *perm, const double *xyz_dev, size_t n, const int32_t *offsets9_host,
                                    double *out3_dev, void *stream)
{
    WN_ENTRY();
    return potential_points(perm, xyz_dev, nullptr, n, kNoise, 0, offsets9_host, out3_dev, stream);
}

int wn_perlin_curl_potential_points_f32(const wn_perm *perm, const float *xyz_dev, size_t n, int kind, int depth,
                                         const int32_t *offsets9_host, double *out3_dev, void *stream)
{
    WN_ENTRY();
    return potential_points(perm, nullptr, xyz_dev, n, kind, depth, offsets9_host, out3_dev, stream);
}

int wn_perlin_curl_bounded_points_f64(const wn_perm *perm, const double *xyz_dev, size_t n, const int32_t *offsets9_host,
                                  const wn_obstacle *obstacles_host, int nobs, double *out3_dev, void *stream)
{
    WN_ENTRY();
    return bounded_points(perm, false, xyz_dev, nullptr, n, kNoise, 0, offsets9_host, obstacles_host, nobs, out3_dev, stream);
}

int wn_perlin_curl_bounded_points_f32(const wn_perm *perm, const float *xyz_dev, size_t n, int kind, int depth,
                                       const int32_t *offsets9_host, const wn_obstacle *obstacles_host, int nobs,
                                       double *out3_dev, void *stream)
{
    WN_ENTRY();
    return bounded_points(perm, true, nullptr, xyz_dev, n, kind, depth, offsets9_host, obstacles_host, nobs, out3_dev, stream);
}

int wn_perlin_curl_bounded_advect_points_f64(const wn_perm *perm, const double *xyz_in_dev, size_t n, int kind, int depth,
                                         const int32_t *offsets9_host, const wn_obstacle *obstacles_host, int nobs,
                                         const wn_advect *a, double *xyz_out_dev, double *traj_dev, void *stream)
{
    WN_ENTRY();
    return bounded_advect_points(perm, xyz_in_dev, n, kind, depth, offsets9_host, obstacles_host, nobs, a, xyz_out_dev,
                                 traj_dev, stream);
}

int wn_perlin_bounded_advect_launch_steps(int kind, int depth, int method, int nobs)
{
    return launch_steps(kind, depth, method, nobs);
}

} // extern "C"
