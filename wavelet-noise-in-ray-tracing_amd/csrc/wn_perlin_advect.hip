// wn_perlin_advect.hip -- particles moved through the curl noise of Perlin noise potentials (include/wnoise_perlin_advect.h).
//
// The velocity is wn_perlin_curl.hip's point evaluator, wn::perlin_curl_exact / perlin_turb_curl / perlin_fractal_curl; the
// trace of a particle through a launch (wn::advect_trace, in double) and the chain of launches of a call (wn::advect_chain)
// are wn_advect.hpp's, stated once for every advection kernel and for the host's wnhost_perlin_curl_advect.
//
//   perlin_curl_advect_kernel<KIND, METHOD>   one particle per lane in a grid-stride loop: the permutation table is staged
//                                             in LDS (512 bytes), the position is loaded once, the steps of the launch run
//                                             on registers (position, stage point, RK4's running sum), a trajectory snapshot
//                                             is three 8-byte stores to the time-major address, the final position three
//                                             more.  TURB and FRACTAL round the stage point to float on entry to the
//                                             evaluator, as wn_perlin_curl_points_vec3 is given it.  No LDS beyond the
//                                             table, no private segment.
//
// A launch integrates at most launch_steps() steps; a longer trace is a chain of launches on the stream.
#include "wn_perlin_frame.hpp"
#include "wnoise_perlin_advect.h"

#include <algorithm>
#include <cmath>

namespace {

using wn::kNoise, wn::kTurb, wn::kFractal;
static_assert(WN_PERLIN_CURL_NOISE == kNoise && WN_PERLIN_CURL_TURB == kTurb && WN_PERLIN_CURL_FRACTAL == kFractal,
              "the public kinds are the kernels' kinds");

// A launch on a card that others share must end: a launch integrates at most kPerlinAdvectOctaveBudget octave evaluations
// per particle (one octave of the three potentials at one stage point), whatever the kind and the method.
// Measured on one MI355X, 16 M particles uniform in a 128-cell box (profiles/perlin_advect_kernels.txt): one octave
// evaluation over the list takes 0.39 ms (noise) to 0.416 ms (fractal_noise, the slowest row) inside this kernel, 0.42 ms
// as a wn_perlin_curl_points launch; the time does not depend on where the particles are (no gathers from global memory).
// 50 ms, the figure kAdvectLaunchSteps was sized to, hold 120 of the slowest; 112 = 4 * 28 = 4 * 4 * 7 keeps whole RK4 steps
// of turb's seven octaves together and takes 46.6 ms at most (the longest launch measured: 45.4 ms).  A single step of more
// than 112 octave evaluations (turb with depth > 28 under RK4) is still one launch: its time grows with depth as the point
// launch's does.  A launch boundary costs one 48-byte position round trip per particle, about 0.1 ms on that list.
constexpr int kPerlinAdvectOctaveBudget = 112;

int launch_steps(int kind, int depth, int method)
{
    const long long octaves = kind == kNoise ? 1 : (kind == kTurb ? std::max(depth, 1) : wn::kFractalOctaves);
    return (int)std::max(1LL, kPerlinAdvectOctaveBudget / (wn::advect_stages(method) * octaves));
}

struct PerlinAdvectArgs {
    const uint8_t *perm;
    int off[9]; // (x, y, z) of psi0, psi1, psi2, each in 0..255
    int depth;  // TURB
    wn::AdvectTrace<double, 3> t; // xyz interleaved
};

// amdgpu_waves_per_eu(4): at least the 4 waves per SIMD perlin_curl_points_kernel runs at (121 VGPRs).  Left alone,
// <fractal, RK4> takes 165 VGPRs, 3 waves, and measured 1.003 x the 64 point launches it replaces; held to 128 (126, still
// without a private segment) it measures 0.989 x, and the turb rows gain 1 % with it (profiles/perlin_advect_kernels.txt).
template <int KIND, int METHOD>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void perlin_curl_advect_kernel(const PerlinAdvectArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_perm[512];
    wn::load_perm_lds(s_perm, a.perm);
    const uint8_t *perm = s_perm;
    const auto velocity = [&](const double q[3], double v[3]) {
        if (KIND == kNoise) wn::perlin_curl_exact(perm, q[0], q[1], q[2], a.off, v);
        else if (KIND == kTurb) wn::perlin_turb_curl(perm, (float)q[0], (float)q[1], (float)q[2], a.depth, a.off, v);
        else wn::perlin_fractal_curl(perm, (float)q[0], (float)q[1], (float)q[2], a.off, v);
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

int advect_points(const wn_perm *perm, const double *in_dev, size_t n, int kind, int depth, const int32_t *offsets9_host,
                  const wn_advect *adv, double *out_dev, double *traj_dev, hipStream_t stream)
{
    // kind, depth and perm as wn_perlin_curl_points_vec3 checks them
    if (kind < kNoise || kind > kFractal) return wn::fail(WN_ERR_INVALID, "kind must be 0 (noise), 1 (turb) or 2 (fractal_noise)");
    if (kind == kTurb && depth < 0) return wn::fail(WN_ERR_INVALID, "depth must be >= 0");
    int rc = wn::check_perm(perm, "perlin curl advect points");
    if (rc) return rc;
    rc = wn::check_advect(adv);
    if (rc || n == 0) return rc;
    if (!offsets9_host) return wn::fail(WN_ERR_INVALID, "offsets9_host is NULL");
    rc = wn::check_advect_buffers<double, 3>(in_dev, out_dev, traj_dev, n, adv->traj_every, "xyz_in_dev", "xyz_out_dev");
    if (rc) return rc;

    PerlinAdvectArgs a{};
    a.perm = perm->dev;
    for (int i = 0; i < 9; ++i) a.off[i] = offsets9_host[i] & 255;
    a.depth = depth;
    const dim3 grid = dim3(wn::stride_blocks(n)), block(256);
    const auto launch_one = [&](const wn::AdvectTrace<double, 3> &t) -> int {
        a.t = t;
        wn::with_advect_method(adv->method, [&](auto method) {
            constexpr int kMethod = decltype(method)::value;
            if (kind == kNoise) hipLaunchKernelGGL((perlin_curl_advect_kernel<kNoise, kMethod>), grid, block, 0, stream, a);
            else if (kind == kTurb) hipLaunchKernelGGL((perlin_curl_advect_kernel<kTurb, kMethod>), grid, block, 0, stream, a);
            else hipLaunchKernelGGL((perlin_curl_advect_kernel<kFractal, kMethod>), grid, block, 0, stream, a);
        });
        WN_LAUNCH_CHECK("perlin_curl_advect_kernel");
        return WN_OK;
    };
    return wn::advect_chain(wn::advect_trace_fill<double, 3>(*adv, n), in_dev, out_dev, traj_dev, adv->steps,
                            launch_steps(kind, depth, adv->method), launch_one);
}

} // namespace

extern "C" {

int wn_perlin_curl_advect_points(const wn_perm *perm, const double *xyz_in_dev, size_t n, int kind, int depth,
                                 const int32_t *offsets9_host, const wn_advect *a, double *xyz_out_dev, double *traj_dev,
                                 void *stream)
{
    WN_ENTRY();
    return advect_points(perm, xyz_in_dev, n, kind, depth, offsets9_host, a, xyz_out_dev, traj_dev, wn::as_stream(stream));
}

int wn_perlin_advect_launch_steps(int kind, int depth, int method) { return launch_steps(kind, depth, method); }

} // extern "C"
