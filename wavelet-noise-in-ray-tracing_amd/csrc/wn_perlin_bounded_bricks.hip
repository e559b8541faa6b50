// wn_perlin_bounded_bricks.hip -- curl brick lists of Perlin noise potentials with solid boundaries for gfx950
// (include/wnoise_perlin_bounded_bricks.h; absent from the reference): the lattices, lists and slots of wn_perlin_curl_bricks
// (wn_perlin_bricks.hip) with the obstacles of include/wnoise_bounded.h and the field of include/wnoise_perlin_bounded.h,
// v = A curl Psi + grad A x Psi, in fp64, unfused: (float) of wn_perlin_curl_bounded_points_f32's record, times out_scale.
//
//   perlin_curl_bounded_bricks_kernel<KIND>   the shape of perlin_bricks_kernel<kCurl, KIND>: one wave per brick, four waves
//                                             per workgroup, lane ly + 8 lz owns a row of 8 x samples, the table and one
//                                             axis slice per wave in LDS, octaves tabulated one at a time (no depth cap),
//                                             two float4 per lane and channel.  The walk is wn_perlin_brick_walk.hpp's.
//
// The obstacle list travels by value in the launch arguments (wn_obstacles.hpp): the same for every lane, read with scalar
// loads.  Per brick, each lane first classifies its 8 samples with wn::obstacle_ramp in double at the samples' float
// coordinates widened (two bits per sample are kept; A and G are formed again at the finish, by the same function and so
// with the same bits, instead of living through the walk in 64 registers), and the wave votes.  Every branch on the vote
// is wave-uniform:
//     no sample outside a solid    (float)0.0 * out_scale is stored and the octave loop is skipped;
//     no near sample               the 6-sum walk (kCurl): exactly the unbounded kernel's work and bits;
//     otherwise                    the 9-sum walk (kCurlPsi): the six partials and the three potential values, as
//                                  wn::perlin_curl_octave<.., VALUES = true> accumulates them, over the row's two halves of
//                                  four samples one after the other; a half votes again, and one without a near sample
//                                  takes the 6-sum walk on its four samples (wholly inside: none).
// The finish takes one sample at a time through wn::bounded_velocity around wn::perlin_curl_of -- the functions the point
// kernel (wn_perlin_bounded.hip) and the host twin compile -- then (float)v * out_scale.
// LDS: kPermBytes + kWaves * kSliceBytes, static.  The sums live in registers; nine sums of eight samples would cost the
// second wave per SIMD for every brick of the launch, far ones included, so the near walk takes half rows and pays the
// cell's hashes and corner constants twice: register counts, occupancy and timings are in
// profiles/perlin_bounded_bricks_kernels.txt.
#include "wn_obstacles.hpp"
#include "wn_perlin_brick_walk.hpp"
#include "wnoise_perlin_bounded_bricks.h"

namespace {

using wn::GridArgs, wn::BrickRange, wn::kNoise, wn::kTurb, wn::kFractal, wn::kBrickEdge, wn::kBrickSamples;
using wn::BrickAxisSlice, wn::Obstacles;
static_assert(WN_PERLIN_CURL_NOISE == kNoise && WN_PERLIN_CURL_TURB == kTurb && WN_PERLIN_CURL_FRACTAL == kFractal,
              "the public kinds are the kernels' kinds");

constexpr int kWaves = 4;                    // bricks (waves) per workgroup: they share the permutation table
constexpr size_t kBrickBlockCap = 256u * 8u; // workgroups of the brick-stride launch: wn_perlin_bricks.hip's
constexpr int kHalf = kBrickEdge / 2;          // samples per trip of the walk that also sums the potential values
constexpr int kPermBytes = 512;
constexpr int kSliceBytes = 600; // 24 x {f, fade, fade'} + 24 cell bytes
static_assert(sizeof(BrickAxisSlice) == kSliceBytes && kSliceBytes % 8 == 0, "the slice as stated");

struct PerlinBoundedBricksArgs {
    const uint8_t *perm;
    const int32_t *bricks;
    float *out; // 3 consecutive arrays of `count` slots
    size_t count;
    GridArgs g;
    BrickRange range;
    int depth;   // the octaves of the call (wn::perlin_octaves)
    int vec4_ok; // out is 16-byte aligned: so is every slot of every channel
    int off[9];  // (x, y, z) of psi0, psi1, psi2, each in 0..255
    Obstacles o;
};

template <int KIND>
__global__ __launch_bounds__(64 * kWaves) void perlin_curl_bounded_bricks_kernel(const PerlinBoundedBricksArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_perm[kPermBytes];
    __shared__ __attribute__((aligned(8))) BrickAxisSlice s_axis[kWaves];
    const GridArgs &g = a.g;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    wn::run_load_perm(s_perm, a.perm, tid, 64 * kWaves);
    __syncthreads(); // the only barrier: from here on the waves are on their own
    const uint8_t *const perm = s_perm;
    BrickAxisSlice &ax = s_axis[wave];
    const int ly = lane & (kBrickEdge - 1), lz = lane >> 3;
    const float den = (float)g.den;
    const int depth = wn::run_depth<KIND>(a);
    const size_t chan = a.count * kBrickSamples;

    for (size_t i = (size_t)blockIdx.x * kWaves + wave; i < a.count; i += (size_t)gridDim.x * kWaves) {
        const int bx = __builtin_amdgcn_readfirstlane(a.bricks[3 * i]);
        const int by = __builtin_amdgcn_readfirstlane(a.bricks[3 * i + 1]);
        const int bz = __builtin_amdgcn_readfirstlane(a.bricks[3 * i + 2]);
        if (!wn::brick_in_range(a.range, bx, by, bz)) continue; // uniform per wave

        // ---- this lane's 8 samples and their classes: the coordinates the walk tabulates, widened
        const double py = (double)wn::grid_coord(g, den, kBrickEdge * by + ly), pz = (double)wn::grid_coord(g, den, kBrickEdge * bz + lz);
        auto point = [&](int q, double (&p)[3]) {
            p[0] = (double)wn::grid_coord(g, den, kBrickEdge * bx + q);
            p[1] = py;
            p[2] = pz;
        };
        int where = 0; // two bits per sample
        bool lane_near = false;
#pragma unroll
        for (int q = 0; q < kBrickEdge; ++q) {
            double p[3], A, G[3];
            point(q, p);
            const int w = wn::obstacle_ramp(a.o.list, a.o.nobs, p, A, G);
            where |= w << (2 * q);
            lane_near = lane_near || w == wn::kBoundNear;
        }
        const bool wave_open = __ballot(where != wn::kBoundInside * 0x5555) != 0;
        const bool wave_near = __ballot(lane_near) != 0;

        float *const dst = a.out + i * kBrickSamples + lane * kBrickEdge;
        if (!wave_open) {
            float fin[3][kBrickEdge];
            const float zero = (float)0.0 * g.out_scale;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
#pragma unroll
                for (int q = 0; q < kBrickEdge; ++q) fin[ch][q] = zero;
            wn::perlin_brick_store(dst, chan, a.vec4_ok, fin);
            continue;
        }

        // one sample's velocity from its six partials c (after fractal_noise's division) and, near a solid, its values
        auto finish = [&](int w, double A, const double (&G)[3], const double *c, auto &&values, float (&out)[3]) {
            double v[3];
            wn::bounded_velocity(w, A, G, v, [&](double *curl) { wn::perlin_curl_of(c, curl); }, values);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) out[ch] = (float)v[ch] * g.out_scale;
        };

        if (!wave_near) {
            // far and inside samples only: the unbounded walk; the classes are the ballot's
            float fin[3][kBrickEdge];
            double s[6][kBrickEdge], amp_sum;
            wn::perlin_brick_walk<wn::kCurl, KIND>(perm, ax, g, den, a.off, depth, lane, ly, lz, bx, by, bz, s, amp_sum);
#pragma unroll
            for (int q = 0; q < kBrickEdge; ++q) {
                double c[6];
#pragma unroll
                for (int j = 0; j < 6; ++j) c[j] = (KIND == kFractal) ? s[j][q] / amp_sum : s[j][q];
                const double G[3] = {0.0, 0.0, 0.0};
                const bool inside = ((where >> (2 * q)) & 3) == wn::kBoundInside;
                float out[3];
                finish(inside ? wn::kBoundInside : wn::kBoundFar, 1.0, G, c, [](double *) {}, out); // no near sample: no values
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) fin[ch][q] = out[ch];
                __builtin_amdgcn_sched_barrier(0); // one sample's divisions at a time
            }
            wn::perlin_brick_store(dst, chan, a.vec4_ok, fin);
            continue;
        }

        // a near sample in the wave: the row's two halves of kHalf samples one after the other, each by its own ballots.  A
        // half with a near sample takes the 9-sum walk, whose sums take 9 x 4 register pairs and not 9 x 8
        // (profiles/perlin_bounded_bricks_kernels.txt); a half without one the 6-sum walk on its four samples, and a half
        // wholly inside a solid none.  A half's samples leave as one float4 per channel.
#pragma nounroll
        for (int q0 = 0; q0 < kBrickEdge; q0 += kHalf) {
            const int mine = (where >> (2 * q0)) & 0xff;                    // this lane's four classes of the half
            const bool half_open = __ballot(mine != wn::kBoundInside * 0x55) != 0;
            const bool half_near = __ballot((mine & (wn::kBoundNear * 0x55)) != 0) != 0;
            float fin[3][kHalf];
            if (!half_open) {
                const float zero = (float)0.0 * g.out_scale;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch)
#pragma unroll
                    for (int q = 0; q < kHalf; ++q) fin[ch][q] = zero;
            } else if (!half_near) {
                double s[6][kHalf], amp_sum;
                wn::perlin_brick_walk<wn::kCurl, KIND, kHalf>(perm, ax, g, den, a.off, depth, lane, ly, lz, bx, by, bz, s, amp_sum, q0);
#pragma unroll
                for (int q = 0; q < kHalf; ++q) {
                    double c[6];
#pragma unroll
                    for (int j = 0; j < 6; ++j) c[j] = (KIND == kFractal) ? s[j][q] / amp_sum : s[j][q];
                    const double G[3] = {0.0, 0.0, 0.0};
                    const bool inside = ((mine >> (2 * q)) & 3) == wn::kBoundInside;
                    float out[3];
                    finish(inside ? wn::kBoundInside : wn::kBoundFar, 1.0, G, c, [](double *) {}, out);
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) fin[ch][q] = out[ch];
                    __builtin_amdgcn_sched_barrier(0); // one sample's divisions at a time
                }
            } else {
                double s[9][kHalf], amp_sum;
                wn::perlin_brick_walk<wn::kCurlPsi, KIND, kHalf>(perm, ax, g, den, a.off, depth, lane, ly, lz, bx, by, bz, s, amp_sum, q0);
#pragma unroll
                for (int q = 0; q < kHalf; ++q) {
                    double c[9];
#pragma unroll
                    for (int j = 0; j < 9; ++j) c[j] = (KIND == kFractal) ? s[j][q] / amp_sum : s[j][q];
                    double p[3], A, G[3];
                    point(q0 + q, p);
                    const int w = wn::obstacle_ramp(a.o.list, a.o.nobs, p, A, G);
                    float out[3];
                    finish(w, A, G, c, [&](double *psi) {
#pragma unroll
                        for (int k = 0; k < 3; ++k) psi[k] = c[6 + k];
                    }, out);
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) fin[ch][q] = out[ch];
                    __builtin_amdgcn_sched_barrier(0); // one sample's ramp and divisions at a time
                }
            }
            wn::perlin_brick_store4(dst + q0, chan, a.vec4_ok, fin);
        }
    }
}

const void *kernel_of(int kind)
{
    return kind == kNoise  ? reinterpret_cast<const void *>(&perlin_curl_bounded_bricks_kernel<kNoise>)
           : kind == kTurb ? reinterpret_cast<const void *>(&perlin_curl_bounded_bricks_kernel<kTurb>)
                           : reinterpret_cast<const void *>(&perlin_curl_bounded_bricks_kernel<kFractal>);
}

} // namespace

extern "C" {

int wn_perlin_curl_bounded_bricks(const wn_perm *perm, const wn_grid *grid, int kind, int depth, const int32_t *offsets9_host,
                                  const wn_obstacle *obstacles_host, int nobs, const int32_t *bricks_dev, size_t n,
                                  float *out_dev, void *stream)
{
    WN_ENTRY();
    // without a device every call says so, refused ones included (the unbounded call looks for the device at the table)
    int rc = wn::require_device();
    if (rc) return rc;
    // no obstacle: the unbounded call, its checks, its kernels and its bits
    if (nobs == 0) return wn_perlin_curl_bricks(perm, grid, kind, depth, offsets9_host, bricks_dev, n, out_dev, stream);
    // wn_perlin_curl_bricks' checks, in its order and with its messages
    if ((rc = wn::perlin_curl_bricks_checks(perm, grid, kind, depth, offsets9_host)) != WN_OK) return rc;
    PerlinBoundedBricksArgs a{};
    if ((rc = wn::obstacle_args(obstacles_host, nobs, "perlin curl bounded bricks", &a.o)) != WN_OK) return rc;
    wn::BrickListPlan plan;
    bool launch;
    rc = wn::brick_list_plan(grid, bricks_dev, n, 3, out_dev, &plan, &launch);
    if (!launch) return rc;

    a.perm = perm->dev;
    a.bricks = bricks_dev;
    a.out = out_dev;
    a.count = n;
    a.g = plan.g;
    a.range = plan.range;
    a.depth = wn::perlin_octaves(kind, depth);
    a.vec4_ok = (reinterpret_cast<uintptr_t>(out_dev) & 15) == 0;
    for (int i = 0; i < 9; ++i) a.off[i] = offsets9_host[i] & 255;
    const void *const fn = kernel_of(kind);
    void *params[] = {&a};
    const size_t groups = (n + kWaves - 1) / kWaves; // n <= SIZE_MAX / 512: groups * 256 does not overflow
    const hipError_t e = hipLaunchKernel(fn, dim3(wn::stride_blocks(groups * 256, kBrickBlockCap)), dim3(256), params, 0, wn::as_stream(stream));
    if (e != hipSuccess) return wn::hip_fail(e, "perlin_curl_bounded_bricks_kernel");
    WN_LAUNCH_CHECK("perlin_curl_bounded_bricks_kernel");
    return WN_OK;
}

} // extern "C"
