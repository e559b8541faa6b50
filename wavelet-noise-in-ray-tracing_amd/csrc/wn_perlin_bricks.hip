// wn_perlin_bricks.hip -- sparse brick lists of perlin::noise, RTOW turb and perlin::fractal_noise for gfx950: the value,
// the analytic gradient {value, d/dx, d/dy, d/dz} and the curl {vx, vy, vz} of three shifted potentials on a device list of
// 8 x 8 x 8 leaves of the lattices of wn_perlin_grid, wn_perlin_grad_grid and wn_perlin_curl_grid
// (include/wnoise_perlin_bricks.h; absent from the reference).
//
// The run form of wn_perlin_frame.hpp on rows of 8 samples.  What the dense run kernels share along a row of >= 128 samples
// -- a cell's eight hashes and its corner constants -- an 8-sample brick row shares as well; what differs is who owns a row:
//   * one wave per brick, lane l = ly + 8 lz owns the row of 8 x samples at (ly, lz).  Its 8 floats per channel leave as
//     two float4: a wave's stores are one contiguous 2 KiB per channel, straight from registers;
//   * per brick and octave, lanes 0..23 tabulate {f, fade, fade', cell} of the brick's 8 x, 8 y and 8 z indices in the
//     wave's own LDS slice.  A lane keeps a wn::RunOctaveWalker for its index and steps it once per octave, so one octave is
//     tabulated at a time and there is no depth cap;
//   * the 64 lanes of a wave hold 64 different rows, so the per-row {K, mm, t} table of the dense form has nothing to serve:
//     a lane forms its eight corners' entries in registers (wn::run_corner_entries) from its own y and z entries;
//   * the x cells of a brick are the same for all 64 rows, so the walk over the cells a run crosses is WAVE-UNIFORM: the
//     eight hashes are taken once per cell the rows enter (at a step of <= 1/8 cell: once per row and octave, the loop's
//     single trip), and every branch on it is a scalar branch.  y and z cells differ per lane and cost nothing extra;
//   * the running sums of a lane's 8 samples live in registers (1, 4 or 6 sums per sample: value, gradient, curl) in the
//     reference's accumulation order, unfused; the 8 samples are unrolled inside the rolled loop over cells, so the sums
//     are indexed at compile time.
// The field enumerators and the axis slice are wn_perlin_brick_walk.hpp's.  That header also states the walk below (octave
// tabulation, segment loop, per-potential body) as a function template for wn_perlin_bounded_bricks.hip; this file keeps its
// own text of it, because calling the function from here changes the nine kernels' register allocation and schedule
// (profiles/perlin_bounded_bricks_kernels.txt).  A change to one text is a change to both:
// tests/test_perlin_bounded_bricks_host.py compares them.
// LDS: the permutation table of the workgroup and one axis slice per wave (kPermBytes, kSliceBytes below).  Evaluators,
// hashes, corner constants and lerps are those of wn_perlin_frame.hpp / wn_perlin_run.hpp / wn_eval.hpp: fp64, contraction
// off, the bits of the dense grids and of the point entries.
#include "wn_perlin_brick_walk.hpp"
#include "wnoise_perlin_bricks.h"

namespace {

using wn::GridArgs, wn::BrickRange, wn::kNoise, wn::kTurb, wn::kFractal, wn::kBrickEdge, wn::kBrickSamples;
using wn::RunAxisEntryD, wn::BrickAxisSlice, wn::kValue, wn::kGrad, wn::kCurl, wn::field_sums, wn::field_potentials;
static_assert(WN_PERLIN_CURL_NOISE == kNoise && WN_PERLIN_CURL_TURB == kTurb && WN_PERLIN_CURL_FRACTAL == kFractal,
              "the public kinds are the kernels' kinds");

constexpr int field_channels(int field) { return field == kValue ? 1 : (field == kGrad ? 4 : 3); }

constexpr int kWaves = 4;                   // bricks (waves) per workgroup: they share the permutation table
constexpr int kAxisEntries = wn::kBrickAxisEntries;
constexpr size_t kBrickBlockCap = 256u * 8u; // workgroups of the brick-stride launch

constexpr int kPermBytes = 512;
constexpr int kSliceBytes = 600; // 24 x {f, fade, fade'} + 24 cell bytes
static_assert(sizeof(BrickAxisSlice) == kSliceBytes && kSliceBytes % 8 == 0, "the slice as stated");

struct PerlinBricksArgs {
    const uint8_t *perm;
    const int32_t *bricks;
    float *out; // CH consecutive arrays of `count` slots
    size_t count;
    GridArgs g;
    BrickRange range;
    int depth;   // the octaves of the call (wn::perlin_octaves)
    int vec4_ok; // out is 16-byte aligned: so is every slot of every channel
    int off[9];  // curl: (x, y, z) of psi0, psi1, psi2, each in 0..255
};

template <int FIELD, int KIND>
__global__ __launch_bounds__(64 * kWaves) void perlin_bricks_kernel(const PerlinBricksArgs a)
{
    constexpr int CH = field_channels(FIELD), NS = field_sums(FIELD), NP = field_potentials(FIELD);
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

        // lanes 0..23: the walker of axis index lane & 7 of axis lane >> 3 (z indices are absolute: a.g.z0 == 0)
        const int first = (lane < kBrickEdge) ? bx : ((lane < 2 * kBrickEdge) ? by : bz);
        wn::RunOctaveWalker<KIND> walker{wn::grid_coord(g, den, kBrickEdge * first + ly)};

        double s[NS][kBrickEdge]; // the running sums of the row's 8 samples
#pragma unroll
        for (int j = 0; j < NS; ++j)
#pragma unroll
            for (int q = 0; q < kBrickEdge; ++q) s[j][q] = 0.0;
        double amp_sum = 0.0, weight = 1.0; // fractal max_value; turb weight / fractal amplitude

#pragma nounroll
        for (int oc = 0; oc < depth; ++oc) {
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); // the previous octave's (brick's) reads are done
            if (lane < kAxisEntries)
                walker.step([&](int cell, double f) {
                    ax.e[lane] = RunAxisEntryD::of(f);
                    ax.cell[lane] = (uint8_t)cell;
                });
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");

            const RunAxisEntryD ye = ax.e[kBrickEdge + ly], ze = ax.e[2 * kBrickEdge + lz];
            const int Y = ax.cell[kBrickEdge + ly], Z = ax.cell[2 * kBrickEdge + lz];
            const double v = ye.fade, w = ze.fade, dv = ye.dfade, dw = ze.dfade;
            // the 8 x cells: the same for every lane, held on the scalar side
            const uint32_t *const xc = reinterpret_cast<const uint32_t *>(ax.cell);
            const uint64_t cells = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)xc[1]) << 32) |
                                   (uint32_t)__builtin_amdgcn_readfirstlane((int)xc[0]);
            auto cell_at = [&](int q) { return (int)((cells >> (8 * q)) & 255u); };

            // Segments of the rows that stay inside one cell: todo, X and `mine` are wave-uniform.  At a step of <= 1/8
            // cell per sample a brick row is one segment and the loop takes one trip (the BASELINE lattice, and every
            // octave of turb(7) on the 1/128 lattice but the last two).
            uint32_t todo = 0xffu; // samples not yet computed
            do {
                const int X = cell_at(__ffs((int)todo) - 1);
                uint32_t mine = 0;
#pragma unroll
                for (int q = 0; q < kBrickEdge; ++q) mine |= (((todo >> q) & 1u) && cell_at(q) == X) ? (1u << q) : 0u;

                auto potential = [&](auto kc) __attribute__((always_inline)) {
                    constexpr int k = decltype(kc)::value;
                    // the corner state of the cell (of potential k)
                    int h[8];
                    double K[8], P0[3] = {0.0, 0.0, 0.0}, P1[3] = {0.0, 0.0, 0.0};
                    uint32_t mm[8], tt[8];
                    if (FIELD == kCurl)
                        wn::run_hash_corners(perm, (X + a.off[3 * k]) & 255, (Y + a.off[3 * k + 1]) & 255,
                                             (Z + a.off[3 * k + 2]) & 255, h);
                    else wn::run_hash_corners(perm, X, Y, Z, h);
                    wn::run_corner_entries(h, ye.f, ze.f, K, mm, tt);
                    if (FIELD != kValue) {
                        __builtin_amdgcn_sched_barrier(0); // the corner blend's decoded components after the entries
                        wn::perlin_corner_blend(h, v, w, P0, P1);
                    }
#pragma unroll
                    for (int q = 0; q < kBrickEdge; ++q) {
                        if ((mine >> q) & 1u) {
                            const RunAxisEntryD xe = ax.e[q]; // one address for the wave: a broadcast read
                            double gr[8], gn[3];
                            wn::run_corner_gradients(K, mm, tt, xe.f, gr);
                            // the value's lerps and the partials; what a field does not read falls away at compile time
                            const double nv = wn::perlin_sample_grad(gr, xe.fade, v, w, xe.dfade, dv, dw, P0, P1, gn);
                            if (FIELD == kCurl) {
                                const double one = gn[k == 0 ? 1 : 0], two = gn[k == 2 ? 1 : 2];
                                double &sa = s[(2 * k) % NS][q], &sb = s[(2 * k + 1) % NS][q];
                                sa = (KIND == kNoise) ? one : sa + one;
                                sb = (KIND == kNoise) ? two : sb + two;
                            } else {
                                double &sv = s[0][q];
                                sv = (KIND == kNoise) ? nv : ((KIND == kTurb) ? sv + weight * nv : sv + nv * weight);
                                if (FIELD == kGrad) {
#pragma unroll
                                    for (int c = 0; c < 3; ++c) {
                                        double &sg = s[(1 + c) % NS][q];
                                        sg = (KIND == kNoise) ? gn[c] : sg + gn[c];
                                    }
                                }
                            }
                        }
                        if (FIELD != kValue || (q & 1)) __builtin_amdgcn_sched_barrier(0); // one sample (value: two) at a time
                    }
                };
                potential(std::integral_constant<int, 0>{});
                if (NP == 3) {
                    potential(std::integral_constant<int, 1>{});
                    potential(std::integral_constant<int, 2>{});
                }
                todo &= ~mine;
            } while (todo != 0u);
            amp_sum += weight;
            weight *= 0.5;
        }

        // finish the row: turb's fabs and sign, fractal_noise's division, the curl's subtraction, (float)channel * out_scale
        float fin[CH][kBrickEdge];
#pragma unroll
        for (int q = 0; q < kBrickEdge; ++q) {
            double c[NS];
#pragma unroll
            for (int j = 0; j < NS; ++j) c[j] = (KIND == kFractal) ? s[j][q] / amp_sum : s[j][q];
            if (FIELD == kCurl) {
                double p[6], vel[3];
#pragma unroll
                for (int j = 0; j < 6; ++j) p[j] = c[j % NS];
                wn::perlin_curl_of(p, vel);
#pragma unroll
                for (int ch = 0; ch < CH; ++ch) fin[ch][q] = (float)vel[ch % 3] * g.out_scale;
            } else {
                if (KIND == kTurb) {
                    const bool negative = c[0] < 0.0;
                    c[0] = fabs(c[0]);
#pragma unroll
                    for (int j = 1; j < NS; ++j) c[j] = negative ? -c[j] : c[j];
                }
#pragma unroll
                for (int ch = 0; ch < CH; ++ch) fin[ch][q] = (float)c[ch % NS] * g.out_scale;
            }
            __builtin_amdgcn_sched_barrier(0); // one sample's divisions at a time
        }
        // a lane's row is two float4 of its slot: each channel leaves as one contiguous 2-KiB wave store
        float *const dst = a.out + i * kBrickSamples + lane * kBrickEdge;
#pragma unroll
        for (int ch = 0; ch < CH; ++ch) {
            float *const d = dst + ch * chan;
            if (a.vec4_ok) {
                *reinterpret_cast<v4f *>(d) = v4f{fin[ch][0], fin[ch][1], fin[ch][2], fin[ch][3]};
                *reinterpret_cast<v4f *>(d + 4) = v4f{fin[ch][4], fin[ch][5], fin[ch][6], fin[ch][7]};
            } else {
#pragma unroll
                for (int q = 0; q < kBrickEdge; ++q) d[q] = fin[ch][q];
            }
        }
    }
}

template <int FIELD>
const void *kernel_of(int kind)
{
    return kind == kNoise  ? reinterpret_cast<const void *>(&perlin_bricks_kernel<FIELD, kNoise>)
           : kind == kTurb ? reinterpret_cast<const void *>(&perlin_bricks_kernel<FIELD, kTurb>)
                           : reinterpret_cast<const void *>(&perlin_bricks_kernel<FIELD, kFractal>);
}

// `entry` names the matching dense entry point's checks in check_perm's message (wn_perlin_grid's "perlin grid", ...).
int perlin_bricks(const wn_perm *perm, const wn_grid *grid, int field, int kind, int depth, const int32_t *offsets9_host,
                  const int32_t *bricks_dev, size_t n, float *out_dev, void *stream, const char *entry)
{
    int rc = wn::check_perm(perm, entry);
    if (rc) return rc;
    GridArgs checked;
    if ((rc = wn::check_grid(grid, true, &checked)) != WN_OK) return rc;
    wn::BrickListPlan plan;
    bool launch;
    rc = wn::brick_list_plan(grid, bricks_dev, n, field_channels(field), out_dev, &plan, &launch);
    if (!launch) return rc;

    PerlinBricksArgs a{};
    a.perm = perm->dev;
    a.bricks = bricks_dev;
    a.out = out_dev;
    a.count = n;
    a.g = plan.g;
    a.range = plan.range;
    a.depth = wn::perlin_octaves(kind, depth);
    a.vec4_ok = (reinterpret_cast<uintptr_t>(out_dev) & 15) == 0;
    if (field == kCurl)
        for (int i = 0; i < 9; ++i) a.off[i] = offsets9_host[i] & 255;
    const void *const fn = field == kValue ? kernel_of<kValue>(kind) : (field == kGrad ? kernel_of<kGrad>(kind) : kernel_of<kCurl>(kind));
    void *params[] = {&a};
    const size_t groups = (n + kWaves - 1) / kWaves; // n <= SIZE_MAX / 512: groups * 256 does not overflow
    const hipError_t e = hipLaunchKernel(fn, dim3(wn::stride_blocks(groups * 256, kBrickBlockCap)), dim3(256), params, 0, wn::as_stream(stream));
    if (e != hipSuccess) return wn::hip_fail(e, "perlin_bricks_kernel");
    WN_LAUNCH_CHECK("perlin_bricks_kernel");
    return WN_OK;
}

int check_depth(int depth) { return depth < 0 ? wn::fail(WN_ERR_INVALID, "depth must be >= 0") : WN_OK; }

} // namespace

extern "C" {

int wn_perlin_bricks(const wn_perm *perm, const wn_grid *g, const int32_t *bricks_dev, size_t n, float *out_dev, void *stream)
{
    WN_ENTRY();
    return perlin_bricks(perm, g, kValue, kNoise, 0, nullptr, bricks_dev, n, out_dev, stream, "perlin grid");
}
int wn_perlin_turb_bricks(const wn_perm *perm, const wn_grid *g, int depth, const int32_t *bricks_dev, size_t n, float *out_dev,
                          void *stream)
{
    WN_ENTRY();
    if (const int rc = check_depth(depth)) return rc;
    return perlin_bricks(perm, g, kValue, kTurb, depth, nullptr, bricks_dev, n, out_dev, stream, "perlin grid");
}
int wn_perlin_fractal_bricks(const wn_perm *perm, const wn_grid *g, const int32_t *bricks_dev, size_t n, float *out_dev,
                             void *stream)
{
    WN_ENTRY();
    return perlin_bricks(perm, g, kValue, kFractal, 0, nullptr, bricks_dev, n, out_dev, stream, "perlin grid");
}
int wn_perlin_grad_bricks(const wn_perm *perm, const wn_grid *g, const int32_t *bricks_dev, size_t n, float *out_dev, void *stream)
{
    WN_ENTRY();
    return perlin_bricks(perm, g, kGrad, kNoise, 0, nullptr, bricks_dev, n, out_dev, stream, "perlin gradient grid");
}
int wn_perlin_turb_grad_bricks(const wn_perm *perm, const wn_grid *g, int depth, const int32_t *bricks_dev, size_t n,
                               float *out_dev, void *stream)
{
    WN_ENTRY();
    if (const int rc = check_depth(depth)) return rc;
    return perlin_bricks(perm, g, kGrad, kTurb, depth, nullptr, bricks_dev, n, out_dev, stream, "perlin gradient grid");
}
int wn_perlin_fractal_grad_bricks(const wn_perm *perm, const wn_grid *g, const int32_t *bricks_dev, size_t n, float *out_dev,
                                  void *stream)
{
    WN_ENTRY();
    return perlin_bricks(perm, g, kGrad, kFractal, 0, nullptr, bricks_dev, n, out_dev, stream, "perlin gradient grid");
}
int wn_perlin_curl_bricks(const wn_perm *perm, const wn_grid *g, int kind, int depth, const int32_t *offsets9_host,
                          const int32_t *bricks_dev, size_t n, float *out_dev, void *stream)
{
    WN_ENTRY();
    // kind, depth, table, grid and offsets, stated once for this call and wn_perlin_curl_bounded_bricks; perlin_bricks looks
    // at the table and the grid again
    if (const int rc = wn::perlin_curl_bricks_checks(perm, g, kind, depth, offsets9_host)) return rc;
    return perlin_bricks(perm, g, kCurl, kind, depth, offsets9_host, bricks_dev, n, out_dev, stream, "perlin curl grid");
}

} // extern "C"
