// wn_perlin_curl.hip -- divergence-free curl noise from three Perlin potentials (noise, the signed turb sum,
// fractal_noise) for gfx950: point lists and dense grids of {vx, vy, vz} (include/wnoise_perlin_curl.h; absent from the
// reference).
//
// The evaluators are wn_eval.hpp's perlin_curl_exact / perlin_turb_curl / perlin_fractal_curl: per point and octave the
// lattice decode, fractional parts, fade and fade' once, the hashes per potential, six partials in perlin_sample_grad's
// expressions, one subtraction per component.  fp64, contraction off: host and device return the same bits.
#include "wn_perlin_frame.hpp"
#include "wnoise_perlin_curl.h"

#include <cmath>
#include <type_traits>

namespace {

using wn::GridArgs, wn::kNoise, wn::kTurb, wn::kFractal;
using wn::kRunMaxDepth, wn::kRunTY, wn::kRunTZ, wn::RunAxisEntryD, wn::RunKEntry;
static_assert(WN_PERLIN_CURL_NOISE == kNoise && WN_PERLIN_CURL_TURB == kTurb && WN_PERLIN_CURL_FRACTAL == kFractal,
              "the public kinds are the kernels' kinds");

struct CurlOffsets {
    int o[9]; // (x, y, z) of psi0, psi1, psi2, each in 0..255
};

struct PerlinCurlGridArgs : wn::PerlinGridFrame { // out: three consecutive volumes: vx, vy, vz
    CurlOffsets off;
};

__device__ __forceinline__ void curl_vec3(const uint8_t *perm, int kind, int depth, const int *off, float px, float py, float pz,
                                          double v[3])
{
    if (kind == kNoise) wn::perlin_curl_exact(perm, (double)px, (double)py, (double)pz, off, v);
    else if (kind == kTurb) wn::perlin_turb_curl(perm, px, py, pz, depth, off, v);
    else wn::perlin_fractal_curl(perm, px, py, pz, off, v);
}

// Generic dense-grid kernel: one sample per lane, every sample hashes for itself.  Serves what the run kernel below does
// not (narrow grids, depth 0 or > kRunMaxDepth).
__global__ __launch_bounds__(256) void perlin_curl_grid_generic_kernel(const PerlinCurlGridArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_perm[512];
    wn::load_perm_lds(s_perm, a.perm);
    const uint8_t *perm = s_perm;
    const GridArgs &g = a.g;
    wn::perlin_for_each_sample(g, [&](size_t e, size_t total, float px, float py, float pz) {
        double v[3];
        curl_vec3(perm, a.kind, a.depth, a.off.o, px, py, pz, v);
        a.out[e] = (float)v[0] * g.out_scale;
        a.out[total + e] = (float)v[1] * g.out_scale;
        a.out[2 * total + e] = (float)v[2] * g.out_scale;
    });
}

// ------------------------------------------------------------------------------------------------------------------------
// perlin_curl_grid_run_kernel -- the run form of wn_perlin_frame.hpp carrying three potentials.
// Built once per block and shared by the potentials: the x / y / z axis tables {f, fade, fade'} and the cell-index tables.
// Built once per wave, row and octave and shared: the {K, mm, t} table (wn::run_k_entry depends on h & 15, dy, dz only).
// Per potential and cell: the eight corner hashes at ((X + ox_k) & 255, (Y + oy_k) & 255, (Z + oz_k) & 255), their K / mm /
// t fetches and P0 / P1 of wn::perlin_corner_blend; per potential and sample: wn::perlin_sample_grad, of which the two
// partials the curl reads are kept (the value, the third partial and what only they need fall away at compile time).
// Registers: six running sums per sample.  A run of 8 samples would hold 96 VGPRs of sums where the gradient kernel holds
// 64 and already sits near its budget of 256, so a run is 4 samples (48 VGPRs of sums, 24 of the run's x entries), a block
// is 256 x 8 x 8 samples and runs 8 waves with a 256-VGPR budget.  Everything indexed by sample or potential is indexed at
// compile time: the potentials and the 4 samples are unrolled inside a rolled loop over the cells a run crosses.
// fractal_noise's division and the subtraction happen when the row is finished.
// Stores: a lane's run of 4 samples IS one aligned float4 of the row, so each component's row leaves as one contiguous
// 1-KiB wave store straight from registers -- the per-wave stage of the 8-sample gradient kernel would be the identity
// here -- with scalar stores when rows are not 16-byte aligned and at the row tail.
// ------------------------------------------------------------------------------------------------------------------------
constexpr int kRun = 4;           // samples per lane and row
constexpr int kRunX = 64 * kRun;  // x samples per workgroup
constexpr int kRunWaves = 8;

__host__ __device__ constexpr size_t curl_run_lds_bytes(int depth)
{
    return kRunWaves * 64 * sizeof(RunKEntry) + (size_t)depth * kRunX * sizeof(RunAxisEntryD) +
           (size_t)depth * (kRunTY + kRunTZ) * (sizeof(RunAxisEntryD) + sizeof(int)) + (size_t)depth * kRunX /* x cells */ +
           512 /* perm */;
}

template <int KIND>
__global__ __launch_bounds__(64 * kRunWaves) void perlin_curl_grid_run_kernel(const PerlinCurlGridArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char run_lds[];
    const GridArgs &g = a.g;
    const int depth = wn::run_depth<KIND>(a);
    // LDS carve-up (16-byte aligned members first)
    RunKEntry *const ktab_all = reinterpret_cast<RunKEntry *>(run_lds);                       // [waves][64]
    double *const xtab = reinterpret_cast<double *>(ktab_all + kRunWaves * 64);               // [depth][3 (f, fade, fade')][kRunX]
    RunAxisEntryD *const ytab = reinterpret_cast<RunAxisEntryD *>(xtab + (size_t)depth * 3 * kRunX); // [depth][kRunTY]
    RunAxisEntryD *const ztab = ytab + (size_t)depth * kRunTY;                                // [depth][kRunTZ]
    int *const ycell = reinterpret_cast<int *>(ztab + (size_t)depth * kRunTZ);                // [depth][kRunTY]
    int *const zcell = ycell + depth * kRunTY;                                                // [depth][kRunTZ]
    uint8_t *const xcell = reinterpret_cast<uint8_t *>(zcell + depth * kRunTZ);               // [depth][kRunX]
    uint8_t *const perm = xcell + (size_t)depth * kRunX;                                      // [512]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x_first = blockIdx.x * kRunX, y_first = blockIdx.y * kRunTY, z_first = blockIdx.z * kRunTZ;
    const float den = (float)g.den;

    // ---- per-axis tables of the block, with fade' ---------------------------------------------------------------------
    wn::run_load_perm(perm, a.perm, tid, 64 * kRunWaves);
    // x entries are stored [octave][member][q][lane] (sample x = lane * kRun + q): the 64 lanes of a wave read adjacent doubles
    for (int xi = tid; xi < kRunX; xi += 64 * kRunWaves) {
        const int slot = (xi & (kRun - 1)) * 64 + (xi / kRun);
        wn::run_octave_walk<KIND>(wn::run_coord(g, den, x_first + xi, g.nx), depth, [&](int i, int cell, double f) {
            double *const e = xtab + (size_t)i * 3 * kRunX + slot;
            e[0] = f;
            e[kRunX] = wn::pfade(f);
            e[2 * kRunX] = wn::pfade_d(f);
            xcell[(size_t)i * kRunX + xi] = (uint8_t)cell;
        });
    }
    wn::run_tabulate_yz<KIND>(g, den, depth, y_first, z_first, tid, ytab, ztab, ycell, zcell);
    __syncthreads();

    RunKEntry *const ktab = ktab_all + wave * 64;
    const int rows_y = min(kRunTY, g.ny - y_first), rows_z = min(kRunTZ, g.nz - z_first);
    const size_t total = (size_t)g.nx * g.ny * g.nz;
    for (int r = wave; r < rows_y * rows_z; r += kRunWaves) {
        const int yi = r % rows_y, zi = r / rows_y;
        double amp_sum = 0.0, weight = 1.0; // fractal_noise: max_value and the amplitude
        // the six partials of the run's samples, s[2k], s[2k+1] of potential k:
        // {d psi0/dy, d psi0/dz, d psi1/dx, d psi1/dz, d psi2/dx, d psi2/dy}
        double s[6][kRun];
#pragma unroll
        for (int j = 0; j < 6; ++j)
#pragma unroll
            for (int q = 0; q < kRun; ++q) s[j][q] = 0.0;

#pragma nounroll
        for (int oc = 0; oc < depth; ++oc) {
            const RunAxisEntryD ye = ytab[oc * kRunTY + yi], ze = ztab[oc * kRunTZ + zi];
            const int Y = ycell[oc * kRunTY + yi], Z = zcell[oc * kRunTZ + zi];
            wn::run_publish_ktab(ktab, lane, ye.f, ze.f); // the same table for every potential
            const double v = ye.fade, w = ze.fade, dv = ye.dfade, dw = ze.dfade;
            // the run's x entries, shared by the potentials
            const double *const xe = xtab + (size_t)oc * 3 * kRunX + lane;
            double xf[kRun], xu[kRun], xdu[kRun];
#pragma unroll
            for (int q = 0; q < kRun; ++q) {
                xf[q] = xe[q * 64];
                xu[q] = xe[kRunX + q * 64];
                xdu[q] = xe[2 * kRunX + q * 64];
            }
            const uint32_t cells = *reinterpret_cast<const uint32_t *>(xcell + (size_t)oc * kRunX + lane * kRun);
            auto cell_at = [&](int qq) { return (int)((cells >> (8 * qq)) & 255u); };

            // Segments of the runs that stay inside one cell (rolled, as in the gradient kernel); inside a segment the
            // potentials and the samples are unrolled.  A sample is skipped where no lane of the wave has it in the
            // hashed cell.
            uint32_t todo = (1u << kRun) - 1u; // this lane's samples not yet computed
            do {
                const int X = cell_at(todo ? __ffs((int)todo) - 1 : 0);
                bool in[kRun];
                uint32_t mine = 0;
#pragma unroll
                for (int q = 0; q < kRun; ++q) {
                    in[q] = ((todo >> q) & 1u) && cell_at(q) == X;
                    mine |= in[q] ? (1u << q) : 0u;
                }
                auto potential = [&](auto kc) __attribute__((always_inline)) {
                    constexpr int k = decltype(kc)::value;
                    // the corner state of the cell of potential k
                    double K[8], P0[3], P1[3];
                    uint32_t mm[8], tt[8];
                    {
                        int h[8];
                        wn::run_hash_cell(perm, (X + a.off.o[3 * k]) & 255, (Y + a.off.o[3 * k + 1]) & 255,
                                          (Z + a.off.o[3 * k + 2]) & 255, ktab, h, K, mm, tt);
                        __builtin_amdgcn_sched_barrier(0); // the corner blend's decoded components after the table fetch
                        wn::perlin_corner_blend(h, v, w, P0, P1);
                    }
#pragma unroll
                    for (int q = 0; q < kRun; ++q) {
                        if (__any(in[q])) {
                            double gr[8], gn[3];
                            wn::run_corner_gradients(K, mm, tt, xf[q], gr);
                            wn::perlin_sample_grad(gr, xu[q], v, w, xdu[q], dv, dw, P0, P1, gn);
                            const double first = gn[k == 0 ? 1 : 0], second = gn[k == 2 ? 1 : 2];
                            double &sa = s[2 * k][q], &sb = s[2 * k + 1][q];
                            if (KIND == kNoise) {
                                sa = in[q] ? first : sa;
                                sb = in[q] ? second : sb;
                            } else {
                                sa = in[q] ? sa + first : sa;
                                sb = in[q] ? sb + second : sb;
                            }
                        }
                        __builtin_amdgcn_sched_barrier(0); // one sample at a time
                    }
                };
                potential(std::integral_constant<int, 0>{});
                potential(std::integral_constant<int, 1>{});
                potential(std::integral_constant<int, 2>{});
                todo &= ~mine;
            } while (__any(todo != 0u));
            amp_sum += weight;
            weight *= 0.5;
        }

        // finish the row: fractal_noise's division, the subtraction, then (float)component * out_scale
        float fin[3][kRun];
#pragma unroll
        for (int q = 0; q < kRun; ++q) {
            double p[6], vel[3];
#pragma unroll
            for (int j = 0; j < 6; ++j) p[j] = (KIND == kFractal) ? s[j][q] / amp_sum : s[j][q];
            wn::perlin_curl_of(p, vel);
#pragma unroll
            for (int c = 0; c < 3; ++c) fin[c][q] = (float)vel[c] * g.out_scale;
            __builtin_amdgcn_sched_barrier(0); // one sample's six divisions at a time
        }
        // a lane's run is one float4 of the row: each component's row leaves as one contiguous wave store
        static_assert(kRun == 4, "a run is one float4");
        const int xo = lane * kRun;
        float *const row = a.out + ((size_t)(z_first + zi) * g.ny + (y_first + yi)) * g.nx + x_first + xo;
#pragma unroll
        for (int c = 0; c < 3; ++c)
            wn::run_store4(row + (size_t)c * total, 0, a.vec4_ok, x_first + xo, g.nx, v4f{fin[c][0], fin[c][1], fin[c][2], fin[c][3]});
    }
}

struct PerlinCurlPointsArgs {
    const uint8_t *perm;
    const double *pts64;
    const float *pts32;
    double *out; // n records {vx, vy, vz}
    size_t count;
    CurlOffsets off;
    int kind, depth;
};

__global__ __launch_bounds__(256) void perlin_curl_points_kernel(const PerlinCurlPointsArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_perm[512];
    wn::load_perm_lds(s_perm, a.perm);
    const uint8_t *perm = s_perm;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.count; i += (size_t)gridDim.x * blockDim.x) {
        double v[3];
        if (a.pts64) {
            const double *p = a.pts64 + 3 * i;
            wn::perlin_curl_exact(perm, p[0], p[1], p[2], a.off.o, v);
        } else {
            const float *p = a.pts32 + 3 * i;
            curl_vec3(perm, a.kind, a.depth, a.off.o, p[0], p[1], p[2], v);
        }
        double *const rec = a.out + 3 * i;
        rec[0] = v[0];
        rec[1] = v[1];
        rec[2] = v[2];
    }
}

int check_kind(int kind, int depth)
{
    if (kind < kNoise || kind > kFractal) return wn::fail(WN_ERR_INVALID, "kind must be 0 (noise), 1 (turb) or 2 (fractal_noise)");
    if (kind == kTurb && depth < 0) return wn::fail(WN_ERR_INVALID, "depth must be >= 0");
    return WN_OK;
}

CurlOffsets reduce_offsets(const int32_t *offsets9_host)
{
    CurlOffsets off;
    for (int i = 0; i < 9; ++i) off.o[i] = offsets9_host[i] & 255;
    return off;
}

int perlin_curl_grid(const wn_perm *perm, const wn_grid *grid, int kind, int depth, const int32_t *offsets9_host,
                     float *out_dev, void *stream)
{
    int rc = check_kind(kind, depth);
    if (rc) return rc;
    PerlinCurlGridArgs a;
    if (!wn::perlin_grid_frame(perm, grid, kind, depth, out_dev, "perlin curl grid", &a, &rc)) return rc;
    if (!offsets9_host) return wn::fail(WN_ERR_INVALID, "offsets9_host is NULL");
    a.off = reduce_offsets(offsets9_host);
    const void *fn = kind == kNoise  ? reinterpret_cast<const void *>(&perlin_curl_grid_run_kernel<kNoise>)
                     : kind == kTurb ? reinterpret_cast<const void *>(&perlin_curl_grid_run_kernel<kTurb>)
                                     : reinterpret_cast<const void *>(&perlin_curl_grid_run_kernel<kFractal>);
    return wn::perlin_grid_launch(a, kRunX, fn, curl_run_lds_bytes(a.depth), curl_run_lds_bytes(kRunMaxDepth), 64 * kRunWaves,
                                  "perlin_curl_grid_run_kernel", reinterpret_cast<const void *>(&perlin_curl_grid_generic_kernel),
                                  "perlin_curl_grid_generic_kernel", stream);
}

int perlin_curl_points(const wn_perm *perm, const double *p64, const float *p32, size_t n, int kind, int depth,
                       const int32_t *offsets9_host, double *out3_dev, void *stream)
{
    int rc = check_kind(kind, depth);
    if (rc) return rc;
    rc = wn::check_perm(perm, "perlin curl points");
    if (rc || n == 0) return rc;
    if ((!p64 && !p32) || !out3_dev) return wn::fail(WN_ERR_INVALID, "points/out pointer is NULL");
    if (!offsets9_host) return wn::fail(WN_ERR_INVALID, "offsets9_host is NULL");
    PerlinCurlPointsArgs a{perm->dev, p64, p32, out3_dev, n, reduce_offsets(offsets9_host), kind, depth};
    hipLaunchKernelGGL(perlin_curl_points_kernel, dim3(wn::stride_blocks(n)), dim3(256), 0, wn::as_stream(stream), a);
    WN_LAUNCH_CHECK("perlin_curl_points_kernel");
    return WN_OK;
}

} // namespace

extern "C" {

int wn_perlin_curl_points(const wn_perm *perm, const double *xyz_dev, size_t n, const int32_t *offsets9_host, double *out3_dev,
                          void *stream)
{
    WN_ENTRY();
    return perlin_curl_points(perm, xyz_dev, nullptr, n, kNoise, 0, offsets9_host, out3_dev, stream);
}
int wn_perlin_curl_points_vec3(const wn_perm *perm, const float *xyz_dev, size_t n, int kind, int depth,
                               const int32_t *offsets9_host, double *out3_dev, void *stream)
{
    WN_ENTRY();
    return perlin_curl_points(perm, nullptr, xyz_dev, n, kind, depth, offsets9_host, out3_dev, stream);
}
int wn_perlin_curl_grid(const wn_perm *perm, const wn_grid *g, int kind, int depth, const int32_t *offsets9_host, float *out_dev,
                        void *stream)
{
    WN_ENTRY();
    return perlin_curl_grid(perm, g, kind, depth, offsets9_host, out_dev, stream);
}

} // extern "C"
