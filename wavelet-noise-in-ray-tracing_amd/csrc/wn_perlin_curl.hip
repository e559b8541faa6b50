// wn_perlin_curl.hip -- divergence-free curl noise from three Perlin potentials (noise, the signed turb sum,
// fractal_noise) for gfx950: point lists and dense grids of {vx, vy, vz} (include/wnoise_perlin_curl.h; absent from the
// reference).
//
// The evaluators are wn_eval.hpp's perlin_curl_exact / perlin_turb_curl / perlin_fractal_curl: per point and octave the
// lattice decode, fractional parts, fade and fade' once, the hashes per potential, six partials in perlin_sample_grad's
// expressions, one subtraction per component.  fp64, contraction off: host and device return the same bits.
#include "wn_internal.hpp"
#include "wn_device_eval.hpp"
#include "wn_perlin_run.hpp"
#include "wnoise_perlin_curl.h"

#include <cmath>
#include <type_traits>

namespace {

using wn::GridArgs;

enum { kNoise = WN_PERLIN_CURL_NOISE, kTurb = WN_PERLIN_CURL_TURB, kFractal = WN_PERLIN_CURL_FRACTAL };

struct CurlOffsets {
    int o[9]; // (x, y, z) of psi0, psi1, psi2, each in 0..255
};

struct PerlinCurlGridArgs {
    const uint8_t *perm;
    float *out; // three consecutive volumes: vx, vy, vz
    GridArgs g;
    CurlOffsets off;
    int kind, depth;
    int vec4_ok; // rows of every channel start 16-byte aligned
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
    const float den = (float)g.den;
    const unsigned plane = (unsigned)g.nx * (unsigned)g.ny;
    const size_t total = (size_t)plane * g.nz;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const unsigned z = (unsigned)(e / plane);
        const unsigned r = (unsigned)(e - (size_t)z * plane);
        const unsigned y = r / (unsigned)g.nx, x = r - y * (unsigned)g.nx;
        const float px = wn::lattice_coord((int)x, den, g.base_range, g.octave_scale, g.post_scale);
        const float py = wn::lattice_coord((int)y, den, g.base_range, g.octave_scale, g.post_scale);
        const float pz = g.z_const_mode ? g.z_const
                                        : wn::lattice_coord(g.z0 + (int)z, den, g.base_range, g.octave_scale, g.post_scale);
        double v[3];
        curl_vec3(perm, a.kind, a.depth, a.off.o, px, py, pz, v);
        a.out[e] = (float)v[0] * g.out_scale;
        a.out[total + e] = (float)v[1] * g.out_scale;
        a.out[2 * total + e] = (float)v[2] * g.out_scale;
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// perlin_curl_grid_run_kernel -- the cell-sharing organisation of perlin_grad_grid_run_kernel (wn_perlin_grad.hip: per-axis
// tables of the block in LDS, a lane walks a run of consecutive x samples, corner state once per cell the run enters),
// carrying three potentials.
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
constexpr int kRunMaxDepth = 8;
constexpr int kRun = 4;           // samples per lane and row
constexpr int kRunX = 64 * kRun;  // x samples per workgroup
constexpr int kRunTY = 8;         // rows ...
constexpr int kRunTZ = 8;         // ... and planes per workgroup
constexpr int kRunWaves = 8;

struct RunAxisEntryD {
    double f, fade, dfade; // fractional part, fade() and fade'()
};
using wn::RunKEntry;

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
    const int depth = (KIND == kNoise) ? 1 : a.depth; // fractal_noise: the host passes its 6 octaves
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

    // ---- per-axis tables of the block (wn_perlin_grad.hip's) -------------------------------------------------------
    for (int i = tid; i < 128; i += 64 * kRunWaves)
        reinterpret_cast<uint32_t *>(perm)[i] = reinterpret_cast<const uint32_t *>(a.perm)[i];
    auto tabulate = [&](float p, auto store) {
        float cur = p;          // turb: the float point doubles per octave
        double frequency = 1.0; // fractal_noise: float point times a double frequency
        for (int i = 0; i < depth; ++i) {
            const double c = (KIND == kFractal) ? (double)p * frequency : (double)cur;
            const double fl = floor(c);
            store(i, (int)fl & 255, c - fl);
            cur *= 2.0f;
            frequency *= 2.0;
        }
    };
    // x entries are stored [octave][member][q][lane] (sample x = lane * kRun + q): the 64 lanes of a wave read adjacent doubles
    for (int xi = tid; xi < kRunX; xi += 64 * kRunWaves) {
        const int x = min(x_first + xi, g.nx - 1);
        const int slot = (xi & (kRun - 1)) * 64 + (xi / kRun);
        tabulate(wn::lattice_coord(x, den, g.base_range, g.octave_scale, g.post_scale), [&](int i, int cell, double f) {
            double *const e = xtab + (size_t)i * 3 * kRunX + slot;
            e[0] = f;
            e[kRunX] = wn::pfade(f);
            e[2 * kRunX] = wn::pfade_d(f);
            xcell[(size_t)i * kRunX + xi] = (uint8_t)cell;
        });
    }
    if (tid >= 256 && tid < 256 + kRunTY) {
        const int yi = tid - 256;
        const int y = min(y_first + yi, g.ny - 1);
        tabulate(wn::lattice_coord(y, den, g.base_range, g.octave_scale, g.post_scale), [&](int i, int cell, double f) {
            ytab[i * kRunTY + yi] = RunAxisEntryD{f, wn::pfade(f), wn::pfade_d(f)};
            ycell[i * kRunTY + yi] = cell;
        });
    } else if (tid >= 320 && tid < 320 + kRunTZ) {
        const int zi = tid - 320;
        const int z = g.z0 + min(z_first + zi, g.nz - 1);
        const float pz = g.z_const_mode ? g.z_const : wn::lattice_coord(z, den, g.base_range, g.octave_scale, g.post_scale);
        tabulate(pz, [&](int i, int cell, double f) {
            ztab[i * kRunTZ + zi] = RunAxisEntryD{f, wn::pfade(f), wn::pfade_d(f)};
            zcell[i * kRunTZ + zi] = cell;
        });
    }
    __syncthreads();

    RunKEntry *const ktab = ktab_all + wave * 64;
    const int rows_y = min(kRunTY, g.ny - y_first), rows_z = min(kRunTZ, g.nz - z_first);
    const size_t total = (size_t)g.nx * g.ny * g.nz;
    // this lane's entry of the per-row table: hash h, corner (cy, cz)
    const int kh = lane & 15, kcy = (lane >> 4) & 1, kcz = lane >> 5;
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
            { // per-row table: entry (cy, cz, h) -> {K, mm, t} (grad(), perlin.h:26-31), the same for every potential
                const double dy = kcy ? ye.f - 1.0 : ye.f, dz = kcz ? ze.f - 1.0 : ze.f;
                const RunKEntry mine = wn::run_k_entry(kh, dy, dz);
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); // the previous octave's reads are done
                ktab[lane] = mine;
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            }
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
                        const int Xk = (X + a.off.o[3 * k]) & 255, Yk = (Y + a.off.o[3 * k + 1]) & 255,
                                  Zk = (Z + a.off.o[3 * k + 2]) & 255;
                        const int A = perm[Xk] + Yk, AA = perm[A] + Zk, AB = perm[A + 1] + Zk;
                        const int B = perm[Xk + 1] + Yk, BA = perm[B] + Zk, BB = perm[B + 1] + Zk;
                        const int h[8] = {perm[AA], perm[BA], perm[AB], perm[BB], perm[AA + 1], perm[BA + 1], perm[AB + 1], perm[BB + 1]};
#pragma unroll
                        for (int c = 0; c < 8; ++c) {
                            const RunKEntry e = ktab[(c >> 1) * 16 + (h[c] & 15)];
                            K[c] = e.K;
                            mm[c] = e.mm;
                            tt[c] = e.t;
                        }
                        __builtin_amdgcn_sched_barrier(0); // the corner blend's decoded components after the table fetch
                        wn::perlin_corner_blend(h, v, w, P0, P1);
                    }
#pragma unroll
                    for (int q = 0; q < kRun; ++q) {
                        if (__any(in[q])) {
                            const double xm1 = xf[q] - 1.0;
                            const uint64_t b0 = (uint64_t)__double_as_longlong(xf[q]), b1 = (uint64_t)__double_as_longlong(xm1);
                            double gr[8], gn[3];
#pragma unroll
                            for (int c = 0; c < 8; ++c) gr[c] = wn::run_gradient(K[c], mm[c], tt[c], (c & 1) ? b1 : b0);
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
        for (int c = 0; c < 3; ++c) {
            float *const dst = row + (size_t)c * total;
            if (a.vec4_ok && x_first + xo + 4 <= g.nx) *reinterpret_cast<v4f *>(dst) = v4f{fin[c][0], fin[c][1], fin[c][2], fin[c][3]};
            else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (x_first + xo + e < g.nx) dst[e] = fin[c][e];
            }
        }
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

constexpr size_t kBlockCap = 256u * 8u * 8u; // workgroups of a grid-stride launch (wn::stride_blocks)

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
    rc = wn::check_perm(perm, "perlin curl grid");
    if (rc) return rc;
    GridArgs g;
    rc = wn::check_grid(grid, true, &g);
    if (rc) return rc;
    const size_t total = (size_t)g.nx * g.ny * g.nz;
    if (total == 0) return WN_OK;
    if (!out_dev) return wn::fail(WN_ERR_INVALID, "out_dev is NULL");
    if (!offsets9_host) return wn::fail(WN_ERR_INVALID, "offsets9_host is NULL");
    if ((size_t)g.nx * g.ny > 0xffffffffull) return wn::fail(WN_ERR_INVALID, "plane too large");
    PerlinCurlGridArgs a{perm->dev, out_dev, g, reduce_offsets(offsets9_host), kind, depth, 0};
    a.vec4_ok = wn::vec4_ok(out_dev, g.nx); // nx % 4 == 0: every channel volume starts 16-byte aligned too
    const int octaves = kind == kNoise ? 1 : (kind == kFractal ? 6 : depth);
    if (kind == kFractal) a.depth = octaves;
    const dim3 rgrid((g.nx + kRunX - 1) / kRunX, (g.ny + kRunTY - 1) / kRunTY, (g.nz + kRunTZ - 1) / kRunTZ);
    // the run kernel: rows of >= 128 samples, 1..8 octaves (the gradient's rule)
    if (g.nx >= 128 && octaves >= 1 && octaves <= kRunMaxDepth && rgrid.y <= 65535u && rgrid.z <= 65535u) {
        const size_t lds = curl_run_lds_bytes(octaves);
        const void *fn = kind == kNoise  ? reinterpret_cast<const void *>(&perlin_curl_grid_run_kernel<kNoise>)
                         : kind == kTurb ? reinterpret_cast<const void *>(&perlin_curl_grid_run_kernel<kTurb>)
                                         : reinterpret_cast<const void *>(&perlin_curl_grid_run_kernel<kFractal>);
        if (lds <= 48 * 1024 || wn::ensure_dynamic_lds(fn, wn::current_device(), curl_run_lds_bytes(kRunMaxDepth))) {
            void *params[] = {&a};
            const hipError_t e = hipLaunchKernel(fn, rgrid, dim3(64 * kRunWaves), params, lds, wn::as_stream(stream));
            if (e != hipSuccess) return wn::hip_fail(e, "perlin_curl_grid_run_kernel");
            WN_LAUNCH_CHECK("perlin_curl_grid_run_kernel");
            return WN_OK;
        }
    }
    hipLaunchKernelGGL(perlin_curl_grid_generic_kernel, dim3(wn::stride_blocks(total, kBlockCap)), dim3(256), 0,
                       wn::as_stream(stream), a);
    WN_LAUNCH_CHECK("perlin_curl_grid_generic_kernel");
    return WN_OK;
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
    hipLaunchKernelGGL(perlin_curl_points_kernel, dim3(wn::stride_blocks(n, kBlockCap)), dim3(256), 0, wn::as_stream(stream), a);
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
