// wn_perlin_grad.hip -- analytic gradients of perlin::noise, RTOW turb and perlin::fractal_noise for gfx950: point lists
// and dense grids of {value, d/dx, d/dy, d/dz} (include/wnoise.h; absent from the reference).
//
// The evaluators are wn_eval.hpp's perlin_grad_exact / perlin_turb_grad / perlin_fractal_grad: the value channel is
// perlin_exact's arithmetic (the bits of the value kernels of wn_perlin.hip, which this file leaves alone), the gradient
// blends the corner vectors over z, then y, and over x last.  fp64, contraction off: host and device return the same bits.
#include "wn_perlin_frame.hpp"

#include <cmath>

namespace {

using wn::GridArgs, wn::kNoise, wn::kTurb, wn::kFractal;
using wn::kRunMaxDepth, wn::kRunTY, wn::kRunTZ, wn::RunAxisEntry, wn::RunAxisEntryD, wn::RunKEntry;

struct PerlinGradGridArgs : wn::PerlinGridFrame {}; // out: four consecutive volumes: value, d/dx, d/dy, d/dz

__device__ __forceinline__ double grad_vec3(const uint8_t *perm, int kind, int depth, float px, float py, float pz, double g[3])
{
    if (kind == kNoise) return wn::perlin_grad_exact(perm, (double)px, (double)py, (double)pz, g);
    if (kind == kTurb) return wn::perlin_turb_grad(perm, px, py, pz, depth, g);
    return wn::perlin_fractal_grad(perm, px, py, pz, g);
}

// Generic dense-grid kernel: one sample per lane, every sample hashes for itself.  Serves what the run kernel below does
// not (narrow grids, depth 0 or > kRunMaxDepth).
__global__ __launch_bounds__(256) void perlin_grad_grid_generic_kernel(const PerlinGradGridArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_perm[512];
    wn::load_perm_lds(s_perm, a.perm);
    const uint8_t *perm = s_perm;
    const GridArgs &g = a.g;
    wn::perlin_for_each_sample(g, [&](size_t e, size_t total, float px, float py, float pz) {
        double gr[3];
        const double v = grad_vec3(perm, a.kind, a.depth, px, py, pz, gr);
        a.out[e] = (float)v * g.out_scale;
        a.out[total + e] = (float)gr[0] * g.out_scale;
        a.out[2 * total + e] = (float)gr[1] * g.out_scale;
        a.out[3 * total + e] = (float)gr[2] * g.out_scale;
    });
}

// ------------------------------------------------------------------------------------------------------------------------
// perlin_grad_grid_run_kernel -- the run form of wn_perlin_frame.hpp carrying the gradient:
//   * the axis tables gain fade'(f) per entry;
//   * per cell and row the lane decodes the eight corner vectors from the hashes it already has and blends them over z,
//     then y: the six constants P0_k, P1_k (wn::perlin_corner_blend);
//   * per sample, wn::perlin_sample_grad adds the three final lerps over x and the three difference terms to the value's
//     own 7 lerps, whose intermediates it reuses: ~34 fp64 operations on top of the value's ~29.
// Running sums: the value kernel parks its sums in LDS (4 KB per wave).  Four channels of them at 16 waves would need
// 256 KB beside the axis tables (86 KB at 7 octaves with fade'), so this kernel keeps the sums of a lane's 8 samples x 4
// channels in registers (64 VGPRs) and runs 8 waves per workgroup with a 256-VGPR budget.  Everything indexed by the
// sample number is therefore indexed at compile time: the 8 samples are unrolled inside a rolled loop over the cells a
// run crosses.  turb's sign is known after the last octave and is applied when the row is finished.
// A finished row leaves channel by channel through a 2-KB stage per wave (fp32, x order): four contiguous 2-KiB wave
// stores, one per channel volume.
// ------------------------------------------------------------------------------------------------------------------------
constexpr int kRunX = 512; // x samples per workgroup (64 lanes x 8)
constexpr int kRun = 8;    // samples per lane and row
constexpr int kRunWaves = 8;

__host__ __device__ constexpr size_t grad_run_lds_bytes(int depth)
{
    return kRunWaves * 64 * sizeof(RunKEntry) + (size_t)depth * kRunX * (sizeof(RunAxisEntry) + sizeof(double)) +
           kRunWaves * kRunX * sizeof(float) /* stage */ + (size_t)depth * (kRunTY + kRunTZ) * (sizeof(RunAxisEntryD) + sizeof(int)) +
           (size_t)depth * kRunX /* x cells */ + 512 /* perm */;
}

template <int KIND>
__global__ __launch_bounds__(64 * kRunWaves) void perlin_grad_grid_run_kernel(const PerlinGradGridArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char run_lds[];
    const GridArgs &g = a.g;
    const int depth = wn::run_depth<KIND>(a);
    // LDS carve-up (16-byte aligned members first)
    RunKEntry *const ktab_all = reinterpret_cast<RunKEntry *>(run_lds);                    // [waves][64]
    RunAxisEntry *const xtab = reinterpret_cast<RunAxisEntry *>(ktab_all + kRunWaves * 64); // [depth][512]
    double *const xdf = reinterpret_cast<double *>(xtab + (size_t)depth * kRunX);           // [depth][512] fade'
    float *const stage_all = reinterpret_cast<float *>(xdf + (size_t)depth * kRunX);        // [waves][512]
    RunAxisEntryD *const ytab = reinterpret_cast<RunAxisEntryD *>(stage_all + kRunWaves * kRunX); // [depth][kRunTY]
    RunAxisEntryD *const ztab = ytab + (size_t)depth * kRunTY;                              // [depth][kRunTZ]
    int *const ycell = reinterpret_cast<int *>(ztab + (size_t)depth * kRunTZ);              // [depth][kRunTY]
    int *const zcell = ycell + depth * kRunTY;                                              // [depth][kRunTZ]
    uint8_t *const xcell = reinterpret_cast<uint8_t *>(zcell + depth * kRunTZ);             // [depth][512]
    uint8_t *const perm = xcell + (size_t)depth * kRunX;                                    // [512]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x_first = blockIdx.x * kRunX, y_first = blockIdx.y * kRunTY, z_first = blockIdx.z * kRunTZ;
    const float den = (float)g.den;

    // ---- per-axis tables of the block, with fade' ---------------------------------------------------------------------
    wn::run_load_perm(perm, a.perm, tid, 64 * kRunWaves);
    // x entries are stored [octave][q][lane] (sample x = lane*8 + q): the 64 lanes of a wave read adjacent entries
    for (int xi = tid; xi < kRunX; xi += 64 * kRunWaves) {
        const int slot = (xi & (kRun - 1)) * 64 + (xi >> 3);
        wn::run_octave_walk<KIND>(wn::run_coord(g, den, x_first + xi, g.nx), depth, [&](int i, int cell, double f) {
            xtab[(size_t)i * kRunX + slot] = RunAxisEntry::of(f);
            xdf[(size_t)i * kRunX + slot] = wn::pfade_d(f);
            xcell[(size_t)i * kRunX + xi] = (uint8_t)cell;
        });
    }
    wn::run_tabulate_yz<KIND>(g, den, depth, y_first, z_first, tid, ytab, ztab, ycell, zcell);
    __syncthreads();

    RunKEntry *const ktab = ktab_all + wave * 64;
    float *const stage = stage_all + wave * kRunX;
    const int rows_y = min(kRunTY, g.ny - y_first), rows_z = min(kRunTZ, g.nz - z_first);
    const size_t total = (size_t)g.nx * g.ny * g.nz;
    for (int r = wave; r < rows_y * rows_z; r += kRunWaves) {
        const int yi = r % rows_y, zi = r / rows_y;
        double amp_sum = 0.0, weight = 1.0; // fractal max_value / turb weight, fractal amplitude
        // the four channels of the run's 8 samples: running sums, then the finished channels
        double sv[kRun], sx[kRun], sy[kRun], sz[kRun];
#pragma unroll
        for (int q = 0; q < kRun; ++q) sv[q] = sx[q] = sy[q] = sz[q] = 0.0;

#pragma nounroll
        for (int oc = 0; oc < depth; ++oc) {
            const RunAxisEntryD ye = ytab[oc * kRunTY + yi], ze = ztab[oc * kRunTZ + zi];
            const int Y = ycell[oc * kRunTY + yi], Z = zcell[oc * kRunTZ + zi];
            wn::run_publish_ktab(ktab, lane, ye.f, ze.f);
            const double v = ye.fade, w = ze.fade, dv = ye.dfade, dw = ze.dfade;
            const RunAxisEntry *const xe = xtab + (size_t)oc * kRunX + lane; // entry q at xe[q * 64]
            const double *const xd = xdf + (size_t)oc * kRunX + lane;
            const uint64_t cells = *reinterpret_cast<const uint64_t *>(xcell + (size_t)oc * kRunX + lane * kRun);

            // The corner state of the cell a lane is in
            double K[8], P0[3], P1[3];
            uint32_t mm[8], tt[8];
            auto hash_cell = [&](int X) {
                int h[8];
                wn::run_hash_cell(perm, X, Y, Z, ktab, h, K, mm, tt);
                __builtin_amdgcn_sched_barrier(0); // the corner blend's 24 decoded components after the table fetch
                wn::perlin_corner_blend(h, v, w, P0, P1);
            };
            // one sample; `in`: this lane's sample belongs to the cell that is hashed (else its channels stay)
            auto sample = [&](bool in, double &qv, double &qx, double &qy, double &qz, const RunAxisEntry &x, double du) {
                double gr[8], gn[3];
                wn::run_corner_gradients(K, mm, tt, x.f, gr);
                const double nv = wn::perlin_sample_grad(gr, x.fade, v, w, du, dv, dw, P0, P1, gn);
                if (KIND == kNoise) {
                    qv = in ? nv : qv;
                    qx = in ? gn[0] : qx;
                    qy = in ? gn[1] : qy;
                    qz = in ? gn[2] : qz;
                } else {
                    qv = in ? ((KIND == kTurb) ? qv + weight * nv : qv + nv * weight) : qv;
                    qx = in ? qx + gn[0] : qx;
                    qy = in ? qy + gn[1] : qy;
                    qz = in ? qz + gn[2] : qz;
                }
            };
            auto cell_at = [&](int qq) { return (int)((cells >> (8 * qq)) & 255u); };
            // Segments of the runs that stay inside one cell.  The loop over segments is rolled, so the corner state is
            // defined at one place; inside it the 8 samples are unrolled -- the sums are indexed at compile time -- and a
            // sample is skipped where no lane of the wave has it in the hashed cell.  On the BASELINE lattice, and in
            // every octave of turb up to a step of 1/8, every run is one segment: one trip.  Where the step is a power
            // of two the runs of a wave change cells together and every sample is computed once; otherwise a sample is
            // computed once per distinct cell among the wave's lanes at that position.
            uint32_t todo = 0xffu; // this lane's samples not yet computed
            do {
                const int X = cell_at(todo ? __ffs((int)todo) - 1 : 0);
                hash_cell(X);
                uint32_t mine = 0;
#pragma unroll
                for (int q = 0; q < kRun; ++q) {
                    const bool in = ((todo >> q) & 1u) && cell_at(q) == X;
                    if (__any(in)) {
                        sample(in, sv[q], sx[q], sy[q], sz[q], xe[q * 64], xd[q * 64]);
                        mine |= in ? (1u << q) : 0u;
                    }
                    __builtin_amdgcn_sched_barrier(0); // one sample at a time: the sums already hold 64 VGPRs
                }
                todo &= ~mine;
            } while (__any(todo != 0u));
            amp_sum += weight;
            weight *= 0.5;
        }

        // finish the row: turb's sign and fabs, fractal's division, then (float)channel * out_scale
        float fin[4][kRun];
#pragma unroll
        for (int q = 0; q < kRun; ++q) {
            double cv = sv[q], cx = sx[q], cy = sy[q], cz = sz[q];
            if (KIND == kTurb) {
                const bool negative = cv < 0.0;
                cv = fabs(cv);
                cx = negative ? -cx : cx;
                cy = negative ? -cy : cy;
                cz = negative ? -cz : cz;
            }
            if (KIND == kFractal) {
                cv = cv / amp_sum;
                cx = cx / amp_sum;
                cy = cy / amp_sum;
                cz = cz / amp_sum;
            }
            fin[0][q] = (float)cv * g.out_scale;
            fin[1][q] = (float)cx * g.out_scale;
            fin[2][q] = (float)cy * g.out_scale;
            fin[3][q] = (float)cz * g.out_scale;
            __builtin_amdgcn_sched_barrier(0); // one sample's four divisions at a time
        }
        // each channel's row leaves as contiguous wave stores through the wave's stage (x order)
        float *const row = a.out + ((size_t)(z_first + zi) * g.ny + (y_first + yi)) * g.nx + x_first;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); // the previous channel's reads are done
            *reinterpret_cast<v4f *>(stage + lane * kRun) = v4f{fin[c][0], fin[c][1], fin[c][2], fin[c][3]};
            *reinterpret_cast<v4f *>(stage + lane * kRun + 4) = v4f{fin[c][4], fin[c][5], fin[c][6], fin[c][7]};
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            float *const dst = row + (size_t)c * total;
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const int xo = half * 256 + lane * 4;
                wn::run_store4(dst, xo, a.vec4_ok, x_first, g.nx, *reinterpret_cast<const v4f *>(stage + xo));
            }
        }
    }
}

struct PerlinGradPointsArgs {
    const uint8_t *perm;
    const double *pts64;
    const float *pts32;
    double *out; // n records {value, d/dx, d/dy, d/dz}
    size_t count;
    int kind, depth;
};

__global__ __launch_bounds__(256) void perlin_grad_points_kernel(const PerlinGradPointsArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_perm[512];
    wn::load_perm_lds(s_perm, a.perm);
    const uint8_t *perm = s_perm;
    typedef double v2d __attribute__((ext_vector_type(2)));
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.count; i += (size_t)gridDim.x * blockDim.x) {
        double v, g[3];
        if (a.pts64) {
            const double *p = a.pts64 + 3 * i;
            v = wn::perlin_grad_exact(perm, p[0], p[1], p[2], g);
        } else {
            const float *p = a.pts32 + 3 * i;
            v = grad_vec3(perm, a.kind, a.depth, p[0], p[1], p[2], g);
        }
        v2d *const rec = reinterpret_cast<v2d *>(a.out + 4 * i);
        rec[0] = v2d{v, g[0]};
        rec[1] = v2d{g[1], g[2]};
    }
}

int perlin_grad_grid(const wn_perm *perm, const wn_grid *grid, int kind, int depth, float *out_dev, void *stream)
{
    int rc;
    PerlinGradGridArgs a;
    if (!wn::perlin_grid_frame(perm, grid, kind, depth, out_dev, "perlin gradient grid", &a, &rc)) return rc;
    const void *fn = kind == kNoise  ? reinterpret_cast<const void *>(&perlin_grad_grid_run_kernel<kNoise>)
                     : kind == kTurb ? reinterpret_cast<const void *>(&perlin_grad_grid_run_kernel<kTurb>)
                                     : reinterpret_cast<const void *>(&perlin_grad_grid_run_kernel<kFractal>);
    return wn::perlin_grid_launch(a, kRunX, fn, grad_run_lds_bytes(a.depth), grad_run_lds_bytes(kRunMaxDepth), 64 * kRunWaves,
                                  "perlin_grad_grid_run_kernel", reinterpret_cast<const void *>(&perlin_grad_grid_generic_kernel),
                                  "perlin_grad_grid_generic_kernel", stream);
}

int perlin_grad_points(const wn_perm *perm, const double *p64, const float *p32, size_t n, int kind, int depth,
                       double *out4_dev, void *stream)
{
    const int rc = wn::check_perm(perm, "perlin gradient points");
    if (rc || n == 0) return rc;
    if ((!p64 && !p32) || !out4_dev) return wn::fail(WN_ERR_INVALID, "points/out pointer is NULL");
    if (reinterpret_cast<uintptr_t>(out4_dev) & 15) return wn::fail(WN_ERR_INVALID, "out4_dev must be 16-byte aligned");
    PerlinGradPointsArgs a{perm->dev, p64, p32, out4_dev, n, kind, depth};
    hipLaunchKernelGGL(perlin_grad_points_kernel, dim3(wn::stride_blocks(n)), dim3(256), 0, wn::as_stream(stream), a);
    WN_LAUNCH_CHECK("perlin_grad_points_kernel");
    return WN_OK;
}

} // namespace

extern "C" {

int wn_perlin_grad_grid(const wn_perm *perm, const wn_grid *g, float *out_dev, void *stream)
{
    WN_ENTRY();
    return perlin_grad_grid(perm, g, kNoise, 0, out_dev, stream);
}
int wn_perlin_turb_grad_grid(const wn_perm *perm, const wn_grid *g, int depth, float *out_dev, void *stream)
{
    WN_ENTRY();
    if (depth < 0) return wn::fail(WN_ERR_INVALID, "depth must be >= 0");
    return perlin_grad_grid(perm, g, kTurb, depth, out_dev, stream);
}
int wn_perlin_fractal_grad_grid(const wn_perm *perm, const wn_grid *g, float *out_dev, void *stream)
{
    WN_ENTRY();
    return perlin_grad_grid(perm, g, kFractal, 0, out_dev, stream);
}
int wn_perlin_grad_points(const wn_perm *perm, const double *xyz_dev, size_t n, double *out4_dev, void *stream)
{
    WN_ENTRY();
    return perlin_grad_points(perm, xyz_dev, nullptr, n, kNoise, 0, out4_dev, stream);
}
int wn_perlin_grad_points_vec3(const wn_perm *perm, const float *xyz_dev, size_t n, double *out4_dev, void *stream)
{
    WN_ENTRY();
    return perlin_grad_points(perm, nullptr, xyz_dev, n, kNoise, 0, out4_dev, stream);
}
int wn_perlin_turb_grad_points(const wn_perm *perm, const float *xyz_dev, size_t n, int depth, double *out4_dev, void *stream)
{
    WN_ENTRY();
    if (depth < 0) return wn::fail(WN_ERR_INVALID, "depth must be >= 0");
    return perlin_grad_points(perm, nullptr, xyz_dev, n, kTurb, depth, out4_dev, stream);
}
int wn_perlin_fractal_grad_points(const wn_perm *perm, const float *xyz_dev, size_t n, double *out4_dev, void *stream)
{
    WN_ENTRY();
    return perlin_grad_points(perm, nullptr, xyz_dev, n, kFractal, 0, out4_dev, stream);
}

} // extern "C"
