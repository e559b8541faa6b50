// wn_perlin_frame.hpp -- the frame of the dense Perlin grids: what the value, gradient and curl kernels of wn_perlin.hip,
// wn_perlin_grad.hip and wn_perlin_curl.hip share, stated once.  The grids promise the bits of the point kernels, so the
// octave walk, the hashes and the routing rule must not exist in copies that can drift.
//
// The run form (perlin_grid_run_kernel, perlin_grad_grid_run_kernel, perlin_curl_grid_run_kernel) is built around what
// consecutive samples of an axis-aligned lattice SHARE (perlin.h:42-62 evaluated for a whole block):
//   * everything per axis is per axis: floor / fractional part / fade of a coordinate depend on one index only.  A workgroup
//     owns kRunX x samples x kRunTY rows x <= kRunTZ planes and first tabulates, per octave, the fractional part, its fade
//     and the cell index for its x samples, rows and planes (LDS; fp64, the reference's operation order);
//   * a lane walks a RUN of consecutive x samples of one row.  The eight corner hashes p[p[p[X]+Y]+Z] ... (perlin.h:55-61:
//     14 table look-ups) and everything derived from them are computed once per cell the run enters (at the BASELINE
//     lattice -- step 1/8 per sample -- once per run), not once per sample;
//   * grad() (perlin.h:26-31) picks two of (x,y,z) and two signs from the low 4 hash bits.  Inside a run only x moves, so a
//     corner's gradient is  (+-dx | nothing) + K  with K = (+-dy) + (+-dz), +-dy or +-dz, a per-row constant
//     (wn_perlin_run.hpp).  Per row and octave the wave builds a 64-entry LDS table [cy][cz][h] -> {K, and-mask, sign-xor}
//     with one lane per entry; a lane fetches its 8 corners' entries with 8 ds_read_b128;
//   * per sample what is left is 8 x (2 and + 1 xor + 1 fp64 add) for the gradients and the lerps (unfused, reference order).
// Each kernel keeps what is its own: the LDS layout, the walk over the cells a run crosses, accumulation and finishing.
// The brick kernels (wn_perlin_bricks.hip) are the same form on rows of 8 samples, one row per lane: they take the octave walk
// (RunOctaveWalker), the hashes (run_hash_corners) and the corner entries in registers (run_corner_entries) from here.
#pragma once

#include "wn_internal.hpp"
#include "wn_device_eval.hpp"
#include "wn_perlin_run.hpp"

namespace wn {

enum { kNoise = 0, kTurb = 1, kFractal = 2 };
constexpr int kFractalOctaves = 6; // perlin::fractal_noise (perlin.h:82-84)
constexpr int perlin_octaves(int kind, int depth) { return kind == kNoise ? 1 : (kind == kFractal ? kFractalOctaves : depth); }

constexpr int kRunMaxDepth = 8; // octaves the run form tabulates
constexpr int kRunTY = 8;       // rows ...
constexpr int kRunTZ = 8;       // ... and planes per workgroup

// What the grid kernels' argument structs begin with.
struct PerlinGridFrame {
    const uint8_t *perm;
    float *out; // consecutive channel volumes
    GridArgs g;
    int kind, depth; // depth: the octaves of the call (perlin_octaves)
    int vec4_ok;     // rows of every channel start 16-byte aligned (nx % 4 == 0 and an aligned output pointer)
};

// ---- host side ----------------------------------------------------------------------------------------------------------
// The first checks of a grid entry point (`entry` names it in the message).  true: *f is filled, launch.  false: return
// *rc (an error, or WN_OK for an empty lattice).
inline bool perlin_grid_frame(const wn_perm *perm, const wn_grid *grid, int kind, int depth, float *out_dev, const char *entry,
                              PerlinGridFrame *f, int *rc)
{
    if ((*rc = check_perm(perm, entry)) != WN_OK) return false;
    GridArgs g;
    if ((*rc = check_grid(grid, true, &g)) != WN_OK) return false;
    if ((size_t)g.nx * g.ny * g.nz == 0) return false;
    if (!out_dev) *rc = fail(WN_ERR_INVALID, "out_dev is NULL");
    else if ((size_t)g.nx * g.ny > 0xffffffffull) *rc = fail(WN_ERR_INVALID, "plane too large");
    if (*rc != WN_OK) return false;
    *f = PerlinGridFrame{perm->dev, out_dev, g, kind, perlin_octaves(kind, depth), vec4_ok(out_dev, g.nx)};
    return true;
}

// The run form serves rows of >= 128 samples (a lane owns a run of consecutive x samples) at 1..kRunMaxDepth octaves, in
// workgroups of run_x x kRunTY x kRunTZ samples.
inline bool perlin_run_eligible(const GridArgs &g, int octaves, int run_x, dim3 *rgrid)
{
    *rgrid = dim3((g.nx + run_x - 1) / run_x, (g.ny + kRunTY - 1) / kRunTY, (g.nz + kRunTZ - 1) / kRunTZ);
    return g.nx >= 128 && octaves >= 1 && octaves <= kRunMaxDepth && rgrid->y <= 65535u && rgrid->z <= 65535u;
}

// Launches the run form `run_fn` (workgroups of `block` lanes and run_x x samples, `lds` bytes of dynamic LDS, lds_max at
// kRunMaxDepth) where it is eligible, else the sample-per-lane kernel `generic_fn`.
template <typename Args>
int perlin_grid_launch(Args &a, int run_x, const void *run_fn, size_t lds, size_t lds_max, int block, const char *run_name,
                       const void *generic_fn, const char *generic_name, void *stream)
{
    void *params[] = {&a};
    dim3 rgrid;
    if (perlin_run_eligible(a.g, a.depth, run_x, &rgrid) &&
        (lds <= 48 * 1024 || ensure_dynamic_lds(run_fn, current_device(), lds_max))) {
        const hipError_t e = hipLaunchKernel(run_fn, rgrid, dim3(block), params, lds, as_stream(stream));
        if (e != hipSuccess) return hip_fail(e, run_name);
        WN_LAUNCH_CHECK(run_name);
        return WN_OK;
    }
    const size_t total = (size_t)a.g.nx * a.g.ny * a.g.nz;
    const hipError_t e = hipLaunchKernel(generic_fn, dim3(stride_blocks(total)), dim3(256), params, 0, as_stream(stream));
    if (e != hipSuccess) return hip_fail(e, generic_name);
    WN_LAUNCH_CHECK(generic_name);
    return WN_OK;
}

// ---- the generic kernels: one sample per lane, every sample hashes for itself ---------------------------------------------
// Grid-stride loop over the lattice (a plane has < 2^32 samples): body(e, total, px, py, pz) for sample e of total, x fastest.
template <typename Body>
__device__ __forceinline__ void perlin_for_each_sample(const GridArgs &g, Body &&body)
{
    const float den = (float)g.den;
    const unsigned plane = (unsigned)g.nx * (unsigned)g.ny;
    const size_t total = (size_t)plane * g.nz;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const unsigned z = (unsigned)(e / plane);
        const unsigned r = (unsigned)(e - (size_t)z * plane);
        const unsigned y = r / (unsigned)g.nx, x = r - y * (unsigned)g.nx;
        body(e, total, grid_coord(g, den, (int)x), grid_coord(g, den, (int)y), grid_zcoord(g, den, (int)z));
    }
}

// ---- the run form: tables of the block ----------------------------------------------------------------------------------
struct RunAxisEntry {
    double f, fade; // fractional part and its fade()
    static __device__ __forceinline__ RunAxisEntry of(double f) { return RunAxisEntry{f, pfade(f)}; }
};
struct RunAxisEntryD {
    double f, fade, dfade; // ... and fade'()
    static __device__ __forceinline__ RunAxisEntryD of(double f) { return RunAxisEntryD{f, pfade(f), pfade_d(f)}; }
};

// The octaves of a run kernel: known at compile time for noise and fractal_noise; turb's depth comes from the host.
template <int KIND, typename Args>
__device__ __forceinline__ int run_depth(const Args &a)
{
    return (KIND == kNoise) ? 1 : ((KIND == kFractal) ? kFractalOctaves : a.depth);
}

__device__ __forceinline__ void run_load_perm(uint8_t *perm, const uint8_t *gperm, int tid, int threads)
{
    for (int i = tid; i < 128; i += threads) reinterpret_cast<uint32_t *>(perm)[i] = reinterpret_cast<const uint32_t *>(gperm)[i];
}

// The octave walk of coordinate p, one octave per step(): store(cell, f) with the lattice cell (& 255) and the fractional
// part.  The dense run kernels walk all octaves at once (run_octave_walk); the brick kernels (wn_perlin_bricks.hip) keep a
// walker per axis index and tabulate one octave at a time, so they have no depth cap.
template <int KIND>
struct RunOctaveWalker {
    float p;
    float cur = p;          // turb: the float point doubles per octave
    double frequency = 1.0; // fractal_noise: float point times a double frequency (perlin.h:82-84)
    template <typename Store>
    __device__ __forceinline__ void step(Store &&store)
    {
        const double c = (KIND == kFractal) ? (double)p * frequency : (double)cur;
        const double fl = floor(c);
        store((int)fl & 255, c - fl);
        cur *= 2.0f;
        frequency *= 2.0;
    }
};

// ... of all `depth` octaves: store(octave, cell, f).
template <int KIND, typename Store>
__device__ __forceinline__ void run_octave_walk(float p, int depth, Store &&store)
{
    RunOctaveWalker<KIND> walker{p};
    for (int i = 0; i < depth; ++i) walker.step([&](int cell, double f) { store(i, cell, f); });
}

// Coordinate of x / y sample i of n, and of plane zi of the call; a block's tail repeats the last sample.
__device__ __forceinline__ float run_coord(const GridArgs &g, float den, int i, int n) { return grid_coord(g, den, min(i, n - 1)); }
__device__ __forceinline__ float run_zcoord(const GridArgs &g, float den, int zi) { return grid_zcoord(g, den, min(zi, g.nz - 1)); }

// The row and plane tables of the block, [octave][kRunTY] and [octave][kRunTZ]: entries and cell indices.
template <int KIND, typename Entry>
__device__ __forceinline__ void run_tabulate_yz(const GridArgs &g, float den, int depth, int y_first, int z_first, int tid,
                                                Entry *ytab, Entry *ztab, int *ycell, int *zcell)
{
    if (tid < kRunTY) {
        run_octave_walk<KIND>(run_coord(g, den, y_first + tid, g.ny), depth, [&](int i, int cell, double f) {
            ytab[i * kRunTY + tid] = Entry::of(f);
            ycell[i * kRunTY + tid] = cell;
        });
    } else if (tid >= 64 && tid < 64 + kRunTZ) {
        const int zi = tid - 64;
        run_octave_walk<KIND>(run_zcoord(g, den, z_first + zi), depth, [&](int i, int cell, double f) {
            ztab[i * kRunTZ + zi] = Entry::of(f);
            zcell[i * kRunTZ + zi] = cell;
        });
    }
}

// ---- the run form: per row, cell and sample -----------------------------------------------------------------------------
// Per-row table of a wave: entry (cy, cz, h) -> {K, mm, t} (grad(), perlin.h:26-31) from the row's fractional parts, one
// lane per entry.
__device__ __forceinline__ void run_publish_ktab(RunKEntry *ktab, int lane, double yf, double zf)
{
    const int kh = lane & 15, kcy = (lane >> 4) & 1, kcz = lane >> 5;
    const double dy = kcy ? yf - 1.0 : yf, dz = kcz ? zf - 1.0 : zf;
    const RunKEntry mine = run_k_entry(kh, dy, dz);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); // the previous octave's reads are done
    ktab[lane] = mine;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}

// Hashes the 8 corners of cell (X, Y, Z) (perlin.h:55-61): corner c = cx + 2 cy + 4 cz.
__device__ __forceinline__ void run_hash_corners(const uint8_t *perm, int X, int Y, int Z, int (&h)[8])
{
    const int A = perm[X] + Y, AA = perm[A] + Z, AB = perm[A + 1] + Z;
    const int B = perm[X + 1] + Y, BA = perm[B] + Z, BB = perm[B + 1] + Z;
    h[0] = perm[AA], h[1] = perm[BA], h[2] = perm[AB], h[3] = perm[BB];
    h[4] = perm[AA + 1], h[5] = perm[BA + 1], h[6] = perm[AB + 1], h[7] = perm[BB + 1];
}

// ... and fetches their {K, mm, t} from the row's table.
__device__ __forceinline__ void run_hash_cell(const uint8_t *perm, int X, int Y, int Z, const RunKEntry *ktab, int (&h)[8],
                                              double (&K)[8], uint32_t (&mm)[8], uint32_t (&tt)[8])
{
    run_hash_corners(perm, X, Y, Z, h);
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const RunKEntry e = ktab[(c >> 1) * 16 + (h[c] & 15)];
        K[c] = e.K;
        mm[c] = e.mm;
        tt[c] = e.t;
    }
}

// The 8 corners' {K, mm, t} formed in registers from the hashes: run_publish_ktab's entries without the table, for a lane
// whose row is its own (wn_perlin_bricks.hip: the 64 lanes of a wave hold 64 rows, so there is no row a table could serve).
__device__ __forceinline__ void run_corner_entries(const int (&h)[8], double yf, double zf, double (&K)[8], uint32_t (&mm)[8],
                                                   uint32_t (&tt)[8])
{
    const double ym1 = yf - 1.0, zm1 = zf - 1.0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const RunKEntry e = run_k_entry(h[c] & 15, (c & 2) ? ym1 : yf, (c & 4) ? zm1 : zf);
        K[c] = e.K;
        mm[c] = e.mm;
        tt[c] = e.t;
    }
}

// The 8 corner gradients of the sample at fractional part xf of the hashed cell.
__device__ __forceinline__ void run_corner_gradients(const double (&K)[8], const uint32_t (&mm)[8], const uint32_t (&tt)[8],
                                                     double xf, double (&gr)[8])
{
    const double xm1 = xf - 1.0;
    const uint64_t b0 = (uint64_t)__double_as_longlong(xf), b1 = (uint64_t)__double_as_longlong(xm1);
#pragma unroll
    for (int c = 0; c < 8; ++c) gr[c] = run_gradient(K[c], mm[c], tt[c], (c & 1) ? b1 : b0);
}

// Stores samples xo .. xo + 3 of a block's row (row: its first sample, sample x_first of the nx of the lattice's row): one
// float4, or scalars where rows are not 16-byte aligned or the lattice's row ends inside the 4.
__device__ __forceinline__ void run_store4(float *row, int xo, int vec4_ok, int x_first, int nx, v4f val)
{
    if (vec4_ok && x_first + xo + 4 <= nx) *reinterpret_cast<v4f *>(row + xo) = val;
    else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (x_first + xo + e < nx) row[xo + e] = val[e];
    }
}

} // namespace wn
