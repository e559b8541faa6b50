// wn_perlin_footprint.hip -- Perlin turb and fractal_noise on point lists with the octave limit taken from a footprint per
// point (include/wnoise_perlin_footprint.h): both values, both gradients, and the texture adaptor noise_multiband_texture.
// Every point is one call of wn::perlin_turb_footprint / perlin_fractal_footprint / noise_multiband_texture_value
// (wn_eval.hpp), which host/scalar_eval.cpp compiles too: the same bits, whichever kernel serves the list.
//
//   perlin_footprint_points_kernel<Ops>  one point per lane, grid-stride, the table in LDS (perlin_points_kernel's shape);
//                                        each lane loops over its own octaves.  Lists shorter than kSortMinPoints.
//   perlin_footprint_sorted_kernel<Ops>  one workgroup per chunk of kChunk consecutive points, counting-sorted in LDS by
//                                        octave count so that the 64 lanes of a wave run the same number of octaves.
//
// These lists are bound by fp64 VALU, not by memory: the table is in LDS and a point is 16 bytes in, 8 to 32 out.  A wave
// whose lanes loop over their own octave counts runs as long as its longest lane, so with the counts mixed the per-lane
// kernel gains little from the octaves it drops; the sorted kernel turns dropped octaves into dropped instructions.
// (For the wavelet lists of wn_wavelet_footprint.hip the same sort lost: those are bound by L1 misses, and a lane that has
// run out of bands stops missing.)  Measured on 16 M points with the counts 0 .. 7 mixed: 470 us sorted, 650 us per lane, 675 us
// for turb(7) everywhere (profiles/perlin_footprint_kernels.txt).
#include "wn_device_eval.hpp"
#include "wn_internal.hpp"
#include "wnoise_perlin_footprint.h"

#include <cmath>

// Lists of at least this many points take the sorted kernel: 2^20 is the measured crossover (38.4 against 44.4 us; at 2^19 the
// per-lane kernel still wins, 23.8 against 26.1 us).  A build-time macro so that profiles/perlin_footprint_timing.py can time
// either kernel alone on every length (0: the sorted kernel always; SIZE_MAX: never).
#ifndef WN_PERLIN_FOOTPRINT_SORT_MIN_POINTS
#define WN_PERLIN_FOOTPRINT_SORT_MIN_POINTS (size_t(1) << 20)
#endif

namespace {

constexpr size_t kSortMinPoints = WN_PERLIN_FOOTPRINT_SORT_MIN_POINTS;
// Points per chunk of the sorted kernel: 4 per lane, 16 waves of sorted positions.  Chunks of 4096 (16 per lane) measured
// slower on every length of the value sweep: a lane walks its points one after the other, so a list of 2^20 points was 256
// serial chains of 16 on 256 compute units (71 against 39 us), and at 16 M points the short chunk still won (470 against
// 487 us; only the gradient call pays for it there, 845 against 833 us).  A smaller pool sorts less well, but neighbouring
// bins differ by one octave, so a wave that straddles a boundary loses little.
constexpr int kChunk = 1024;
constexpr int kLanes = 256;
constexpr int kBins = wn::kPerlinFootprintMaxOctaves + 1; // octave counts 0 .. 16 (bin 0 stays empty)
static_assert(kChunk <= 65536 && kChunk % kLanes == 0, "16-bit local indices, whole rounds of the workgroup");

enum Kind { kTurbValue, kFractalValue, kTurbGrad, kFractalGrad, kTexture };

struct PerlinFootprintArgs {
    const uint8_t *perm;
    const float *pts;      // xyz interleaved
    const float *s;        // the footprint of every point
    const uint8_t *active; // texture: NULL, or one byte per point
    double *out;           // one double per point; gradient kinds: four (16-byte aligned)
    float *grey;           // texture
    size_t count;
    int octaves; // turb: depth
    float bias;
    int fade;
    float fscale; // texture: (float)scale
};

// What a point is to the kernels: active(i); octave_count(i); eval(perm, i, r); store(i, r); store_none(i) -- the record
// of a point without an active octave, the evaluator's result for it.
template <int KIND, bool MASKED>
struct PerlinFootprintOps {
    static constexpr int kChannels = (KIND == kTurbGrad || KIND == kFractalGrad) ? 4 : 1;
    PerlinFootprintArgs a;
    __device__ bool active(size_t i) const { return !MASKED || a.active[i] != 0; }
    __device__ int octave_count(size_t i) const { return wn::perlin_footprint_count(a.s[i], a.bias, a.octaves); }
    __device__ void eval(const uint8_t *perm, size_t i, double r[kChannels]) const
    {
        const float x = a.pts[3 * i], y = a.pts[3 * i + 1], z = a.pts[3 * i + 2];
        const float s = a.s[i];
        if constexpr (KIND == kTexture)
            r[0] = (double)wn::noise_multiband_texture_value(perm, a.fscale, a.octaves, a.bias, a.fade, x, y, z, s);
        else if constexpr (KIND == kTurbValue) r[0] = wn::perlin_turb_footprint<false>(perm, x, y, z, a.octaves, s, a.bias, a.fade, nullptr);
        else if constexpr (KIND == kFractalValue) r[0] = wn::perlin_fractal_footprint<false>(perm, x, y, z, a.octaves, s, a.bias, a.fade, nullptr);
        else if constexpr (KIND == kTurbGrad) r[0] = wn::perlin_turb_footprint<true>(perm, x, y, z, a.octaves, s, a.bias, a.fade, r + 1);
        else r[0] = wn::perlin_fractal_footprint<true>(perm, x, y, z, a.octaves, s, a.bias, a.fade, r + 1);
    }
    __device__ void store(size_t i, const double r[kChannels]) const
    {
        typedef double v2d __attribute__((ext_vector_type(2)));
        if constexpr (KIND == kTexture) a.grey[i] = (float)r[0]; // r[0] holds a float: the cast is exact
        else if constexpr (kChannels == 4) {
            v2d *const rec = reinterpret_cast<v2d *>(a.out + 4 * i);
            rec[0] = v2d{r[0], r[1]};
            rec[1] = v2d{r[2], r[3]};
        } else a.out[i] = r[0];
    }
    __device__ void store_none(size_t i) const
    {
        double r[kChannels];
        for (int c = 0; c < kChannels; ++c) r[c] = 0.0;
        if constexpr (KIND == kTexture) r[0] = 0.5; // (float)(0.5 * (1.0 + 0.0))
        store(i, r);
    }
};

template <typename Ops>
__global__ __launch_bounds__(kLanes) void perlin_footprint_points_kernel(const Ops ops)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_perm[512];
    wn::load_perm_lds(s_perm, ops.a.perm);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < ops.a.count; i += (size_t)gridDim.x * blockDim.x)
        if (ops.active(i)) {
            double r[Ops::kChannels];
            ops.eval(s_perm, i, r);
            ops.store(i, r);
        }
}

// Pass 1, stream order: every lane forms the octave count k of its points, writes the record of those with k == 0 and
// counts the others into the bins.  Scan: the bins' first sorted positions, longest count first, so that the longest
// waves start first and the tail is short.  Scatter: every lane writes the local index of its points with k > 0 to the
// next free position of bin k (the order inside a bin is free: no result depends on it).  Pass 2: lanes walk the sorted
// positions 256 at a time, gather their point from the chunk's window (12 KB of xyz and 4 KB of s, read by pass 1),
// evaluate it and store the record at the point's own index; only a wave that straddles a bin boundary runs mixed counts.
template <typename Ops>
__global__ __launch_bounds__(kLanes) void perlin_footprint_sorted_kernel(const Ops ops, const size_t chunks)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_perm[512];
    __shared__ uint16_t s_sorted[kChunk];
    __shared__ int s_bins[kBins];
    wn::load_perm_lds(s_perm, ops.a.perm);
    const int tid = threadIdx.x;
    for (size_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const size_t base = c * (size_t)kChunk;
        const int len = (int)min((size_t)kChunk, ops.a.count - base);
        if (tid < kBins) s_bins[tid] = 0;
        __syncthreads();
        for (int l = tid; l < len; l += kLanes) {
            if (!ops.active(base + l)) continue;
            const int k = ops.octave_count(base + l);
            if (k == 0) ops.store_none(base + l);
            else atomicAdd(&s_bins[k], 1);
        }
        __syncthreads();
        if (tid == 0) {
            int first = 0;
            for (int k = kBins - 1; k >= 1; --k) {
                const int cnt = s_bins[k];
                s_bins[k] = first;
                first += cnt;
            }
            s_bins[0] = first; // the number of points to evaluate
        }
        __syncthreads();
        const int total = s_bins[0]; // bin 0 is not bumped below
        for (int l = tid; l < len; l += kLanes) {
            if (!ops.active(base + l)) continue;
            const int k = ops.octave_count(base + l);
            if (k == 0) continue;
            const int pos = atomicAdd(&s_bins[k], 1); // < total <= len <= kChunk while s_dev holds what pass 1 read
            if (pos < kChunk) s_sorted[pos] = (uint16_t)l;
        }
        __syncthreads();
        for (int pos = tid; pos < total; pos += kLanes) {
            const int l = s_sorted[pos];
            if (l >= len) continue; // cannot happen while s_dev holds what pass 1 read; never write outside the list
            const size_t i = base + l;
            double r[Ops::kChannels];
            ops.eval(s_perm, i, r);
            ops.store(i, r);
        }
        __syncthreads(); // the sorted positions are read before the next chunk's scatter
    }
}

template <typename Ops>
int launch(const Ops &ops, hipStream_t stream)
{
    const size_t n = ops.a.count;
    if (n >= kSortMinPoints) {
        const size_t chunks = (n + kChunk - 1) / kChunk;
        const size_t blocks = chunks < wn::kStrideBlockCap ? chunks : wn::kStrideBlockCap;
        hipLaunchKernelGGL((perlin_footprint_sorted_kernel<Ops>), dim3((unsigned)blocks), dim3(kLanes), 0, stream, ops, chunks);
        WN_LAUNCH_CHECK("perlin_footprint_sorted_kernel");
        return WN_OK;
    }
    hipLaunchKernelGGL((perlin_footprint_points_kernel<Ops>), dim3(wn::stride_blocks(n)), dim3(kLanes), 0, stream, ops);
    WN_LAUNCH_CHECK("perlin_footprint_points_kernel");
    return WN_OK;
}

// The checks of the Perlin point entry points, in their order, with the octave range in front of the list's length.
template <int KIND>
int footprint_entry(const char *entry, const wn_perm *perm, const float *xyz, const float *s_dev, const uint8_t *active,
                    size_t n, int octaves, float bias, int fade, double scale, void *out, void *stream)
{
    constexpr bool grad = KIND == kTurbGrad || KIND == kFractalGrad;
    const int rc = wn::check_perm(perm, entry);
    if (rc) return rc;
    if (octaves < 0 || octaves > wn::kPerlinFootprintMaxOctaves)
        return wn::fail(WN_ERR_INVALID, "%s must be in 0..%d (got %d)", (KIND == kTurbValue || KIND == kTurbGrad) ? "depth" : "octaves",
                        wn::kPerlinFootprintMaxOctaves, octaves);
    if (n == 0) return WN_OK;
    if (!xyz || !out) return wn::fail(WN_ERR_INVALID, "points/out pointer is NULL");
    if (!s_dev) return wn::fail(WN_ERR_INVALID, "s_dev is NULL");
    if (grad && (reinterpret_cast<uintptr_t>(out) & 15)) return wn::fail(WN_ERR_INVALID, "out4_dev must be 16-byte aligned");
    PerlinFootprintArgs a{};
    a.perm = perm->dev;
    a.pts = xyz;
    a.s = s_dev;
    a.active = active;
    if constexpr (KIND == kTexture) a.grey = static_cast<float *>(out);
    else a.out = static_cast<double *>(out);
    a.count = n;
    a.octaves = octaves;
    a.bias = bias;
    a.fade = fade ? 1 : 0;
    a.fscale = (float)scale;
    if constexpr (KIND == kTexture)
        if (active) return launch(PerlinFootprintOps<KIND, true>{a}, wn::as_stream(stream));
    return launch(PerlinFootprintOps<KIND, false>{a}, wn::as_stream(stream));
}

} // namespace

extern "C" {

int wn_perlin_turb_footprint_points(const wn_perm *perm, const float *xyz_dev, const float *s_dev, size_t n, int depth,
                                    float bias, int fade, double *out_dev, void *stream)
{
    WN_ENTRY();
    return footprint_entry<kTurbValue>("wn_perlin_turb_footprint_points", perm, xyz_dev, s_dev, nullptr, n, depth, bias, fade,
                                       1.0, out_dev, stream);
}

int wn_perlin_fractal_footprint_points(const wn_perm *perm, const float *xyz_dev, const float *s_dev, size_t n, int octaves,
                                       float bias, int fade, double *out_dev, void *stream)
{
    WN_ENTRY();
    return footprint_entry<kFractalValue>("wn_perlin_fractal_footprint_points", perm, xyz_dev, s_dev, nullptr, n, octaves, bias,
                                          fade, 1.0, out_dev, stream);
}

int wn_perlin_turb_footprint_grad_points(const wn_perm *perm, const float *xyz_dev, const float *s_dev, size_t n, int depth,
                                         float bias, int fade, double *out4_dev, void *stream)
{
    WN_ENTRY();
    return footprint_entry<kTurbGrad>("wn_perlin_turb_footprint_grad_points", perm, xyz_dev, s_dev, nullptr, n, depth, bias,
                                      fade, 1.0, out4_dev, stream);
}

int wn_perlin_fractal_footprint_grad_points(const wn_perm *perm, const float *xyz_dev, const float *s_dev, size_t n,
                                            int octaves, float bias, int fade, double *out4_dev, void *stream)
{
    WN_ENTRY();
    return footprint_entry<kFractalGrad>("wn_perlin_fractal_footprint_grad_points", perm, xyz_dev, s_dev, nullptr, n, octaves,
                                         bias, fade, 1.0, out4_dev, stream);
}

int wn_noise_multiband_texture_points(const wn_perm *perm, double scale, int octaves, float bias, int fade,
                                      const float *xyz_dev, const float *s_dev, const uint8_t *active_dev, size_t n,
                                      float *grey_dev, void *stream)
{
    WN_ENTRY();
    return footprint_entry<kTexture>("wn_noise_multiband_texture_points", perm, xyz_dev, s_dev, active_dev, n, octaves, bias,
                                     fade, scale, grey_dev, stream);
}

} // extern "C"
