// wn_wavelet_footprint.hip -- WMultibandNoise on point lists with the band limit taken from a footprint per point
// (include/wnoise_footprint.h): value, the projected (normal != NULL) branch, both gradients, and the texture adaptor
// wavelet_multiband_texture.  Every point is one call of wn::multiband_footprint_exact (wn_eval.hpp), which the host's
// wnhost_multiband3d_footprint compiles too: the same bits.
//
//   footprint_points_kernel<Ops>  one point per lane, grid-stride; each lane loops over its own bands.
//
// The band count differs from lane to lane, so a wave runs as long as its longest lane.  A second kernel that took lists of
// 65,536 points and more in chunks of 4096, counting-sorted in LDS by (band count, z plane of the finest band) so that a
// wave's lanes ran the same number of bands, with the records returned to stream order through LDS, was built and measured
// on 16 M uniformly random points with the band counts 0 .. 5 evenly mixed: 2,689 us against this kernel's 2,501 us
// (profiles/footprint_kernels.txt).  The gathers of scattered points are bound by L1 misses, not by issue slots: a lane
// that has run out of bands stops missing, which is what this kernel already gains, and the sorting passes and the lower
// occupancy cost more than lock-step waves return.  It was dropped; one kernel serves every list length.
#include "wn_internal.hpp"
#include "wnoise_footprint.h"

#include <cmath>

namespace {

static_assert(wn::kFootprintMaxBands == wn::kMaxBands, "one band limit for the uniform and the footprint entry points");

enum Kind { kValue, kProjected, kGrad, kProjectedGrad, kTexture };

struct FootprintArgs : wn::FootprintBands {
    const float *coef; // the padded tile; projected kinds: the linear layout
    int n, nmask;
    const float *pts;      // xyz interleaved
    const float *normals;  // projected kinds: xyz per point, or one for all (one_normal)
    const float *s;        // the footprint of every point
    const uint8_t *active; // texture: NULL, or one byte per point
    float *out;            // one float per point; gradient kinds: four (16-byte aligned)
    size_t count;
    int one_normal;
    double scale; // texture
};

// What a point is to the kernel: active(i); eval(i, r); store(i, r).
template <int KIND, bool MASKED>
struct FootprintOps {
    static constexpr int kChannels = (KIND == kGrad || KIND == kProjectedGrad) ? 4 : 1;
    static constexpr bool kProjectedKind = KIND == kProjected || KIND == kProjectedGrad;
    FootprintArgs a;
    __device__ bool active(size_t i) const { return !MASKED || a.active[i] != 0; }
    __device__ void eval(size_t i, float r[kChannels]) const
    {
        const float p[3] = {a.pts[3 * i], a.pts[3 * i + 1], a.pts[3 * i + 2]};
        const float s = a.s[i];
        if constexpr (KIND == kTexture) {
            r[0] = wn::wavelet_multiband_texture_value<true>(a, p[0], p[1], p[2], s);
        } else if constexpr (kProjectedKind) {
            const float *nrp = a.normals + (a.one_normal ? 0 : 3 * i);
            const float nr[3] = {nrp[0], nrp[1], nrp[2]};
            if constexpr (KIND == kProjectedGrad) r[0] = wn::multiband_footprint_exact<false, true, true>(a, p, nr, s, r + 1);
            else r[0] = wn::multiband_footprint_exact<false, true, false>(a, p, nr, s, nullptr);
        } else if constexpr (KIND == kGrad) {
            r[0] = wn::multiband_footprint_exact<true, false, true>(a, p, nullptr, s, r + 1);
        } else {
            r[0] = wn::multiband_footprint_exact<true, false, false>(a, p, nullptr, s, nullptr);
        }
    }
    __device__ void store(size_t i, const float r[kChannels]) const
    {
        if constexpr (kChannels == 4) reinterpret_cast<v4f *>(a.out)[i] = v4f{r[0], r[1], r[2], r[3]};
        else a.out[i] = r[0];
    }
};

template <typename Ops>
__global__ __launch_bounds__(256) void footprint_points_kernel(const Ops ops)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < ops.a.count; i += (size_t)gridDim.x * blockDim.x)
        if (ops.active(i)) {
            float r[Ops::kChannels];
            ops.eval(i, r);
            ops.store(i, r);
        }
}

template <typename Ops>
int launch(const Ops &ops, hipStream_t stream)
{
    hipLaunchKernelGGL((footprint_points_kernel<Ops>), dim3(wn::stride_blocks(ops.a.count)), dim3(256), 0, stream, ops);
    WN_LAUNCH_CHECK("footprint_points_kernel");
    return WN_OK;
}

// The checks of wn_multiband3d_points and its twins, in their order: the tile, the bands, then -- for a list that is not
// empty -- the pointers and, for float4 records, out's 16-byte alignment.
template <int KIND>
int footprint_entry(const char *entry, const wn_tile *tile, const float *xyz, const float *normals, int one_normal,
                    const float *s_dev, size_t n, int first_band, int nbands, const float *w_host, float var_per_band,
                    int fade, double scale, const uint8_t *active, float *out, void *stream)
{
    constexpr bool projected = KIND == kProjected || KIND == kProjectedGrad;
    constexpr bool grad = KIND == kGrad || KIND == kProjectedGrad;
    const int rc = wn::check_tile(tile, 3, entry);
    if (rc) return rc;
    if (nbands < 0 || nbands > wn::kFootprintMaxBands)
        return wn::fail(WN_ERR_INVALID, "nbands must be in 0..%d (got %d)", wn::kFootprintMaxBands, nbands);
    if (nbands && !w_host) return wn::fail(WN_ERR_INVALID, "w_host is NULL");
    if (n == 0) return WN_OK;
    if (!xyz || !out) return wn::fail(WN_ERR_INVALID, "points/out pointer is NULL");
    if (!s_dev) return wn::fail(WN_ERR_INVALID, "s_dev is NULL");
    if (projected && !normals) return wn::fail(WN_ERR_INVALID, "normals_dev is NULL");
    if (grad && (reinterpret_cast<uintptr_t>(out) & 15)) return wn::fail(WN_ERR_INVALID, "out4_dev must be 16-byte aligned");
    if (!projected && tile->count && !tile->dev_padded) return wn::fail(WN_ERR_INVALID, "%s: the tile has no padded copy", entry);
    FootprintArgs a{};
    wn::footprint_bands_fill(first_band, nbands, w_host, var_per_band, fade, &a);
    a.coef = projected ? tile->dev : tile->dev_padded; // an empty tile: never read
    a.n = tile->count ? tile->n : 0;
    a.nmask = wn::pow2_mask(a.n);
    a.pts = xyz;
    a.normals = normals;
    a.s = s_dev;
    a.active = active;
    a.out = out;
    a.count = n;
    a.one_normal = one_normal ? 1 : 0;
    a.scale = scale;
    if constexpr (KIND == kTexture)
        if (active) return launch(FootprintOps<KIND, true>{a}, wn::as_stream(stream));
    return launch(FootprintOps<KIND, false>{a}, wn::as_stream(stream));
}

} // namespace

extern "C" {

int wn_multiband3d_footprint_points(const wn_tile *tile, const float *xyz_dev, const float *s_dev, size_t n, int first_band,
                                    int nbands, const float *w_host, float var_per_band, int fade, float *out_dev,
                                    void *stream)
{
    WN_ENTRY();
    return footprint_entry<kValue>("wn_multiband3d_footprint_points", tile, xyz_dev, nullptr, 0, s_dev, n, first_band, nbands,
                                   w_host, var_per_band, fade, 1.0, nullptr, out_dev, stream);
}

int wn_multiband3d_projected_footprint_points(const wn_tile *tile, const float *xyz_dev, const float *normals_dev,
                                              int one_normal, const float *s_dev, size_t n, int first_band, int nbands,
                                              const float *w_host, float var_per_band, int fade, float *out_dev,
                                              void *stream)
{
    WN_ENTRY();
    return footprint_entry<kProjected>("wn_multiband3d_projected_footprint_points", tile, xyz_dev, normals_dev, one_normal,
                                       s_dev, n, first_band, nbands, w_host, var_per_band, fade, 1.0, nullptr, out_dev, stream);
}

int wn_multiband3d_footprint_grad_points(const wn_tile *tile, const float *xyz_dev, const float *s_dev, size_t n,
                                         int first_band, int nbands, const float *w_host, float var_per_band, int fade,
                                         float *out4_dev, void *stream)
{
    WN_ENTRY();
    return footprint_entry<kGrad>("wn_multiband3d_footprint_grad_points", tile, xyz_dev, nullptr, 0, s_dev, n, first_band,
                                  nbands, w_host, var_per_band, fade, 1.0, nullptr, out4_dev, stream);
}

int wn_multiband3d_projected_footprint_grad_points(const wn_tile *tile, const float *xyz_dev, const float *normals_dev,
                                                   int one_normal, const float *s_dev, size_t n, int first_band,
                                                   int nbands, const float *w_host, float var_per_band, int fade,
                                                   float *out4_dev, void *stream)
{
    WN_ENTRY();
    return footprint_entry<kProjectedGrad>("wn_multiband3d_projected_footprint_grad_points", tile, xyz_dev, normals_dev,
                                           one_normal, s_dev, n, first_band, nbands, w_host, var_per_band, fade, 1.0,
                                           nullptr, out4_dev, stream);
}

int wn_wavelet_multiband_texture_points(const wn_tile *tile, double scale, int first_band, int nbands, const float *w_host,
                                        float var_per_band, int fade, const float *xyz_dev, const float *s_dev,
                                        const uint8_t *active_dev, size_t n, float *grey_dev, void *stream)
{
    WN_ENTRY();
    return footprint_entry<kTexture>("wn_wavelet_multiband_texture_points", tile, xyz_dev, nullptr, 0, s_dev, n, first_band,
                                     nbands, w_host, var_per_band, fade, scale, active_dev, grey_dev, stream);
}

} // extern "C"
