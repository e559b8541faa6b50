// WaveletNoise.cpp -- host side of class WaveletNoise over libwnoise_hip.so: tile filtering and every evaluation of
// more than one sample are HIP kernels behind include/wnoise.h; the scalar members (one sample, needed at once) are
// evaluated where the caller is (scalar_eval.h), or by the resident scalar kernel with WN_SCALAR_ON_DEVICE=1.
#include "WaveletNoise.h"

#include <algorithm>
#include <cmath>

#include "scalar_eval.h"
#include "wn_host.hpp"
#include "wnoise_advect.h"
#include "wnoise_bounded.h"
#include "wnoise_bounded2d.h"
#include "wnoise_curl2d.h"
#include "wnoise_footprint.h"
#include "wnoise_multiband2d.h"

using wnhost::check;

WaveletNoise::WaveletNoise(int tileSize, unsigned int seed)
    : tileSizeN(wn_tile_even_size(tileSize)), randomSeed(seed), rng(seed), gaussianDist(0.0f, 1.0f),
      tile_(nullptr)
{
    if (tileSizeN != tileSize) // WaveletNoise.cpp:22-25
        std::cerr << "Warning: Tile size adjusted to " << tileSizeN << " (must be even)" << std::endl;
}

WaveletNoise::~WaveletNoise() { wn_tile_destroy(tile_); }

void WaveletNoise::generate(int dims)
{
    const size_t n = static_cast<size_t>(tileSizeN);
    const size_t count = dims == 2 ? n * n : n * n * n;
    std::vector<float> field(count);
    for (size_t i = 0; i < count; ++i) field[i] = gaussianDist(rng); // WaveletNoise.cpp:74-77,146-147
    wn_tile *t = nullptr;
    check(wn_tile_generate_from_field(tileSizeN, dims, field.data(), &t), "wn_tile_generate_from_field");
    wn_tile_destroy(tile_);
    tile_ = t;
    noiseCoefficients.resize(count);
    check(wn_tile_download(tile_, noiseCoefficients.data()), "wn_tile_download");
    tileDims = dims;
}

void WaveletNoise::generateNoiseTile2D() { generate(2); }
void WaveletNoise::generateNoiseTile3D() { generate(3); }

const wn_tile *WaveletNoise::tile(int dims) const
{
    if (!tile_) check(wn_tile_create(0, dims, nullptr, &tile_), "wn_tile_create"); // empty: evaluates to 0
    return tile_;
}

// ---- scalar members: evaluated on the host from the mirrored coefficients (scalar_eval.h; the kernels' evaluators, csrc/wn_eval.hpp), or one
// request each to the resident scalar kernel (wn_scalar_*, include/wnoise.h) with WN_SCALAR_ON_DEVICE=1.  A tile of the other
// dimension goes to the C ABI either way, which reports it.
float WaveletNoise::evaluate2D(const float p[2]) const
{
    if (!wnhost_scalar_on_device() && tileDims != 3)
        return wnhost_eval2d(noiseCoefficients.empty() ? nullptr : noiseCoefficients.data(), tileSizeN, p);
    float v = 0.0f;
    check(wn_scalar_eval2d(tile(2), p, &v), "wn_scalar_eval2d");
    return v;
}

float WaveletNoise::evaluate3D(const float p[3]) const
{
    if (!wnhost_scalar_on_device() && tileDims != 2)
        return wnhost_eval3d(noiseCoefficients.empty() ? nullptr : noiseCoefficients.data(), tileSizeN, p);
    float v = 0.0f;
    check(wn_scalar_eval3d(tile(3), p, &v), "wn_scalar_eval3d");
    return v;
}

float WaveletNoise::evaluate3DProjected(const float p[3], const float normal[3]) const
{
    if (!wnhost_scalar_on_device() && tileDims != 2)
        return wnhost_eval3d_projected(noiseCoefficients.empty() ? nullptr : noiseCoefficients.data(), tileSizeN, p, normal);
    float v = 0.0f;
    check(wn_scalar_eval3d_projected(tile(3), p, normal, &v), "wn_scalar_eval3d_projected");
    return v;
}

float WaveletNoise::WMultibandNoise(const float p[3], float sarg, int firstBand, int nbands,
                                    const float *w, float variance) const
{
    auto &s = wnhost::Scratch::get();
    std::copy(p, p + 3, s.in_host());
    check(wn_multiband3d_points(tile(3), static_cast<const float *>(s.in_dev()), 1, sarg, firstBand,
                                nbands, w, variance, static_cast<float *>(s.out_dev()), nullptr),
          "wn_multiband3d_points");
    check(wn_stream_sync(nullptr), "wn_stream_sync");
    return s.out_host()[0];
}

float WaveletNoise::WMultibandNoise(const float p[3], float sarg, const float *normal, int firstBand,
                                    int nbands, const float *w, float variance) const
{
    if (!normal) return WMultibandNoise(p, sarg, firstBand, nbands, w, variance);
    auto &s = wnhost::Scratch::get();
    std::copy(p, p + 3, s.in_host());
    std::copy(normal, normal + 3, s.in_host() + 4);
    const float *in = static_cast<const float *>(s.in_dev());
    check(wn_multiband3d_projected_points(tile(3), in, in + 4, 1, 1, sarg, firstBand, nbands, w, variance,
                                          static_cast<float *>(s.out_dev()), nullptr),
          "wn_multiband3d_projected_points");
    check(wn_stream_sync(nullptr), "wn_stream_sync");
    return s.out_host()[0];
}

// ---- gradients: the scalar member on the host (bit-identical to the point kernel; WN_SCALAR_ON_DEVICE does not apply), the
// multiband one a batch of one on the device; a 2-D tile goes to the C ABI, which reports it
float WaveletNoise::evaluate3DGradient(const float p[3], float grad[3]) const
{
    if (tileDims != 2)
        return wnhost_eval3d_grad(noiseCoefficients.empty() ? nullptr : noiseCoefficients.data(), tileSizeN, p, grad);
    float out4[4];
    evaluate3DGradient(p, 1, out4);
    std::copy(out4 + 1, out4 + 4, grad);
    return out4[0];
}

float WaveletNoise::WMultibandNoiseGradient(const float p[3], float sarg, int firstBand, int nbands, const float *w,
                                            float grad[3], float variance) const
{
    auto &s = wnhost::Scratch::get();
    std::copy(p, p + 3, s.in_host());
    check(wn_multiband3d_grad_points(tile(3), static_cast<const float *>(s.in_dev()), 1, sarg, firstBand, nbands, w,
                                     variance, static_cast<float *>(s.out_dev()), nullptr),
          "wn_multiband3d_grad_points");
    check(wn_stream_sync(nullptr), "wn_stream_sync");
    std::copy(s.out_host() + 1, s.out_host() + 4, grad);
    return s.out_host()[0];
}

void WaveletNoise::evaluate3DGradient(const float *xyz, size_t n, float *out4) const
{
    if (!n) return;
    wnhost::DeviceBuffer in(3 * n * sizeof(float)), res(4 * n * sizeof(float));
    in.upload(xyz);
    check(wn_eval3d_grad_points(tile(3), in.as<float>(), n, res.as<float>(), nullptr), "wn_eval3d_grad_points");
    res.download(out4);
}

void WaveletNoise::WMultibandNoiseGradient(const float *xyz, size_t n, float sarg, int firstBand, int nbands,
                                           const float *w, float variance, float *out4) const
{
    if (!n) return;
    wnhost::DeviceBuffer in(3 * n * sizeof(float)), res(4 * n * sizeof(float));
    in.upload(xyz);
    check(wn_multiband3d_grad_points(tile(3), in.as<float>(), n, sarg, firstBand, nbands, w, variance, res.as<float>(),
                                     nullptr), "wn_multiband3d_grad_points");
    res.download(out4);
}

float WaveletNoise::evaluate2DGradient(const float p[2], float grad[2]) const
{
    if (tileDims != 3)
        return wnhost_eval2d_grad(noiseCoefficients.empty() ? nullptr : noiseCoefficients.data(), tileSizeN, p, grad);
    float out3[3];
    evaluate2DGradient(p, 1, out3);
    std::copy(out3 + 1, out3 + 3, grad);
    return out3[0];
}

float WaveletNoise::evaluate3DProjectedGradient(const float p[3], const float normal[3], float grad[3]) const
{
    if (tileDims != 2)
        return wnhost_eval3d_projected_grad(noiseCoefficients.empty() ? nullptr : noiseCoefficients.data(), tileSizeN, p,
                                            normal, grad);
    float out4[4];
    evaluate3DProjectedGradient(p, normal, 1, out4);
    std::copy(out4 + 1, out4 + 4, grad);
    return out4[0];
}

float WaveletNoise::WMultibandNoiseGradient(const float p[3], float sarg, const float *normal, int firstBand, int nbands,
                                            const float *w, float grad[3], float variance) const
{
    if (!normal) return WMultibandNoiseGradient(p, sarg, firstBand, nbands, w, grad, variance);
    auto &s = wnhost::Scratch::get();
    std::copy(p, p + 3, s.in_host());
    std::copy(normal, normal + 3, s.in_host() + 4);
    const float *in = static_cast<const float *>(s.in_dev());
    check(wn_multiband3d_projected_grad_points(tile(3), in, in + 4, 1, 1, sarg, firstBand, nbands, w, variance,
                                               static_cast<float *>(s.out_dev()), nullptr),
          "wn_multiband3d_projected_grad_points");
    check(wn_stream_sync(nullptr), "wn_stream_sync");
    std::copy(s.out_host() + 1, s.out_host() + 4, grad);
    return s.out_host()[0];
}

void WaveletNoise::evaluate2DGradient(const float *xy, size_t n, float *out3) const
{
    if (!n) return;
    wnhost::DeviceBuffer in(2 * n * sizeof(float)), res(3 * n * sizeof(float));
    in.upload(xy);
    check(wn_eval2d_grad_points(tile(2), in.as<float>(), n, res.as<float>(), nullptr), "wn_eval2d_grad_points");
    res.download(out3);
}

void WaveletNoise::evaluate3DProjectedGradient(const float *xyz, const float *normals, size_t n, float *out4) const
{
    if (!n) return;
    wnhost::DeviceBuffer in(3 * n * sizeof(float)), nr(3 * n * sizeof(float)), res(4 * n * sizeof(float));
    in.upload(xyz);
    nr.upload(normals);
    check(wn_eval3d_projected_grad_points(tile(3), in.as<float>(), nr.as<float>(), n, res.as<float>(), nullptr),
          "wn_eval3d_projected_grad_points");
    res.download(out4);
}

void WaveletNoise::WMultibandNoiseGradient(const float *xyz, const float *normals, bool oneNormal, size_t n, float sarg,
                                           int firstBand, int nbands, const float *w, float variance, float *out4) const
{
    if (!normals) return WMultibandNoiseGradient(xyz, n, sarg, firstBand, nbands, w, variance, out4);
    if (!n) return;
    const size_t nn = oneNormal ? 1 : n;
    wnhost::DeviceBuffer in(3 * n * sizeof(float)), nr(3 * nn * sizeof(float)), res(4 * n * sizeof(float));
    in.upload(xyz);
    nr.upload(normals);
    check(wn_multiband3d_projected_grad_points(tile(3), in.as<float>(), nr.as<float>(), oneNormal ? 1 : 0, n, sarg,
                                               firstBand, nbands, w, variance, res.as<float>(), nullptr),
          "wn_multiband3d_projected_grad_points");
    res.download(out4);
}

// ---- WMultibandNoise with a footprint per sample (include/wnoise_footprint.h): the scalar members on the host
// (bit-identical to the kernels), the batched ones on the device; a 2-D tile goes to the C ABI, which reports it
float WaveletNoise::WMultibandNoise(const float p[3], float sarg, bool fade, const float *normal, int firstBand, int nbands,
                                    const float *w, float variance) const
{
    if (tileDims != 2)
        return wnhost_multiband3d_footprint(noiseCoefficients.empty() ? nullptr : noiseCoefficients.data(), tileSizeN, p,
                                            normal, sarg, fade ? 1 : 0, firstBand, nbands, w, variance, nullptr);
    float out = 0.0f;
    WMultibandNoise(p, normal, true, 1, &sarg, fade, firstBand, nbands, w, variance, &out);
    return out;
}

float WaveletNoise::WMultibandNoiseGradient(const float p[3], float sarg, bool fade, const float *normal, int firstBand,
                                            int nbands, const float *w, float grad[3], float variance) const
{
    if (tileDims != 2)
        return wnhost_multiband3d_footprint(noiseCoefficients.empty() ? nullptr : noiseCoefficients.data(), tileSizeN, p,
                                            normal, sarg, fade ? 1 : 0, firstBand, nbands, w, variance, grad);
    float out4[4];
    WMultibandNoiseGradient(p, normal, true, 1, &sarg, fade, firstBand, nbands, w, variance, out4);
    std::copy(out4 + 1, out4 + 4, grad);
    return out4[0];
}

void WaveletNoise::WMultibandNoise(const float *xyz, const float *normals, bool oneNormal, size_t n, const float *sarg,
                                   bool fade, int firstBand, int nbands, const float *w, float variance, float *out) const
{
    if (!n) return;
    wnhost::DeviceBuffer in(3 * n * sizeof(float)), fp(n * sizeof(float)), res(n * sizeof(float));
    in.upload(xyz);
    fp.upload(sarg);
    if (!normals) {
        check(wn_multiband3d_footprint_points(tile(3), in.as<float>(), fp.as<float>(), n, firstBand, nbands, w, variance,
                                              fade ? 1 : 0, res.as<float>(), nullptr), "wn_multiband3d_footprint_points");
    } else {
        wnhost::DeviceBuffer nr(3 * (oneNormal ? 1 : n) * sizeof(float));
        nr.upload(normals);
        check(wn_multiband3d_projected_footprint_points(tile(3), in.as<float>(), nr.as<float>(), oneNormal ? 1 : 0,
                                                        fp.as<float>(), n, firstBand, nbands, w, variance, fade ? 1 : 0,
                                                        res.as<float>(), nullptr),
              "wn_multiband3d_projected_footprint_points");
    }
    res.download(out);
}

void WaveletNoise::WMultibandNoiseGradient(const float *xyz, const float *normals, bool oneNormal, size_t n,
                                           const float *sarg, bool fade, int firstBand, int nbands, const float *w,
                                           float variance, float *out4) const
{
    if (!n) return;
    wnhost::DeviceBuffer in(3 * n * sizeof(float)), fp(n * sizeof(float)), res(4 * n * sizeof(float));
    in.upload(xyz);
    fp.upload(sarg);
    if (!normals) {
        check(wn_multiband3d_footprint_grad_points(tile(3), in.as<float>(), fp.as<float>(), n, firstBand, nbands, w, variance,
                                                   fade ? 1 : 0, res.as<float>(), nullptr),
              "wn_multiband3d_footprint_grad_points");
    } else {
        wnhost::DeviceBuffer nr(3 * (oneNormal ? 1 : n) * sizeof(float));
        nr.upload(normals);
        check(wn_multiband3d_projected_footprint_grad_points(tile(3), in.as<float>(), nr.as<float>(), oneNormal ? 1 : 0,
                                                             fp.as<float>(), n, firstBand, nbands, w, variance,
                                                             fade ? 1 : 0, res.as<float>(), nullptr),
              "wn_multiband3d_projected_footprint_grad_points");
    }
    res.download(out4);
}

// ---- WMultibandNoise on the 2-D tile (include/wnoise_multiband2d.h): the one-sample members on the host (bit-identical to
// the kernels), the batched ones on the device; a 3-D tile goes to the C ABI, which reports it
float WaveletNoise::WMultibandNoise2D(const float p[2], float sarg, int firstBand, int nbands, const float *w, float variance,
                                      bool fade) const
{
    if (tileDims != 3)
        return wnhost_multiband2d_footprint(noiseCoefficients.empty() ? nullptr : noiseCoefficients.data(), tileSizeN, p, sarg,
                                            fade ? 1 : 0, firstBand, nbands, w, variance, nullptr);
    float out = 0.0f;
    WMultibandNoise2D(p, 1, &sarg, fade, firstBand, nbands, w, variance, &out);
    return out;
}

float WaveletNoise::WMultibandNoise2DGradient(const float p[2], float sarg, int firstBand, int nbands, const float *w,
                                              float grad[2], float variance, bool fade) const
{
    if (tileDims != 3)
        return wnhost_multiband2d_footprint(noiseCoefficients.empty() ? nullptr : noiseCoefficients.data(), tileSizeN, p, sarg,
                                            fade ? 1 : 0, firstBand, nbands, w, variance, grad);
    float out3[3];
    WMultibandNoise2DGradient(p, 1, &sarg, fade, firstBand, nbands, w, variance, out3);
    std::copy(out3 + 1, out3 + 3, grad);
    return out3[0];
}

void WaveletNoise::WMultibandNoise2D(const float *xy, size_t n, float sarg, int firstBand, int nbands, const float *w,
                                     float variance, float *out) const
{
    if (!n) return;
    wnhost::DeviceBuffer in(2 * n * sizeof(float)), res(n * sizeof(float));
    in.upload(xy);
    check(wn_multiband2d_points(tile(2), in.as<float>(), n, sarg, firstBand, nbands, w, variance, res.as<float>(), nullptr),
          "wn_multiband2d_points");
    res.download(out);
}

void WaveletNoise::WMultibandNoise2DGradient(const float *xy, size_t n, float sarg, int firstBand, int nbands, const float *w,
                                             float variance, float *out3) const
{
    if (!n) return;
    wnhost::DeviceBuffer in(2 * n * sizeof(float)), res(3 * n * sizeof(float));
    in.upload(xy);
    check(wn_multiband2d_grad_points(tile(2), in.as<float>(), n, sarg, firstBand, nbands, w, variance, res.as<float>(),
                                     nullptr), "wn_multiband2d_grad_points");
    res.download(out3);
}

void WaveletNoise::WMultibandNoise2D(const float *xy, size_t n, const float *sarg, bool fade, int firstBand, int nbands,
                                     const float *w, float variance, float *out) const
{
    if (!n) return;
    wnhost::DeviceBuffer in(2 * n * sizeof(float)), fp(n * sizeof(float)), res(n * sizeof(float));
    in.upload(xy);
    fp.upload(sarg);
    check(wn_multiband2d_footprint_points(tile(2), in.as<float>(), fp.as<float>(), n, firstBand, nbands, w, variance,
                                          fade ? 1 : 0, res.as<float>(), nullptr), "wn_multiband2d_footprint_points");
    res.download(out);
}

void WaveletNoise::WMultibandNoise2DGradient(const float *xy, size_t n, const float *sarg, bool fade, int firstBand,
                                             int nbands, const float *w, float variance, float *out3) const
{
    if (!n) return;
    wnhost::DeviceBuffer in(2 * n * sizeof(float)), fp(n * sizeof(float)), res(3 * n * sizeof(float));
    in.upload(xy);
    fp.upload(sarg);
    check(wn_multiband2d_footprint_grad_points(tile(2), in.as<float>(), fp.as<float>(), n, firstBand, nbands, w, variance,
                                               fade ? 1 : 0, res.as<float>(), nullptr),
          "wn_multiband2d_footprint_grad_points");
    res.download(out3);
}

// ---- curl noise: the scalar member on the host (bit-identical to the point kernel), the multiband one a batch of one on
// the device; a 2-D tile goes to the C ABI, which reports it
void WaveletNoise::defaultCurlOffsets(int offsets9[9]) const
{
    for (int k = 0; k < 3; ++k) offsets9[3 * k] = offsets9[3 * k + 1] = offsets9[3 * k + 2] = k * tileSizeN / 3;
}

void WaveletNoise::evaluate3DCurl(const float p[3], const int *offsets9, float v[3]) const
{
    if (tileDims == 2) return evaluate3DCurl(p, 1, offsets9, v);
    int def[9];
    if (!offsets9) defaultCurlOffsets(def);
    wnhost_eval3d_curl(noiseCoefficients.empty() ? nullptr : noiseCoefficients.data(), tileSizeN, p,
                       offsets9 ? offsets9 : def, v);
}

void WaveletNoise::evaluate3DCurl(const float *xyz, size_t n, const int *offsets9, float *out3) const
{
    if (!n) return;
    int def[9];
    if (!offsets9) defaultCurlOffsets(def);
    wnhost::DeviceBuffer in(3 * n * sizeof(float)), res(3 * n * sizeof(float));
    in.upload(xyz);
    check(wn_eval3d_curl_points(tile(3), in.as<float>(), n, offsets9 ? offsets9 : def, res.as<float>(), nullptr),
          "wn_eval3d_curl_points");
    res.download(out3);
}

void WaveletNoise::WMultibandNoiseCurl(const float p[3], const int *offsets9, float sarg, int firstBand, int nbands,
                                       const float *w, float v[3], float variance) const
{
    int def[9];
    if (!offsets9) defaultCurlOffsets(def);
    auto &s = wnhost::Scratch::get();
    std::copy(p, p + 3, s.in_host());
    check(wn_multiband3d_curl_points(tile(3), static_cast<const float *>(s.in_dev()), 1, offsets9 ? offsets9 : def, sarg,
                                     firstBand, nbands, w, variance, static_cast<float *>(s.out_dev()), nullptr),
          "wn_multiband3d_curl_points");
    check(wn_stream_sync(nullptr), "wn_stream_sync");
    std::copy(s.out_host(), s.out_host() + 3, v);
}

void WaveletNoise::WMultibandNoiseCurl(const float *xyz, size_t n, const int *offsets9, float sarg, int firstBand,
                                       int nbands, const float *w, float variance, float *out3) const
{
    if (!n) return;
    int def[9];
    if (!offsets9) defaultCurlOffsets(def);
    wnhost::DeviceBuffer in(3 * n * sizeof(float)), res(3 * n * sizeof(float));
    in.upload(xyz);
    check(wn_multiband3d_curl_points(tile(3), in.as<float>(), n, offsets9 ? offsets9 : def, sarg, firstBand, nbands, w,
                                     variance, res.as<float>(), nullptr), "wn_multiband3d_curl_points");
    res.download(out3);
}

// ---- particles through the curl field: the scalar member traced on the host (bit-identical to the kernel), the batched ones
// one call of the C ABI, which checks `a`; the trajectory buffer exists only when a.traj_every asks for it
namespace {

// D: floats per particle; Adv: wn_advect (D = 3) or wn_advect2d (D = 2)
template <int D = 3, typename Adv, typename Call>
void advect_batch(const float *pts, size_t n, const Adv &a, float *pts_out, float *traj, Call call, const char *what)
{
    if (!n) return;
    const bool snaps = a.traj_every >= 1 && a.steps >= 0 && traj;
    const size_t traj_bytes = snaps ? ((size_t)(a.steps / a.traj_every) + 1) * D * n * sizeof(float) : 0;
    wnhost::DeviceBuffer pos(D * n * sizeof(float)), path(traj_bytes ? traj_bytes : sizeof(float));
    pos.upload(pts);
    check(call(pos.as<float>(), snaps ? path.as<float>() : nullptr), what); // in place on the device
    if (snaps) check(wn_copy_d2h(traj, path.get(), traj_bytes, nullptr), "wn_copy_d2h");
    pos.download(pts_out);
}

} // namespace

void WaveletNoise::advectCurl(const float p[3], const wn_advect &a, const int *offsets9, float p_out[3], float *traj) const
{
    if (tileDims == 2) return advectCurl(p, 1, a, offsets9, p_out, traj);
    int def[9];
    if (!offsets9) defaultCurlOffsets(def);
    if (wnhost_eval3d_curl_advect(noiseCoefficients.empty() ? nullptr : noiseCoefficients.data(), tileSizeN, p,
                                  offsets9 ? offsets9 : def, &a, p_out, traj))
        throw std::runtime_error("advectCurl: a method outside 0..2, negative steps or traj_every, a non-finite h, gain or "
                                 "drift, or a trajectory without a buffer");
}

void WaveletNoise::advectCurl(const float *xyz, size_t n, const wn_advect &a, const int *offsets9, float *xyz_out,
                              float *traj) const
{
    int def[9];
    if (!offsets9) defaultCurlOffsets(def);
    advect_batch(xyz, n, a, xyz_out, traj, [&](float *pos, float *path) {
        return wn_eval3d_curl_advect_points(tile(3), pos, n, offsets9 ? offsets9 : def, &a, pos, path, nullptr);
    }, "wn_eval3d_curl_advect_points");
}

void WaveletNoise::WMultibandNoiseAdvectCurl(const float p[3], const wn_advect &a, const int *offsets9, float sarg,
                                             int firstBand, int nbands, const float *w, float p_out[3], float *traj,
                                             float variance) const
{
    WMultibandNoiseAdvectCurl(p, 1, a, offsets9, sarg, firstBand, nbands, w, variance, p_out, traj);
}

void WaveletNoise::WMultibandNoiseAdvectCurl(const float *xyz, size_t n, const wn_advect &a, const int *offsets9, float sarg,
                                             int firstBand, int nbands, const float *w, float variance, float *xyz_out,
                                             float *traj) const
{
    int def[9];
    if (!offsets9) defaultCurlOffsets(def);
    advect_batch(xyz, n, a, xyz_out, traj, [&](float *pos, float *path) {
        return wn_multiband3d_curl_advect_points(tile(3), pos, n, offsets9 ? offsets9 : def, sarg, firstBand, nbands, w,
                                                 variance, &a, pos, path, nullptr);
    }, "wn_multiband3d_curl_advect_points");
}

// ---- the curl field with solid boundaries (include/wnoise_bounded.h): as the eight members above, the obstacle list beside
// the offsets
void WaveletNoise::evaluate3DCurlBounded(const float p[3], const int *offsets9, const wn_obstacle *obs, int nobs,
                                         float v[3]) const
{
    if (tileDims == 2) return evaluate3DCurlBounded(p, 1, offsets9, obs, nobs, v);
    int def[9];
    if (!offsets9) defaultCurlOffsets(def);
    if (wnhost_eval3d_curl_bounded(noiseCoefficients.empty() ? nullptr : noiseCoefficients.data(), tileSizeN, p,
                                   offsets9 ? offsets9 : def, obs, nobs, v))
        throw std::runtime_error("evaluate3DCurlBounded: an obstacle list that wn_eval3d_curl_bounded_points refuses");
}

void WaveletNoise::evaluate3DCurlBounded(const float *xyz, size_t n, const int *offsets9, const wn_obstacle *obs, int nobs,
                                         float *out3) const
{
    if (!n) return;
    int def[9];
    if (!offsets9) defaultCurlOffsets(def);
    wnhost::DeviceBuffer in(3 * n * sizeof(float)), res(3 * n * sizeof(float));
    in.upload(xyz);
    check(wn_eval3d_curl_bounded_points(tile(3), in.as<float>(), n, offsets9 ? offsets9 : def, obs, nobs, res.as<float>(),
                                        nullptr), "wn_eval3d_curl_bounded_points");
    res.download(out3);
}

void WaveletNoise::WMultibandNoiseCurlBounded(const float p[3], const int *offsets9, const wn_obstacle *obs, int nobs,
                                              float sarg, int firstBand, int nbands, const float *w, float v[3],
                                              float variance) const
{
    WMultibandNoiseCurlBounded(p, 1, offsets9, obs, nobs, sarg, firstBand, nbands, w, variance, v);
}

void WaveletNoise::WMultibandNoiseCurlBounded(const float *xyz, size_t n, const int *offsets9, const wn_obstacle *obs, int nobs,
                                              float sarg, int firstBand, int nbands, const float *w, float variance,
                                              float *out3) const
{
    if (!n) return;
    int def[9];
    if (!offsets9) defaultCurlOffsets(def);
    wnhost::DeviceBuffer in(3 * n * sizeof(float)), res(3 * n * sizeof(float));
    in.upload(xyz);
    check(wn_multiband3d_curl_bounded_points(tile(3), in.as<float>(), n, offsets9 ? offsets9 : def, sarg, firstBand, nbands, w,
                                             variance, obs, nobs, res.as<float>(), nullptr),
          "wn_multiband3d_curl_bounded_points");
    res.download(out3);
}

void WaveletNoise::advectCurlBounded(const float p[3], const wn_advect &a, const int *offsets9, const wn_obstacle *obs,
                                     int nobs, float p_out[3], float *traj) const
{
    if (tileDims == 2) return advectCurlBounded(p, 1, a, offsets9, obs, nobs, p_out, traj);
    int def[9];
    if (!offsets9) defaultCurlOffsets(def);
    if (wnhost_eval3d_curl_bounded_advect(noiseCoefficients.empty() ? nullptr : noiseCoefficients.data(), tileSizeN, p,
                                          offsets9 ? offsets9 : def, obs, nobs, &a, p_out, traj))
        throw std::runtime_error("advectCurlBounded: an obstacle list or a wn_advect that "
                                 "wn_eval3d_curl_bounded_advect_points refuses, or a trajectory without a buffer");
}

void WaveletNoise::advectCurlBounded(const float *xyz, size_t n, const wn_advect &a, const int *offsets9,
                                     const wn_obstacle *obs, int nobs, float *xyz_out, float *traj) const
{
    int def[9];
    if (!offsets9) defaultCurlOffsets(def);
    advect_batch(xyz, n, a, xyz_out, traj, [&](float *pos, float *path) {
        return wn_eval3d_curl_bounded_advect_points(tile(3), pos, n, offsets9 ? offsets9 : def, obs, nobs, &a, pos, path,
                                                    nullptr);
    }, "wn_eval3d_curl_bounded_advect_points");
}

void WaveletNoise::WMultibandNoiseAdvectCurlBounded(const float p[3], const wn_advect &a, const int *offsets9,
                                                    const wn_obstacle *obs, int nobs, float sarg, int firstBand, int nbands,
                                                    const float *w, float p_out[3], float *traj, float variance) const
{
    WMultibandNoiseAdvectCurlBounded(p, 1, a, offsets9, obs, nobs, sarg, firstBand, nbands, w, variance, p_out, traj);
}

void WaveletNoise::WMultibandNoiseAdvectCurlBounded(const float *xyz, size_t n, const wn_advect &a, const int *offsets9,
                                                    const wn_obstacle *obs, int nobs, float sarg, int firstBand, int nbands,
                                                    const float *w, float variance, float *xyz_out, float *traj) const
{
    int def[9];
    if (!offsets9) defaultCurlOffsets(def);
    advect_batch(xyz, n, a, xyz_out, traj, [&](float *pos, float *path) {
        return wn_multiband3d_curl_bounded_advect_points(tile(3), pos, n, offsets9 ? offsets9 : def, sarg, firstBand, nbands,
                                                         w, variance, obs, nobs, &a, pos, path, nullptr);
    }, "wn_multiband3d_curl_bounded_advect_points");
}

// ---- curl noise on the 2-D tile and particles through it (include/wnoise_curl2d.h): the one-sample members on the host
// (bit-identical to the kernels), the batched ones on the device; a 3-D tile goes to the C ABI, which reports it
void WaveletNoise::WMultibandNoise2DCurl(const float p[2], float sarg, int firstBand, int nbands, const float *w, float v[2],
                                         float variance) const
{
    if (tileDims == 3) return WMultibandNoise2DCurl(p, 1, sarg, firstBand, nbands, w, variance, v);
    wnhost_multiband2d_curl(noiseCoefficients.empty() ? nullptr : noiseCoefficients.data(), tileSizeN, p, sarg, firstBand,
                            nbands, w, variance, v);
}

void WaveletNoise::WMultibandNoise2DCurl(const float *xy, size_t n, float sarg, int firstBand, int nbands, const float *w,
                                         float variance, float *out2) const
{
    if (!n) return;
    wnhost::DeviceBuffer in(2 * n * sizeof(float)), res(2 * n * sizeof(float));
    in.upload(xy);
    check(wn_multiband2d_curl_points(tile(2), in.as<float>(), n, sarg, firstBand, nbands, w, variance, res.as<float>(),
                                     nullptr), "wn_multiband2d_curl_points");
    res.download(out2);
}

void WaveletNoise::WMultibandNoise2DAdvectCurl(const float p[2], const wn_advect2d &a, float sarg, int firstBand, int nbands,
                                               const float *w, float p_out[2], float *traj, float variance) const
{
    if (tileDims == 3) return WMultibandNoise2DAdvectCurl(p, 1, a, sarg, firstBand, nbands, w, variance, p_out, traj);
    if (wnhost_multiband2d_curl_advect(noiseCoefficients.empty() ? nullptr : noiseCoefficients.data(), tileSizeN, p, sarg,
                                       firstBand, nbands, w, variance, &a, p_out, traj))
        throw std::runtime_error("WMultibandNoise2DAdvectCurl: nbands outside 0..8, a method outside 0..2, negative steps or "
                                 "traj_every, a non-finite h, gain or drift, or a trajectory without a buffer");
}

void WaveletNoise::WMultibandNoise2DAdvectCurl(const float *xy, size_t n, const wn_advect2d &a, float sarg, int firstBand,
                                               int nbands, const float *w, float variance, float *xy_out, float *traj) const
{
    advect_batch<2>(xy, n, a, xy_out, traj, [&](float *pos, float *path) {
        return wn_multiband2d_curl_advect_points(tile(2), pos, n, sarg, firstBand, nbands, w, variance, &a, pos, path, nullptr);
    }, "wn_multiband2d_curl_advect_points");
}

// ---- that field with solid boundaries and a background stream (include/wnoise_bounded2d.h): as the four members above, the
// obstacle list and the stream beside the bands
void WaveletNoise::WMultibandNoise2DCurlBounded(const float p[2], const wn_obstacle2d *obs, int nobs, const float *flow,
                                                float sarg, int firstBand, int nbands, const float *w, float v[2],
                                                float variance) const
{
    if (tileDims == 3) return WMultibandNoise2DCurlBounded(p, 1, obs, nobs, flow, sarg, firstBand, nbands, w, variance, v);
    if (wnhost_multiband2d_curl_bounded(noiseCoefficients.empty() ? nullptr : noiseCoefficients.data(), tileSizeN, p, sarg,
                                        firstBand, nbands, w, variance, obs, nobs, flow, v))
        throw std::runtime_error("WMultibandNoise2DCurlBounded: nbands outside 0..8, or an obstacle list or a stream that "
                                 "wn_multiband2d_curl_bounded_points refuses");
}

void WaveletNoise::WMultibandNoise2DCurlBounded(const float *xy, size_t n, const wn_obstacle2d *obs, int nobs,
                                                const float *flow, float sarg, int firstBand, int nbands, const float *w,
                                                float variance, float *out2) const
{
    if (!n) return;
    wnhost::DeviceBuffer in(2 * n * sizeof(float)), res(2 * n * sizeof(float));
    in.upload(xy);
    check(wn_multiband2d_curl_bounded_points(tile(2), in.as<float>(), n, sarg, firstBand, nbands, w, variance, obs, nobs, flow,
                                             res.as<float>(), nullptr), "wn_multiband2d_curl_bounded_points");
    res.download(out2);
}

void WaveletNoise::WMultibandNoise2DAdvectCurlBounded(const float p[2], const wn_advect2d &a, const wn_obstacle2d *obs,
                                                      int nobs, const float *flow, float sarg, int firstBand, int nbands,
                                                      const float *w, float p_out[2], float *traj, float variance) const
{
    if (tileDims == 3)
        return WMultibandNoise2DAdvectCurlBounded(p, 1, a, obs, nobs, flow, sarg, firstBand, nbands, w, variance, p_out, traj);
    if (wnhost_multiband2d_curl_bounded_advect(noiseCoefficients.empty() ? nullptr : noiseCoefficients.data(), tileSizeN, p,
                                               sarg, firstBand, nbands, w, variance, obs, nobs, flow, &a, p_out, traj))
        throw std::runtime_error("WMultibandNoise2DAdvectCurlBounded: nbands outside 0..8, or an obstacle list, a stream or a "
                                 "wn_advect2d that wn_multiband2d_curl_bounded_advect_points refuses");
}

void WaveletNoise::WMultibandNoise2DAdvectCurlBounded(const float *xy, size_t n, const wn_advect2d &a, const wn_obstacle2d *obs,
                                                      int nobs, const float *flow, float sarg, int firstBand, int nbands,
                                                      const float *w, float variance, float *xy_out, float *traj) const
{
    advect_batch<2>(xy, n, a, xy_out, traj, [&](float *pos, float *path) {
        return wn_multiband2d_curl_bounded_advect_points(tile(2), pos, n, sarg, firstBand, nbands, w, variance, obs, nobs, flow,
                                                         &a, pos, path, nullptr);
    }, "wn_multiband2d_curl_bounded_advect_points");
}

// ---- batched members ----------------------------------------------------------------------------------
void WaveletNoise::evaluate2D(const float *xy, size_t n, float *out) const
{
    if (!n) return;
    wnhost::DeviceBuffer in(2 * n * sizeof(float)), res(n * sizeof(float));
    in.upload(xy);
    check(wn_eval2d_points(tile(2), in.as<float>(), n, res.as<float>(), nullptr), "wn_eval2d_points");
    res.download(out);
}

void WaveletNoise::evaluate3D(const float *xyz, size_t n, float *out) const
{
    if (!n) return;
    wnhost::DeviceBuffer in(3 * n * sizeof(float)), res(n * sizeof(float));
    in.upload(xyz);
    check(wn_eval3d_points(tile(3), in.as<float>(), n, res.as<float>(), nullptr), "wn_eval3d_points");
    res.download(out);
}

void WaveletNoise::evaluate3DProjected(const float *xyz, const float *normals, size_t n, float *out) const
{
    if (!n) return;
    wnhost::DeviceBuffer in(3 * n * sizeof(float)), nr(3 * n * sizeof(float)), res(n * sizeof(float));
    in.upload(xyz);
    nr.upload(normals);
    check(wn_eval3d_projected_points(tile(3), in.as<float>(), nr.as<float>(), n, res.as<float>(), nullptr),
          "wn_eval3d_projected_points");
    res.download(out);
}

void WaveletNoise::WMultibandNoise(const float *xyz, size_t n, float sarg, int firstBand, int nbands,
                                   const float *w, float variance, float *out) const
{
    if (!n) return;
    wnhost::DeviceBuffer in(3 * n * sizeof(float)), res(n * sizeof(float));
    in.upload(xyz);
    check(wn_multiband3d_points(tile(3), in.as<float>(), n, sarg, firstBand, nbands, w, variance,
                                res.as<float>(), nullptr), "wn_multiband3d_points");
    res.download(out);
}

// ---- debug helper (WaveletNoise.cpp:268-288; no caller in the reference; host-side statistics) --------
DataStats WaveletNoise::calculateStats(const std::vector<float> &data, const std::string &name) const
{
    DataStats stats;
    if (data.empty()) return stats;
    double total = 0.0, total_sq = 0.0;
    for (float v : data) {
        total += v;
        total_sq += static_cast<double>(v) * v;
        stats.min_val = std::min(stats.min_val, v);
        stats.max_val = std::max(stats.max_val, v);
    }
    stats.avg = static_cast<float>(total / data.size());
    stats.var = static_cast<float>(total_sq / data.size() - static_cast<double>(stats.avg) * stats.avg);
    std::cout << name << " stats: avg=" << stats.avg << ", var=" << stats.var
              << ", stddev=" << std::sqrt(stats.var) << std::endl;
    return stats;
}

const std::vector<float> &WaveletNoise::getNoiseCoefficients() const { return noiseCoefficients; }
int WaveletNoise::getTileSize() const { return tileSizeN; }
