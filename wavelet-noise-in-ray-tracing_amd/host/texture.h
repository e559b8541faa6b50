// texture.h -- the reference's texture adaptor (texture.h:14-115) over the MI355X C ABI.
//
// Same class names, constructors and `value(u, v, p)` signature, so material.h / main.cpp of the
// reference compile against this header unchanged.  value() is one sample, evaluated on the host (scalar_eval.h;
// WN_SCALAR_ON_DEVICE=1: one request to the resident scalar kernel, ~2.6 us) and returns the reference's colour bit for
// bit; values() is the batched GPU form a renderer should use (hit points in, grey levels out, optional per-hit `active`
// bytes compacted with wavefront ballots on the device).
#ifndef TEXTURE_H
#define TEXTURE_H

#include <cstddef>
#include <cstdint>
#include <limits>
#include <memory>
#include <vector>

#include "WaveletNoise.h"
#include "perlin.h"
#include "scalar_eval.h"
#include "vec3.h"
#include "wn_host.hpp"
#include "wnoise_footprint.h"
#include "wnoise_perlin_footprint.h"

using color = vec3;
using point3 = vec3;

class texture {
  public:
    virtual ~texture() = default;
    virtual color value(double u, double v, const point3 &p) const = 0;
};

class solid_color : public texture {
  public:
    solid_color(const color &albedo) : albedo(albedo) {}
    solid_color(double red, double green, double blue) : solid_color(color(red, green, blue)) {}
    color value(double, double, const point3 &) const override { return albedo; }

  private:
    color albedo;
};

namespace wnhost {
// grey levels for n host points through a device round trip
template <typename Launch> inline void texture_batch(const float *xyz, const uint8_t *active, size_t n,
                                                     float *grey, Launch launch)
{
    if (!n) return;
    DeviceBuffer in(3 * n * sizeof(float)), out(n * sizeof(float));
    in.upload(xyz);
    out.upload(grey); // inactive points keep the caller's value
    if (active) {
        DeviceBuffer act(n);
        act.upload(active);
        launch(in.as<float>(), act.as<uint8_t>(), out.as<float>());
        out.download(grey);
    } else {
        launch(in.as<float>(), static_cast<const uint8_t *>(nullptr), out.as<float>());
        out.download(grey);
    }
}
} // namespace wnhost

class noise_texture : public texture {
  public:
    noise_texture(double scale, int octave = 4) : scale(scale), octave_level(octave) {}

    color value(double, double, const point3 &p) const override // texture.h:37-43
    {
        const float xyz[3] = {p.x(), p.y(), p.z()};
        float g = 0.0f;
        if (!wnhost_scalar_on_device()) { // one sample: on the host (scalar_eval.h)
            g = wnhost_noise_texture_value(noise.table().data(), scale, octave_level, xyz);
            return color(g, g, g);
        }
        // WN_SCALAR_ON_DEVICE=1: one request to the resident scalar kernel (include/wnoise.h, wn_scalar_*)
        wnhost::check(wn_scalar_noise_texture(noise.perm(), scale, octave_level, xyz, &g), "wn_scalar_noise_texture");
        return color(g, g, g);
    }
    // additive: batched grey levels (host pointers); active == nullptr means every point
    void values(const float *xyz, const uint8_t *active, size_t n, float *grey) const
    {
        wnhost::texture_batch(xyz, active, n, grey, [&](const float *in, const uint8_t *act, float *out) {
            wnhost::check(wn_noise_texture_points(noise.perm(), scale, octave_level, in, act, n, out, nullptr),
                          "wn_noise_texture_points");
        });
    }
    // additive: device pointers, enqueue only (default stream)
    void values_device(const float *xyz_dev, size_t n, float *grey_dev) const
    {
        wnhost::check(wn_noise_texture_points(noise.perm(), scale, octave_level, xyz_dev, nullptr, n, grey_dev, nullptr),
                      "wn_noise_texture_points");
    }

  private:
    perlin noise; // default seed, texture.h:46
    double scale;
    int octave_level;
};

class wavelet_texture : public texture {
  public:
    wavelet_texture(double scale = 1.0, int octave = 4, bool use_3d = true)
        : scale(scale), octave_level(octave), use_3d_noise(use_3d)
    {
        const int TILE_SIZE = 128;        // texture.h:55
        const unsigned int SEED = 12345;  // texture.h:56
        noise_2d = std::make_unique<WaveletNoise>(TILE_SIZE, SEED);
        noise_2d->generateNoiseTile2D();
        if (use_3d_noise) {
            noise_3d = std::make_unique<WaveletNoise>(TILE_SIZE, SEED);
            noise_3d->generateNoiseTile3D();
        }
    }

    color value(double, double, const point3 &p) const override // texture.h:67-107
    {
        const float xyz[3] = {p.x(), p.y(), p.z()};
        const bool three = use_3d_noise && noise_3d;
        float g = 0.0f;
        if (!wnhost_scalar_on_device()) { // one sample: on the host (scalar_eval.h)
            const WaveletNoise *src = three ? noise_3d.get() : noise_2d.get();
            const std::vector<float> *c = src ? &src->getNoiseCoefficients() : nullptr;
            g = wnhost_wavelet_texture_value(c && !c->empty() ? c->data() : nullptr, src ? src->getTileSize() : 0, three ? 1 : 0,
                                             scale, octave_level, xyz);
            return color(g, g, g);
        }
        wnhost::check(wn_scalar_wavelet_texture(source(three), three ? 1 : 0, scale, octave_level, xyz, &g),
                      "wn_scalar_wavelet_texture");
        return color(g, g, g);
    }
    void values(const float *xyz, const uint8_t *active, size_t n, float *grey) const
    {
        const bool three = use_3d_noise && noise_3d;
        wnhost::texture_batch(xyz, active, n, grey, [&](const float *in, const uint8_t *act, float *out) {
            wnhost::check(wn_wavelet_texture_points(source(three), three ? 1 : 0, scale, octave_level, in,
                                                    act, n, out, nullptr), "wn_wavelet_texture_points");
        });
    }
    // additive: device pointers, enqueue only (default stream)
    void values_device(const float *xyz_dev, size_t n, float *grey_dev) const
    {
        const bool three = use_3d_noise && noise_3d;
        wnhost::check(wn_wavelet_texture_points(source(three), three ? 1 : 0, scale, octave_level, xyz_dev, nullptr, n,
                                                grey_dev, nullptr), "wn_wavelet_texture_points");
    }

  private:
    const wn_tile *source(bool three) const { return three ? noise_3d->tile(3) : noise_2d->tile(2); }
    std::unique_ptr<WaveletNoise> noise_2d;
    std::unique_ptr<WaveletNoise> noise_3d;
    double scale;
    int octave_level;
    bool use_3d_noise;
};

// WMultibandNoise as a texture, band-limited by each hit's footprint (absent from the reference; Cook & DeRose Appendix 2,
// include/wnoise_footprint.h): pos = (float)(p * scale) per axis, n = WMultibandNoise(pos, s, NULL, firstBand, nbands, w)
// normalised with `variance`, grey = 0.5 * (1 + clamp(n / 4, -1, 1)) as wavelet_texture.  s is the log2 of the hit's
// footprint in noise space (after scale); band b runs while (s + firstBand) + b < 0, and with `fade` the finest surviving
// band fades in over one octave.  value() is one sample on the host at the default footprint (-infinity: all bands, until
// set_default_footprint); grey() is the batched GPU form with one footprint per hit.
class wavelet_multiband_texture : public texture {
  public:
    wavelet_multiband_texture(double scale, int firstBand, int nbands, const float *w, float variance = 0.18402f,
                              bool fade = true)
        : scale(scale), first_band(firstBand), nbands(nbands), weights(w, w + (nbands > 0 ? nbands : 0)),
          variance(variance), fade(fade)
    {
        noise_3d = std::make_unique<WaveletNoise>(128, 12345); // wavelet_texture's tile (texture.h:55-56)
        noise_3d->generateNoiseTile3D();
    }

    void set_default_footprint(float s) { default_s = s; }
    float default_footprint() const { return default_s; }

    color value(double, double, const point3 &p) const override
    {
        const float xyz[3] = {p.x(), p.y(), p.z()};
        const std::vector<float> &c = noise_3d->getNoiseCoefficients();
        const float g = wnhost_wavelet_multiband_texture_value(c.empty() ? nullptr : c.data(), noise_3d->getTileSize(), scale,
                                                               first_band, nbands, weights.data(), variance, fade ? 1 : 0,
                                                               xyz, default_s);
        return color(g, g, g);
    }
    // batched grey levels (host pointers): one footprint per hit; active == nullptr means every point, else inactive
    // points keep the caller's value
    void grey(const float *xyz, const float *s, const uint8_t *active, size_t n, float *out) const
    {
        if (!n) return;
        wnhost::DeviceBuffer fp(n * sizeof(float));
        fp.upload(s);
        wnhost::texture_batch(xyz, active, n, out, [&](const float *in, const uint8_t *act, float *res) {
            wnhost::check(wn_wavelet_multiband_texture_points(noise_3d->tile(3), scale, first_band, nbands, weights.data(),
                                                              variance, fade ? 1 : 0, in, fp.as<float>(), act, n, res,
                                                              nullptr), "wn_wavelet_multiband_texture_points");
        });
    }

  private:
    std::unique_ptr<WaveletNoise> noise_3d;
    double scale;
    int first_band, nbands;
    std::vector<float> weights;
    float variance;
    bool fade;
    float default_s = -std::numeric_limits<float>::infinity();
};

// fractal_noise as a texture, octave-limited by each hit's footprint (absent from the reference;
// include/wnoise_perlin_footprint.h): the band-limited Perlin twin of wavelet_multiband_texture.  pos = (float)scale * p per
// axis in float (noise_texture's scaling without its octave factor), n = fractal_noise over `octaves` octaves of which
// octave i runs while (s + bias) + i < 0, grey = 0.5 * (1 + n).  s is the log2 of the hit's footprint in noise space (after
// scale); with `fade` the finest surviving octave fades in over one octave.  value() is one sample on the host at the
// default footprint (-infinity: all octaves, until set_default_footprint); grey() is the batched GPU form with one
// footprint per hit.
class noise_multiband_texture : public texture {
  public:
    noise_multiband_texture(double scale, int octaves = 6, float bias = 0.0f, bool fade = true)
        : scale(scale), octaves(octaves), bias(bias), fade(fade)
    {
    }

    void set_default_footprint(float s) { default_s = s; }
    float default_footprint() const { return default_s; }

    color value(double, double, const point3 &p) const override
    {
        const float xyz[3] = {p.x(), p.y(), p.z()};
        const float g = wnhost_noise_multiband_texture_value(noise.table().data(), scale, octaves, bias, fade ? 1 : 0, xyz, default_s);
        return color(g, g, g);
    }
    // batched grey levels (host pointers): one footprint per hit; active == nullptr means every point, else inactive
    // points keep the caller's value
    void grey(const float *xyz, const float *s, const uint8_t *active, size_t n, float *out) const
    {
        if (!n) return;
        wnhost::DeviceBuffer fp(n * sizeof(float));
        fp.upload(s);
        wnhost::texture_batch(xyz, active, n, out, [&](const float *in, const uint8_t *act, float *res) {
            wnhost::check(wn_noise_multiband_texture_points(noise.perm(), scale, octaves, bias, fade ? 1 : 0, in, fp.as<float>(),
                                                            act, n, res, nullptr), "wn_noise_multiband_texture_points");
        });
    }

  private:
    perlin noise; // default seed, as noise_texture
    double scale;
    int octaves;
    float bias;
    bool fade;
    float default_s = -std::numeric_limits<float>::infinity();
};

#endif
