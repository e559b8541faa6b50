// noise_grid.h -- the five dense-grid generators of the reference's experient/main.cpp (:11-129),
// same names and argument order, as single batched launches through the C ABI instead of 65,536
// scalar calls each.  Output files are the reference's raw format: float32[imageSize*imageSize],
// row-major, index y*imageSize+x (experient/main.cpp:28,32-34).
#pragma once

#include <cmath>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "PerlinNoise.hpp"
#include "WaveletNoise.h"
#include "wn_host.hpp"
#include "wnoise_bounded_bricks.h"
#include "wnoise_brick_fields.h"
#include "wnoise_bricks.h"
#include "wnoise_multiband2d.h"
#include "wnoise_perlin_bounded_bricks.h"
#include "wnoise_perlin_bricks.h"

namespace wnhost {

inline wn_grid lattice2d(int imageSize, int octave, float post_scale, float out_scale, int flags)
{
    wn_grid g{};
    g.den = g.nx = g.ny = imageSize;
    g.z0 = 0;
    g.z1 = 1;
    g.base_range = 4.0f;                          // experient/main.cpp:13
    g.octave_scale = std::pow(2.0f, octave);      // :14
    g.post_scale = post_scale;
    g.z_mode = WN_Z_LATTICE;
    g.z_const = 0.0f;
    g.out_scale = out_scale;
    g.flags = flags;
    return g;
}

template <typename Launch>
inline void run_grid(int imageSize, const std::string &outputFile, Launch launch)
{
    const size_t count = static_cast<size_t>(imageSize) * imageSize;
    std::vector<float> image(count);
    if (count) {
        DeviceBuffer out(count * sizeof(float));
        launch(out.as<float>());
        out.download(image.data());
    }
    std::ofstream outFile(outputFile, std::ios::binary);
    outFile.write(reinterpret_cast<const char *>(image.data()), image.size() * sizeof(float));
}

} // namespace wnhost

// The reference-named generators reproduce the reference's files byte for byte: they ask for
// WN_GRID_EXACT.  (3-D sliced only: pass WN_GRID_DEFAULT to opt in to the separable brick kernel,
// within 1e-5 of the reference -- a single 256x256 plane gains nothing measurable from it.)
inline void generate2DOctaveBandNoise(int imageSize, int octave, const std::string &outputFile,
                                      WaveletNoise &noise) // experient/main.cpp:11-36
{
    wn_grid g = wnhost::lattice2d(imageSize, octave, 2.0f, 1.0f / std::sqrt(0.19686f), WN_GRID_DEFAULT);
    wnhost::run_grid(imageSize, outputFile, [&](float *out) {
        wnhost::check(wn_eval2d_grid(noise.tile(2), &g, out, nullptr), "wn_eval2d_grid");
    });
    std::cout << "Generated Wavelet 2D Octave " << octave << " noise: " << outputFile << std::endl;
}

// A fractal 2-D image in one launch (absent from the reference; include/wnoise_multiband2d.h): WMultibandNoise with
// evaluate2D bands at p = (i / imageSize) * 4 on both axes, bands while (s + firstBand) + b < 0, divided by
// sqrt(sum w^2 * variance); the file format of the generators above.
inline void generate2DMultibandNoise(int imageSize, float s, int firstBand, int nbands, const float *w,
                                     const std::string &outputFile, WaveletNoise &noise, float variance = 0.19686f)
{
    wn_grid g = wnhost::lattice2d(imageSize, 0, 1.0f, 1.0f, WN_GRID_DEFAULT);
    wnhost::run_grid(imageSize, outputFile, [&](float *out) {
        wnhost::check(wn_multiband2d_grid(noise.tile(2), &g, s, firstBand, nbands, w, variance, out, nullptr),
                      "wn_multiband2d_grid");
    });
    std::cout << "Generated Wavelet 2D Multiband (" << nbands << " bands) noise: " << outputFile << std::endl;
}

inline void generate3DSlicedOctaveBandNoise(int imageSize, int octave, const std::string &outputFile,
                                            WaveletNoise &noise, int flags = WN_GRID_EXACT) // :38-64
{
    wn_grid g = wnhost::lattice2d(imageSize, octave, 2.0f, 1.0f / std::sqrt(0.18402f), flags);
    g.z_mode = WN_Z_CONST;
    g.z_const = 1.0f * 2.0f; // p[2] = 1.0f; p[2] *= 2.0f (:46,54)
    wnhost::run_grid(imageSize, outputFile, [&](float *out) {
        wnhost::check(wn_eval3d_grid(noise.tile(3), &g, out, nullptr), "wn_eval3d_grid");
    });
    std::cout << "Generated Wavelet 3D Sliced Octave " << octave << " noise: " << outputFile << std::endl;
}

inline void generate3DProjectedOctaveBandNoise(int imageSize, int octave, const std::string &outputFile,
                                               WaveletNoise &noise) // :66-93
{
    wn_grid g = wnhost::lattice2d(imageSize, octave, 2.0f, 1.0f / std::sqrt(0.296f), WN_GRID_DEFAULT);
    g.z_mode = WN_Z_CONST;
    g.z_const = 1.0f * 2.0f;
    const float normal[3] = {0.0f, 0.0f, 1.0f};
    wnhost::run_grid(imageSize, outputFile, [&](float *out) {
        wnhost::check(wn_eval3d_projected_grid(noise.tile(3), &g, normal, out, nullptr), "wn_eval3d_projected_grid");
    });
    std::cout << "Generated Wavelet 3D Projected Octave " << octave << " noise: " << outputFile << std::endl;
}

inline void generatePerlinNoise2D(int imageSize, int octave, const std::string &outputFile,
                                  const PerlinNoise &perlin) // :95-111
{
    wn_grid g = wnhost::lattice2d(imageSize, octave, 1.0f, 1.0f, WN_GRID_DEFAULT);
    g.z_mode = WN_Z_CONST;
    g.z_const = 0.0f; // noise(x, y) == noise(x, y, 0.0)
    wnhost::run_grid(imageSize, outputFile, [&](float *out) {
        wnhost::check(wn_perlin_grid(perlin.perm(), &g, out, nullptr), "wn_perlin_grid");
    });
    std::cout << "Generated Perlin 2D Octave " << octave << " noise: " << outputFile << std::endl;
}

inline void generatePerlinNoise3DSliced(int imageSize, int octave, const std::string &outputFile,
                                        const PerlinNoise &perlin) // :113-129
{
    wn_grid g = wnhost::lattice2d(imageSize, octave, 1.0f, 1.0f, WN_GRID_DEFAULT);
    g.z_mode = WN_Z_CONST;
    g.z_const = 1.0f * g.octave_scale; // :122
    wnhost::run_grid(imageSize, outputFile, [&](float *out) {
        wnhost::check(wn_perlin_grid(perlin.perm(), &g, out, nullptr), "wn_perlin_grid");
    });
    std::cout << "Generated Perlin 3D Sliced Octave " << octave << " noise: " << outputFile << std::endl;
}

// ---- sparse brick lists (include/wnoise_bricks.h; absent from the reference) -------------------------------------------
// The lattices of the volume generators on a device list of n 8 x 8 x 8 bricks (bx, by, bz): brick i fills
// out_dev[512 i + lx + 8 (ly + 8 lz)].  bounds = {nx, ny, z0, z1} (nullptr: den on each axis) says which bricks are in
// range; the others are left untouched.  Both only enqueue on `stream`: the list and the output stay on the device, where
// a sparse-volume holder keeps them.
namespace wnhost {
inline wn_grid brick_lattice(int den, const int *bounds, float octave_scale, float post_scale, float out_scale, int flags)
{
    wn_grid g{};
    g.den = den;
    g.nx = bounds ? bounds[0] : den;
    g.ny = bounds ? bounds[1] : den;
    g.z0 = bounds ? bounds[2] : 0;
    g.z1 = bounds ? bounds[3] : den;
    g.base_range = 4.0f;
    g.octave_scale = octave_scale;
    g.post_scale = post_scale;
    g.z_mode = WN_Z_LATTICE;
    g.out_scale = out_scale;
    g.flags = flags;
    return g;
}
} // namespace wnhost

// q = ((i / den) * 4) * 2^octave * 2 on all three axes, evaluate3D(q) / sqrt(0.18402): config 2's lattice.
inline void waveletBricks(WaveletNoise &noise, int den, const int32_t *bricks_dev, size_t n, int octave, float *out_dev,
                          const int *bounds = nullptr, int flags = WN_GRID_DEFAULT, void *stream = nullptr)
{
    const wn_grid g = wnhost::brick_lattice(den, bounds, std::pow(2.0f, octave), 2.0f, 1.0f / std::sqrt(0.18402f), flags);
    wnhost::check(wn_eval3d_bricks(noise.tile(3), &g, bricks_dev, n, out_dev, stream), "wn_eval3d_bricks");
}

// WMultibandNoise(p = (i / den) * 4, s, NULL, firstBand, nbands, w): config 3's lattice.
inline void multibandBricks(WaveletNoise &noise, int den, const int32_t *bricks_dev, size_t n, float s, int firstBand,
                            int nbands, const float *w, float *out_dev, float variance = 0.18402f,
                            const int *bounds = nullptr, int flags = WN_GRID_DEFAULT, void *stream = nullptr)
{
    const wn_grid g = wnhost::brick_lattice(den, bounds, 1.0f, 1.0f, 1.0f, flags);
    wnhost::check(wn_multiband3d_bricks(noise.tile(3), &g, bricks_dev, n, s, firstBand, nbands, w, variance, out_dev, stream),
                  "wn_multiband3d_bricks");
}

// ---- gradient and curl brick lists (include/wnoise_brick_fields.h; absent from the reference) ---------------------------
// The same lattices and lists with the derivative fields: CH channel arrays of n slots each, channel ch of brick i at
// out_dev[(ch n + i) 512 + lx + 8 (ly + 8 lz)]; CH = 4 {value, d/dx, d/dy, d/dz} for the gradient, 3 {vx, vy, vz} for the
// curl, whose offsets9 = (x, y, z) of psi0, psi1, psi2 default to noise.defaultCurlOffsets() (nullptr).
inline void waveletGradientBricks(WaveletNoise &noise, int den, const int32_t *bricks_dev, size_t n, int octave, float *out_dev,
                                  const int *bounds = nullptr, int flags = WN_GRID_DEFAULT, void *stream = nullptr)
{
    const wn_grid g = wnhost::brick_lattice(den, bounds, std::pow(2.0f, octave), 2.0f, 1.0f / std::sqrt(0.18402f), flags);
    wnhost::check(wn_eval3d_grad_bricks(noise.tile(3), &g, bricks_dev, n, out_dev, stream), "wn_eval3d_grad_bricks");
}

inline void multibandGradientBricks(WaveletNoise &noise, int den, const int32_t *bricks_dev, size_t n, float s, int firstBand,
                                    int nbands, const float *w, float *out_dev, float variance = 0.18402f,
                                    const int *bounds = nullptr, int flags = WN_GRID_DEFAULT, void *stream = nullptr)
{
    const wn_grid g = wnhost::brick_lattice(den, bounds, 1.0f, 1.0f, 1.0f, flags);
    wnhost::check(wn_multiband3d_grad_bricks(noise.tile(3), &g, bricks_dev, n, s, firstBand, nbands, w, variance, out_dev, stream),
                  "wn_multiband3d_grad_bricks");
}

inline void curlBricks(WaveletNoise &noise, int den, const int32_t *bricks_dev, size_t n, int octave, const int *offsets9,
                       float *out_dev, const int *bounds = nullptr, int flags = WN_GRID_DEFAULT, void *stream = nullptr)
{
    static_assert(sizeof(int) == sizeof(int32_t), "offsets are int32");
    int def[9];
    if (!offsets9) noise.defaultCurlOffsets(def);
    const wn_grid g = wnhost::brick_lattice(den, bounds, std::pow(2.0f, octave), 2.0f, 1.0f / std::sqrt(0.18402f), flags);
    wnhost::check(wn_eval3d_curl_bricks(noise.tile(3), &g, bricks_dev, n, reinterpret_cast<const int32_t *>(offsets9 ? offsets9 : def),
                                        out_dev, stream),
                  "wn_eval3d_curl_bricks");
}

inline void multibandCurlBricks(WaveletNoise &noise, int den, const int32_t *bricks_dev, size_t n, const int *offsets9, float s,
                                int firstBand, int nbands, const float *w, float *out_dev, float variance = 0.18402f,
                                const int *bounds = nullptr, int flags = WN_GRID_DEFAULT, void *stream = nullptr)
{
    int def[9];
    if (!offsets9) noise.defaultCurlOffsets(def);
    const wn_grid g = wnhost::brick_lattice(den, bounds, 1.0f, 1.0f, 1.0f, flags);
    wnhost::check(wn_multiband3d_curl_bricks(noise.tile(3), &g, bricks_dev, n,
                                             reinterpret_cast<const int32_t *>(offsets9 ? offsets9 : def), s, firstBand, nbands, w,
                                             variance, out_dev, stream),
                  "wn_multiband3d_curl_bricks");
}

// ---- curl brick lists with solid boundaries (include/wnoise_bounded_bricks.h; absent from the reference) ----------------
// curlBricks / multibandCurlBricks with the potential faded to zero towards the nobs obstacles of include/wnoise_bounded.h,
// which live in the coordinate the derivative is taken in: the sample's noise-space coordinate, or the multiband lattice's p.
// nobs == 0 gives the unbounded bits.
inline void curlBoundedBricks(WaveletNoise &noise, int den, const int32_t *bricks_dev, size_t n, int octave, const int *offsets9,
                              const wn_obstacle *obstacles, int nobs, float *out_dev, const int *bounds = nullptr,
                              int flags = WN_GRID_DEFAULT, void *stream = nullptr)
{
    int def[9];
    if (!offsets9) noise.defaultCurlOffsets(def);
    const wn_grid g = wnhost::brick_lattice(den, bounds, std::pow(2.0f, octave), 2.0f, 1.0f / std::sqrt(0.18402f), flags);
    wnhost::check(wn_eval3d_curl_bounded_bricks(noise.tile(3), &g, bricks_dev, n,
                                                reinterpret_cast<const int32_t *>(offsets9 ? offsets9 : def), obstacles, nobs,
                                                out_dev, stream),
                  "wn_eval3d_curl_bounded_bricks");
}

inline void multibandCurlBoundedBricks(WaveletNoise &noise, int den, const int32_t *bricks_dev, size_t n, const int *offsets9,
                                       float s, int firstBand, int nbands, const float *w, const wn_obstacle *obstacles,
                                       int nobs, float *out_dev, float variance = 0.18402f, const int *bounds = nullptr,
                                       int flags = WN_GRID_DEFAULT, void *stream = nullptr)
{
    int def[9];
    if (!offsets9) noise.defaultCurlOffsets(def);
    const wn_grid g = wnhost::brick_lattice(den, bounds, 1.0f, 1.0f, 1.0f, flags);
    wnhost::check(wn_multiband3d_curl_bounded_bricks(noise.tile(3), &g, bricks_dev, n,
                                                     reinterpret_cast<const int32_t *>(offsets9 ? offsets9 : def), s, firstBand,
                                                     nbands, w, variance, obstacles, nobs, out_dev, stream),
                  "wn_multiband3d_curl_bounded_bricks");
}

// ---- sparse brick lists of Perlin noise (include/wnoise_perlin_bricks.h; absent from the reference) ---------------------
// The lattice of generatePerlinNoise3DSliced on all three axes, p = ((i / den) * 4) * 2^octave (octave 0: turb's p), on the
// same device lists and slots: one array of n slots for the values; 4 {value, d/dx, d/dy, d/dz} for the gradients and
// 3 {vx, vy, vz} for the curl, laid out as the wavelet derivative bricks above.  Every sample has the bits of the dense
// wn_perlin_*_grid call over the lattice.  Perlin: `perlin` (perlin.h) or `PerlinNoise`, anything with perm().  kind:
// WN_PERLIN_CURL_NOISE / _TURB / _FRACTAL, depth read by TURB only; offsets9 = (x, y, z) of psi0, psi1, psi2, nullptr:
// perlin::default_curl_offsets()'s values.
namespace wnhost {
inline wn_grid perlin_brick_lattice(int den, const int *bounds, int octave)
{
    return brick_lattice(den, bounds, std::pow(2.0f, octave), 1.0f, 1.0f, WN_GRID_DEFAULT);
}
} // namespace wnhost

template <class Perlin>
inline void perlinBricks(const Perlin &perlin, int den, const int32_t *bricks_dev, size_t n, int octave, float *out_dev,
                         const int *bounds = nullptr, void *stream = nullptr)
{
    const wn_grid g = wnhost::perlin_brick_lattice(den, bounds, octave);
    wnhost::check(wn_perlin_bricks(perlin.perm(), &g, bricks_dev, n, out_dev, stream), "wn_perlin_bricks");
}

template <class Perlin>
inline void turbBricks(const Perlin &perlin, int den, const int32_t *bricks_dev, size_t n, float *out_dev, int depth = 7,
                       int octave = 0, const int *bounds = nullptr, void *stream = nullptr)
{
    const wn_grid g = wnhost::perlin_brick_lattice(den, bounds, octave);
    wnhost::check(wn_perlin_turb_bricks(perlin.perm(), &g, depth, bricks_dev, n, out_dev, stream), "wn_perlin_turb_bricks");
}

template <class Perlin>
inline void fractalBricks(const Perlin &perlin, int den, const int32_t *bricks_dev, size_t n, float *out_dev, int octave = 0,
                          const int *bounds = nullptr, void *stream = nullptr)
{
    const wn_grid g = wnhost::perlin_brick_lattice(den, bounds, octave);
    wnhost::check(wn_perlin_fractal_bricks(perlin.perm(), &g, bricks_dev, n, out_dev, stream), "wn_perlin_fractal_bricks");
}

template <class Perlin>
inline void perlinGradientBricks(const Perlin &perlin, int den, const int32_t *bricks_dev, size_t n, int octave, float *out_dev,
                                 const int *bounds = nullptr, void *stream = nullptr)
{
    const wn_grid g = wnhost::perlin_brick_lattice(den, bounds, octave);
    wnhost::check(wn_perlin_grad_bricks(perlin.perm(), &g, bricks_dev, n, out_dev, stream), "wn_perlin_grad_bricks");
}

template <class Perlin>
inline void turbGradientBricks(const Perlin &perlin, int den, const int32_t *bricks_dev, size_t n, float *out_dev, int depth = 7,
                               int octave = 0, const int *bounds = nullptr, void *stream = nullptr)
{
    const wn_grid g = wnhost::perlin_brick_lattice(den, bounds, octave);
    wnhost::check(wn_perlin_turb_grad_bricks(perlin.perm(), &g, depth, bricks_dev, n, out_dev, stream), "wn_perlin_turb_grad_bricks");
}

template <class Perlin>
inline void fractalGradientBricks(const Perlin &perlin, int den, const int32_t *bricks_dev, size_t n, float *out_dev,
                                  int octave = 0, const int *bounds = nullptr, void *stream = nullptr)
{
    const wn_grid g = wnhost::perlin_brick_lattice(den, bounds, octave);
    wnhost::check(wn_perlin_fractal_grad_bricks(perlin.perm(), &g, bricks_dev, n, out_dev, stream), "wn_perlin_fractal_grad_bricks");
}

template <class Perlin>
inline void perlinCurlBricks(const Perlin &perlin, int den, const int32_t *bricks_dev, size_t n, int octave, float *out_dev,
                             int kind = WN_PERLIN_CURL_NOISE, int depth = 7, const int *offsets9 = nullptr,
                             const int *bounds = nullptr, void *stream = nullptr)
{
    static_assert(sizeof(int) == sizeof(int32_t), "offsets are int32");
    static const int def[9] = {0, 0, 0, 85, 85, 85, 170, 170, 170};
    const wn_grid g = wnhost::perlin_brick_lattice(den, bounds, octave);
    wnhost::check(wn_perlin_curl_bricks(perlin.perm(), &g, kind, depth, reinterpret_cast<const int32_t *>(offsets9 ? offsets9 : def),
                                        bricks_dev, n, out_dev, stream),
                  "wn_perlin_curl_bricks");
}

// ---- Perlin curl brick lists with solid boundaries (include/wnoise_perlin_bounded_bricks.h; absent from the reference) --
// perlinCurlBricks with the potential faded to zero towards the nobs obstacles of include/wnoise_bounded.h, which live in the
// coordinate noise() / turb() / fractal_noise() receives: the sample's p.  nobs == 0 gives the unbounded bits.
template <class Perlin>
inline void perlinCurlBoundedBricks(const Perlin &perlin, int den, const int32_t *bricks_dev, size_t n, int octave,
                                    const wn_obstacle *obstacles, int nobs, float *out_dev, int kind = WN_PERLIN_CURL_NOISE,
                                    int depth = 7, const int *offsets9 = nullptr, const int *bounds = nullptr,
                                    void *stream = nullptr)
{
    static_assert(sizeof(int) == sizeof(int32_t), "offsets are int32");
    static const int def[9] = {0, 0, 0, 85, 85, 85, 170, 170, 170};
    const wn_grid g = wnhost::perlin_brick_lattice(den, bounds, octave);
    wnhost::check(wn_perlin_curl_bounded_bricks(perlin.perm(), &g, kind, depth,
                                                reinterpret_cast<const int32_t *>(offsets9 ? offsets9 : def), obstacles, nobs,
                                                bricks_dev, n, out_dev, stream),
                  "wn_perlin_curl_bounded_bricks");
}
