// Host check of the 2-D WMultibandNoise members of class WaveletNoise (host/WaveletNoise.h) and of generate2DMultibandNoise
// (host/noise_grid.h) against each other and the C ABI (include/wnoise_multiband2d.h):
//  (1) the batched WMultibandNoise2D(xy, n, s[], fade, ...) -- wn_multiband2d_footprint_points on the device -- has, per
//      point, the bits of the one-sample member WMultibandNoise2D(p, s_i, ..., fade), which the host evaluator serves;
//  (2) the same for WMultibandNoise2DGradient, all three channels; its value channel has the bits of (1);
//  (3) without fade, the points that share one s have the bits of the uniform batched overloads at that s;
//  (4) generate2DMultibandNoise writes the image whose samples are the one-sample member at p = (i / imageSize) * 4.
// Test infrastructure: built by tests/test_gpu_multiband2d.py with g++ -ffp-contract=off against libwnoise_host.so.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <limits>
#include <random>
#include <vector>

#include "WaveletNoise.h"
#include "noise_grid.h"

static uint32_t bits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }

static long mismatches = 0;
static void expect(bool ok, const char *what, size_t i)
{
    if (!ok && mismatches++ < 10) printf("mismatch: %s at %zu\n", what, i);
}

int main()
{
    const size_t n = 3000;
    const int first = 0, nb = 5;
    const float w[5] = {1.0f, 0.5f, 2.0f, 1.0f, 0.25f};
    const float variance = 0.19686f;
    std::mt19937 rng(7);
    std::uniform_real_distribution<float> coord(-40.0f, 40.0f), foot(-6.5f, 1.5f);
    std::vector<float> xy(2 * n), s(n);
    const float inf = std::numeric_limits<float>::infinity();
    const float special[] = {-inf, inf, std::numeric_limits<float>::quiet_NaN(), 0.0f, -1.0f, -2.0f, -3.0f, -4.0f, -5.0f,
                             std::nextafter(-2.0f, 0.0f), std::nextafter(-2.0f, -3.0f), -2.5f, -0.25f};
    for (size_t i = 0; i < n; ++i) {
        xy[2 * i] = coord(rng);
        xy[2 * i + 1] = coord(rng);
        s[i] = i % 3 == 0 ? special[(i / 3) % (sizeof(special) / sizeof(special[0]))] : foot(rng);
    }

    WaveletNoise noise(128, 12345);
    noise.generateNoiseTile2D();

    for (int fade = 0; fade < 2; ++fade) {
        std::vector<float> val(n), rec(3 * n);
        noise.WMultibandNoise2D(xy.data(), n, s.data(), fade != 0, first, nb, w, variance, val.data());
        noise.WMultibandNoise2DGradient(xy.data(), n, s.data(), fade != 0, first, nb, w, variance, rec.data());
        for (size_t i = 0; i < n; ++i) {
            float g[2];
            const float v = noise.WMultibandNoise2D(xy.data() + 2 * i, s[i], first, nb, w, variance, fade != 0);
            const float vg = noise.WMultibandNoise2DGradient(xy.data() + 2 * i, s[i], first, nb, w, g, variance, fade != 0);
            expect(bits(v) == bits(val[i]), "batched value vs the one-sample member", i);
            expect(bits(vg) == bits(v) && bits(rec[3 * i]) == bits(v), "gradient value channel", i);
            for (int k = 0; k < 2; ++k) expect(bits(g[k]) == bits(rec[3 * i + 1 + k]), "batched gradient vs the one-sample member", i);
        }
        if (fade == 0) { // (3): the uniform overloads, one call per shared footprint
            for (float su : {-inf, inf, 0.0f, -1.0f, -2.0f, -5.0f, -2.5f}) {
                std::vector<float> sub, uni(0), uni3;
                std::vector<size_t> idx;
                for (size_t i = 0; i < n; ++i)
                    if (s[i] == su) {
                        idx.push_back(i);
                        sub.insert(sub.end(), xy.begin() + 2 * i, xy.begin() + 2 * i + 2);
                    }
                if (idx.empty()) { expect(false, "no point at a shared footprint", 0); continue; }
                uni.resize(idx.size());
                uni3.resize(3 * idx.size());
                noise.WMultibandNoise2D(sub.data(), idx.size(), su, first, nb, w, variance, uni.data());
                noise.WMultibandNoise2DGradient(sub.data(), idx.size(), su, first, nb, w, variance, uni3.data());
                for (size_t j = 0; j < idx.size(); ++j) {
                    expect(bits(uni[j]) == bits(val[idx[j]]), "hard cut vs the uniform overload", idx[j]);
                    for (int k = 0; k < 3; ++k)
                        expect(bits(uni3[3 * j + k]) == bits(rec[3 * idx[j] + k]), "hard cut vs the uniform gradient overload", idx[j]);
                }
            }
        }
    }

    // (4) the grid generator: a 64 x 64 image, three of five bands
    const int size = 64;
    generate2DMultibandNoise(size, -2.5f, first, nb, w, "multiband2d_api_check.raw", noise);
    std::vector<float> image(size * size, -7.0f);
    std::ifstream in("multiband2d_api_check.raw", std::ios::binary);
    in.read(reinterpret_cast<char *>(image.data()), image.size() * sizeof(float));
    expect(in.gcount() == (std::streamsize)(image.size() * sizeof(float)), "image file size", 0);
    for (int y = 0; y < size; ++y)
        for (int x = 0; x < size; ++x) {
            const float p[2] = {((float)x / (float)size) * 4.0f, ((float)y / (float)size) * 4.0f};
            expect(bits(image[y * size + x]) == bits(noise.WMultibandNoise2D(p, -2.5f, first, nb, w)), "image sample", y * size + x);
        }
    std::remove("multiband2d_api_check.raw");
    printf("mismatches %ld\n", mismatches);
    return mismatches ? 1 : 0;
}
