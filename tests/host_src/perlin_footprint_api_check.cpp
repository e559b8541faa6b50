// Host check of the per-sample-footprint members of class perlin (host/perlin.h) and of class noise_multiband_texture
// (host/texture.h) against each other and the C ABI (include/wnoise_perlin_footprint.h):
//  (1) the batched turb_footprint / fractal_noise_footprint(xyz, s, n, out, ...) -- the kernels -- have, per point, the bits
//      of the scalar members, which the host evaluators serve;
//  (2) the same for turb_footprint_gradient / fractal_noise_footprint_gradient, all four channels; their value channel has
//      the bits of (1);
//  (3) without fade, a turb point whose footprint leaves k octaves has the bits of turb(p, k) and turb_gradient(p, g, k);
//      a fractal point with all six of six octaves those of fractal_noise(p) and fractal_noise_gradient(p, g);
//  (4) noise_multiband_texture: grey(xyz, s, active, n, out) has the bits of value() at the default footprint s_i, leaves
//      inactive points alone, and the default footprint starts at -infinity (all octaves).
// Test infrastructure: built by tests/test_gpu_perlin_footprint.py with g++ -ffp-contract=off against libwnoise_host.so.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "perlin.h"
#include "texture.h"

static uint64_t bits(double d) { uint64_t b; memcpy(&b, &d, 8); return b; }
static uint32_t bits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }

static long mismatches = 0;
static void expect(bool ok, const char *what, size_t i)
{
    if (!ok && mismatches++ < 10) printf("mismatch: %s at %zu\n", what, i);
}

int main()
{
    const size_t n = 3000;
    std::mt19937 rng(7);
    std::uniform_real_distribution<float> coord(-40.0f, 40.0f), foot(-8.5f, 1.5f);
    std::vector<float> xyz(3 * n), s(n);
    const float inf = std::numeric_limits<float>::infinity();
    const float special[] = {-inf, inf, std::numeric_limits<float>::quiet_NaN(), 0.0f, -1.0f, -2.0f, -3.0f, -6.0f, -7.0f,
                             std::nextafter(-2.0f, 0.0f), std::nextafter(-2.0f, -3.0f), -2.5f, -0.25f};
    for (size_t i = 0; i < n; ++i) {
        for (int k = 0; k < 3; ++k) xyz[3 * i + k] = i % 7 == 0 ? std::round(coord(rng)) : coord(rng);
        s[i] = i % 3 == 0 ? special[(i / 3) % (sizeof(special) / sizeof(special[0]))] : foot(rng);
    }

    perlin noise(12345);
    for (int fade = 0; fade < 2; ++fade)
        for (float bias : {0.0f, -1.0f}) {
            const int depth = 7, octaves = 6;
            const bool fd = fade != 0;
            std::vector<double> tv(n), fv(n), tg(4 * n), fg(4 * n);
            noise.turb_footprint(xyz.data(), s.data(), n, tv.data(), depth, bias, fd);
            noise.fractal_noise_footprint(xyz.data(), s.data(), n, fv.data(), octaves, bias, fd);
            noise.turb_footprint_gradient(xyz.data(), s.data(), n, tg.data(), depth, bias, fd);
            noise.fractal_noise_footprint_gradient(xyz.data(), s.data(), n, fg.data(), octaves, bias, fd);
            for (size_t i = 0; i < n; ++i) {
                const point3 q(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
                double g[3];
                const double t = noise.turb_footprint(q, s[i], depth, bias, fd);
                const double t4 = noise.turb_footprint_gradient(q, s[i], g, depth, bias, fd);
                expect(bits(t) == bits(tv[i]), "batched turb vs scalar member", i);
                expect(bits(t4) == bits(t) && bits(tg[4 * i]) == bits(t), "turb gradient value channel", i);
                for (int k = 0; k < 3; ++k) expect(bits(g[k]) == bits(tg[4 * i + 1 + k]), "batched turb gradient vs scalar member", i);
                int count = 0;
                while (count < depth && (s[i] + bias) + (float)count < 0.0f) ++count;
                if (!fd) {
                    double gu[3];
                    expect(bits(noise.turb(q, count)) == bits(t), "hard cut vs turb at the octave count", i);
                    expect(bits(noise.turb_gradient(q, gu, count)) == bits(t), "hard cut vs turb_gradient value", i);
                    for (int k = 0; k < 3; ++k) expect(bits(gu[k]) == bits(g[k]), "hard cut vs turb_gradient", i);
                }
                const double f = noise.fractal_noise_footprint(q, s[i], octaves, bias, fd);
                const double f4 = noise.fractal_noise_footprint_gradient(q, s[i], g, octaves, bias, fd);
                expect(bits(f) == bits(fv[i]), "batched fractal vs scalar member", i);
                expect(bits(f4) == bits(f) && bits(fg[4 * i]) == bits(f), "fractal gradient value channel", i);
                for (int k = 0; k < 3; ++k) expect(bits(g[k]) == bits(fg[4 * i + 1 + k]), "batched fractal gradient vs scalar member", i);
                if (!fd && (s[i] + bias) + 5.0f < 0.0f) {
                    double gu[3];
                    expect(bits(noise.fractal_noise(q)) == bits(f), "all six octaves vs fractal_noise", i);
                    expect(bits(noise.fractal_noise_gradient(q, gu)) == bits(f), "all six octaves vs fractal_noise_gradient value", i);
                    for (int k = 0; k < 3; ++k) expect(bits(gu[k]) == bits(g[k]), "all six octaves vs fractal_noise_gradient", i);
                }
            }
        }

    // (4) the texture
    for (int fade = 0; fade < 2; ++fade) {
        noise_multiband_texture tex(3.7, 6, -1.0f, fade != 0);
        expect(tex.default_footprint() == -inf, "default footprint", 0);
        std::vector<uint8_t> active(n);
        std::vector<float> grey(n, -7.0f), all(n, -7.0f);
        for (size_t i = 0; i < n; ++i) active[i] = (i * 2654435761u >> 7) % 5 < 2;
        tex.grey(xyz.data(), s.data(), active.data(), n, grey.data());
        tex.grey(xyz.data(), s.data(), nullptr, n, all.data());
        for (size_t i = 0; i < n; ++i) {
            tex.set_default_footprint(s[i]);
            const color c = tex.value(0.0, 0.0, point3(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]));
            expect(bits((float)c.x()) == bits(all[i]) && c.x() == c.y() && c.y() == c.z(), "texture grey vs value()", i);
            expect(active[i] ? bits(grey[i]) == bits(all[i]) : grey[i] == -7.0f, "masked texture grey", i);
        }
    }
    printf("mismatches %ld\n", mismatches);
    return mismatches ? 1 : 0;
}
