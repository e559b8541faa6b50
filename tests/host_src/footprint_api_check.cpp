// Host check of the per-sample-footprint members of class WaveletNoise (host/WaveletNoise.h) and of class
// wavelet_multiband_texture (host/texture.h) against each other and the C ABI (include/wnoise_footprint.h):
//  (1) the batched WMultibandNoise(xyz, normals, oneNormal, n, s, fade, ...) -- wn_multiband3d[_projected]_footprint_points
//      on the device -- has, per point, the bits of the scalar member WMultibandNoise(p, s_i, fade, normal, ...), which the
//      host evaluator serves; normals: none, one per point, one for all;
//  (2) the same for WMultibandNoiseGradient, all four channels; its value channel has the bits of (1);
//  (3) without fade, the points that share one s have the bits of the uniform batched overload at that s;
//  (4) wavelet_multiband_texture: grey(xyz, s, active, n, out) has the bits of value() at the default footprint s_i, leaves
//      inactive points alone, and the default footprint starts at -infinity (all bands).
// Test infrastructure: built by tests/test_gpu_footprint.py with g++ -ffp-contract=off against libwnoise_host.so.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "WaveletNoise.h"
#include "texture.h"

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
    std::mt19937 rng(7);
    std::uniform_real_distribution<float> coord(-40.0f, 40.0f), foot(-6.5f, 1.5f), unit(-1.0f, 1.0f);
    std::vector<float> xyz(3 * n), nrm(3 * n), s(n);
    const float inf = std::numeric_limits<float>::infinity();
    const float special[] = {-inf, inf, std::numeric_limits<float>::quiet_NaN(), 0.0f, -1.0f, -2.0f, -3.0f, -4.0f, -5.0f,
                             std::nextafter(-2.0f, 0.0f), std::nextafter(-2.0f, -3.0f), -2.5f, -0.25f};
    for (size_t i = 0; i < n; ++i) {
        float len = 0.0f;
        for (int k = 0; k < 3; ++k) {
            xyz[3 * i + k] = coord(rng);
            nrm[3 * i + k] = unit(rng);
            len += nrm[3 * i + k] * nrm[3 * i + k];
        }
        len = std::sqrt(len) > 1e-3f ? std::sqrt(len) : 1.0f;
        for (int k = 0; k < 3; ++k) nrm[3 * i + k] /= len;
        s[i] = i % 3 == 0 ? special[(i / 3) % (sizeof(special) / sizeof(special[0]))] : foot(rng);
    }

    WaveletNoise noise(128, 12345);
    noise.generateNoiseTile3D();

    for (int fade = 0; fade < 2; ++fade)
        for (int mode = 0; mode < 3; ++mode) { // normals: none, one per point, one for all
            const float *normals = mode == 0 ? nullptr : nrm.data();
            const bool one = mode == 2;
            const float variance = mode == 0 ? 0.18402f : 0.296f;
            std::vector<float> val(n), rec(4 * n);
            noise.WMultibandNoise(xyz.data(), normals, one, n, s.data(), fade != 0, first, nb, w, variance, val.data());
            noise.WMultibandNoiseGradient(xyz.data(), normals, one, n, s.data(), fade != 0, first, nb, w, variance, rec.data());
            for (size_t i = 0; i < n; ++i) {
                const float *nr = mode == 0 ? nullptr : (one ? nrm.data() : nrm.data() + 3 * i);
                float g[3];
                const float v = noise.WMultibandNoise(xyz.data() + 3 * i, s[i], fade != 0, nr, first, nb, w, variance);
                const float vg = noise.WMultibandNoiseGradient(xyz.data() + 3 * i, s[i], fade != 0, nr, first, nb, w, g, variance);
                expect(bits(v) == bits(val[i]), "batched value vs scalar member", i);
                expect(bits(vg) == bits(v) && bits(rec[4 * i]) == bits(v), "gradient value channel", i);
                for (int k = 0; k < 3; ++k) expect(bits(g[k]) == bits(rec[4 * i + 1 + k]), "batched gradient vs scalar member", i);
            }
            if (fade == 0 && mode != 1) { // (3): the uniform overloads, one call per shared footprint
                for (float su : {-inf, inf, 0.0f, -1.0f, -2.0f, -5.0f, -2.5f}) {
                    std::vector<float> sub, uni4;
                    std::vector<size_t> idx;
                    for (size_t i = 0; i < n; ++i)
                        if (s[i] == su) {
                            idx.push_back(i);
                            sub.insert(sub.end(), xyz.begin() + 3 * i, xyz.begin() + 3 * i + 3);
                        }
                    if (idx.empty()) { expect(false, "no point at a shared footprint", 0); continue; }
                    uni4.resize(4 * idx.size());
                    noise.WMultibandNoiseGradient(sub.data(), normals, true, idx.size(), su, first, nb, w, variance, uni4.data());
                    for (size_t j = 0; j < idx.size(); ++j)
                        for (int k = 0; k < 4; ++k)
                            expect(bits(uni4[4 * j + k]) == bits(rec[4 * idx[j] + k]), "hard cut vs the uniform overload", idx[j]);
                }
            }
        }

    // (4) the texture
    for (int fade = 0; fade < 2; ++fade) {
        wavelet_multiband_texture tex(3.7, first, nb, w, 0.18402f, fade != 0);
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
