// Host check of waveletBricks and multibandBricks (host/noise_grid.h) against the C ABI (include/wnoise_bricks.h): on a
// list of in-range and out-of-range bricks, in both tiers, the host functions leave the bits that wn_eval3d_bricks /
// wn_multiband3d_bricks leave for the wn_grid the Python wrappers describe, untouched slots included, and the exact tier
// has the bits of wn_eval3d_points at the samples' float coordinates, times out_scale.
// Test infrastructure: built by tests/test_gpu_bricks.py with g++ -ffp-contract=off against libwnoise_host.so.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "noise_grid.h"
#include "wnoise_bricks.h"

static uint32_t bits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }

static long mismatches = 0;
static void expect(bool ok, const char *what, size_t i)
{
    if (!ok && mismatches++ < 10) printf("mismatch: %s at %zu\n", what, i);
}

static void check(int rc, const char *what)
{
    if (rc != WN_OK) {
        printf("%s failed: %s\n", what, wn_last_error());
        std::exit(2);
    }
}

static const float kFill = -12345.5f;

// One call into a slot buffer that holds kFill everywhere.
template <typename F>
static std::vector<float> run(size_t n, F call)
{
    std::vector<float> host(512 * n, kFill);
    void *out = nullptr;
    check(wn_dev_alloc(&out, host.size() * sizeof(float)), "wn_dev_alloc");
    check(wn_copy_h2d(out, host.data(), host.size() * sizeof(float), nullptr), "wn_copy_h2d");
    call(static_cast<float *>(out));
    check(wn_copy_d2h(host.data(), out, host.size() * sizeof(float), nullptr), "wn_copy_d2h");
    check(wn_stream_sync(nullptr), "wn_stream_sync");
    wn_dev_free(out);
    return host;
}

int main()
{
    WaveletNoise noise(128, 12345);
    noise.generateNoiseTile3D();
    const wn_tile *t = noise.tile(3);
    const int den = 512, octave = 4;
    const int bounds[4] = {40, 24, 8, 32}; // 5 x 3 x 3 bricks in range
    const std::vector<int32_t> list = {0, 0, 1, 4, 2, 3, 2, 1, 2, -1, 0, 1, 5, 0, 1, 0, 0, 0, 0, 0, 4, 4, 2, 3, 3, 0, 2};
    const size_t n = list.size() / 3;
    void *bricks = nullptr;
    check(wn_dev_alloc(&bricks, list.size() * sizeof(int32_t)), "wn_dev_alloc");
    check(wn_copy_h2d(bricks, list.data(), list.size() * sizeof(int32_t), nullptr), "wn_copy_h2d");
    const int32_t *bd = static_cast<const int32_t *>(bricks);
    const float w[5] = {1.0f, 0.5f, 2.0f, 1.0f, 0.25f};

    for (int flags : {WN_GRID_DEFAULT, WN_GRID_EXACT}) {
        wn_grid g{};
        g.den = den;
        g.nx = bounds[0], g.ny = bounds[1], g.z0 = bounds[2], g.z1 = bounds[3];
        g.base_range = 4.0f;
        g.octave_scale = std::pow(2.0f, octave);
        g.post_scale = 2.0f;
        g.out_scale = 1.0f / std::sqrt(0.18402f);
        g.flags = flags;
        const std::vector<float> abi = run(n, [&](float *out) { check(wn_eval3d_bricks(t, &g, bd, n, out, nullptr), "wn_eval3d_bricks"); });
        const std::vector<float> host = run(n, [&](float *out) { waveletBricks(noise, den, bd, n, octave, out, bounds, flags); });
        for (size_t e = 0; e < abi.size(); ++e) expect(bits(abi[e]) == bits(host[e]), "waveletBricks", e);

        wn_grid gm = g;
        gm.octave_scale = gm.post_scale = gm.out_scale = 1.0f;
        const std::vector<float> mabi = run(n, [&](float *out) {
            check(wn_multiband3d_bricks(t, &gm, bd, n, -16.0f, -1, 5, w, 0.18402f, out, nullptr), "wn_multiband3d_bricks");
        });
        const std::vector<float> mhost = run(n, [&](float *out) {
            multibandBricks(noise, den, bd, n, -16.0f, -1, 5, w, out, 0.18402f, bounds, flags);
        });
        for (size_t e = 0; e < mabi.size(); ++e) expect(bits(mabi[e]) == bits(mhost[e]), "multibandBricks", e);

        // which slots are written; the exact tier against the host's evaluate3D at the float coordinates
        for (size_t i = 0; i < n; ++i) {
            const int bx = list[3 * i], by = list[3 * i + 1], bz = list[3 * i + 2];
            const bool in = bx >= 0 && bx < 5 && by >= 0 && by < 3 && bz >= 1 && bz < 4;
            for (int l = 0; l < 512; ++l) {
                const float v = abi[512 * i + l];
                expect((bits(v) != bits(kFill)) == in && (bits(mabi[512 * i + l]) != bits(kFill)) == in, "in-range slots", 512 * i + l);
                if (!in || flags != WN_GRID_EXACT) continue;
                const int idx[3] = {8 * bx + (l & 7), 8 * by + ((l >> 3) & 7), 8 * bz + (l >> 6)};
                float p[3];
                for (int a = 0; a < 3; ++a) {
                    float c = ((float)idx[a] / (float)den) * g.base_range;
                    c = c * g.octave_scale;
                    p[a] = c * g.post_scale;
                }
                expect(bits(noise.evaluate3D(p) * g.out_scale) == bits(v), "exact tier against evaluate3D", 512 * i + l);
            }
        }
    }
    wn_dev_free(bricks);
    printf("bricks %zu, mismatches %ld\n", n, mismatches);
    return mismatches ? 1 : 0;
}
