// Host check of curlBoundedBricks and multibandCurlBoundedBricks (host/noise_grid.h) against the C ABI
// (include/wnoise_bounded_bricks.h): on a list of in-range and out-of-range bricks, in both tiers, the host functions leave
// the bits that the wn_*_curl_bounded_bricks calls leave for the wn_grid the Python wrappers describe, untouched slots
// included in every component; a null offsets9 means the noise object's defaultCurlOffsets(); nobs == 0 gives the bits of
// curlBricks; and the exact tier has the bits of the host's evaluate3DCurlBounded at the samples' float coordinates, times
// out_scale.  The scene is tests/test_gpu_bounded_bricks.py's: far, near and inside samples.
// Test infrastructure: built by tests/test_gpu_bounded_bricks.py with g++ -ffp-contract=off against libwnoise_host.so.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "noise_grid.h"
#include "wnoise_bounded_bricks.h"

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

// One call into three component arrays of n slots that hold kFill everywhere.
template <typename F>
static std::vector<float> run(size_t n, F call)
{
    std::vector<float> host(3 * 512 * n, kFill);
    void *out = nullptr;
    check(wn_dev_alloc(&out, host.size() * sizeof(float)), "wn_dev_alloc");
    check(wn_copy_h2d(out, host.data(), host.size() * sizeof(float), nullptr), "wn_copy_h2d");
    call(static_cast<float *>(out));
    check(wn_copy_d2h(host.data(), out, host.size() * sizeof(float), nullptr), "wn_copy_d2h");
    check(wn_stream_sync(nullptr), "wn_stream_sync");
    wn_dev_free(out);
    return host;
}

static void same(const std::vector<float> &a, const std::vector<float> &b, const char *what)
{
    expect(a.size() == b.size(), what, 0);
    for (size_t e = 0; e < a.size() && e < b.size(); ++e) expect(bits(a[e]) == bits(b[e]), what, e);
}

static wn_obstacle obstacle(int kind, float c0, float c1, float c2, float r, float d0)
{
    wn_obstacle o{};
    o.kind = kind;
    o.c[0] = c0, o.c[1] = c1, o.c[2] = c2;
    o.r = r;
    o.d0 = d0;
    return o;
}

// The scene in lattice-index units, scaled by the lattice's step h.
static std::vector<wn_obstacle> scene(float h)
{
    return {obstacle(WN_OBSTACLE_SPHERE, 19.5f * h, 11.5f * h, 19.5f * h, 7.0f * h, 5.0f * h),
            obstacle(WN_OBSTACLE_HALFSPACE, 0.0f, 1.0f, 0.0f, 2.5f * h, 3.0f * h),
            obstacle(WN_OBSTACLE_CONTAINER, 19.5f * h, 11.5f * h, 19.5f * h, 28.0f * h, 5.0f * h)};
}

int main()
{
    WaveletNoise noise(128, 12345);
    noise.generateNoiseTile3D();
    const wn_tile *t = noise.tile(3);
    const int den = 512, octave = 4;
    const int bounds[4] = {40, 24, 8, 32}; // 5 x 3 x 3 bricks in range
    const std::vector<int32_t> list = {0, 0, 1, 4, 2, 3, 2, 1, 2, -1, 0, 1, 5, 0, 1, 0, 0, 0, 0, 0, 4, 4, 2, 3, 3, 1, 2, 0, 1, 2};
    const size_t n = list.size() / 3;
    void *bricks = nullptr;
    check(wn_dev_alloc(&bricks, list.size() * sizeof(int32_t)), "wn_dev_alloc");
    check(wn_copy_h2d(bricks, list.data(), list.size() * sizeof(int32_t), nullptr), "wn_copy_h2d");
    const int32_t *bd = static_cast<const int32_t *>(bricks);
    const float w[5] = {1.0f, 0.5f, 2.0f, 1.0f, 0.25f};
    const int mixed[9] = {0, 0, 0, 1, 2, 3, -5, 7, 130};
    int def[9];
    noise.defaultCurlOffsets(def);

    for (int flags : {WN_GRID_DEFAULT, WN_GRID_EXACT}) {
        wn_grid g{};
        g.den = den;
        g.nx = bounds[0], g.ny = bounds[1], g.z0 = bounds[2], g.z1 = bounds[3];
        g.base_range = 4.0f;
        g.octave_scale = std::pow(2.0f, octave);
        g.post_scale = 2.0f;
        g.out_scale = 1.0f / std::sqrt(0.18402f);
        g.flags = flags;
        wn_grid gm = g;
        gm.octave_scale = gm.post_scale = gm.out_scale = 1.0f;
        const std::vector<wn_obstacle> so = scene(((1.0f / (float)den) * g.base_range) * g.octave_scale * g.post_scale);
        const std::vector<wn_obstacle> sm = scene((1.0f / (float)den) * gm.base_range);
        const int nobs = (int)so.size();

        const std::vector<float> curl = run(n, [&](float *out) {
            check(wn_eval3d_curl_bounded_bricks(t, &g, bd, n, mixed, so.data(), nobs, out, nullptr), "wn_eval3d_curl_bounded_bricks");
        });
        same(curl, run(n, [&](float *out) { curlBoundedBricks(noise, den, bd, n, octave, mixed, so.data(), nobs, out, bounds, flags); }),
             "curlBoundedBricks");
        const std::vector<float> dcurl = run(n, [&](float *out) {
            check(wn_eval3d_curl_bounded_bricks(t, &g, bd, n, def, so.data(), nobs, out, nullptr), "wn_eval3d_curl_bounded_bricks");
        });
        same(dcurl, run(n, [&](float *out) { curlBoundedBricks(noise, den, bd, n, octave, nullptr, so.data(), nobs, out, bounds, flags); }),
             "curlBoundedBricks, default offsets");
        const std::vector<float> mcurl = run(n, [&](float *out) {
            check(wn_multiband3d_curl_bounded_bricks(t, &gm, bd, n, mixed, -16.0f, -1, 5, w, 0.18402f, sm.data(), nobs, out, nullptr),
                  "wn_multiband3d_curl_bounded_bricks");
        });
        same(mcurl, run(n, [&](float *out) {
                 multibandCurlBoundedBricks(noise, den, bd, n, mixed, -16.0f, -1, 5, w, sm.data(), nobs, out, 0.18402f, bounds, flags);
             }),
             "multibandCurlBoundedBricks");
        const std::vector<float> mdcurl = run(n, [&](float *out) {
            check(wn_multiband3d_curl_bounded_bricks(t, &gm, bd, n, def, -16.0f, -1, 5, w, 0.18402f, sm.data(), nobs, out, nullptr),
                  "wn_multiband3d_curl_bounded_bricks");
        });
        same(mdcurl, run(n, [&](float *out) {
                 multibandCurlBoundedBricks(noise, den, bd, n, nullptr, -16.0f, -1, 5, w, sm.data(), nobs, out, 0.18402f, bounds, flags);
             }),
             "multibandCurlBoundedBricks, default offsets");
        // no obstacle: the unbounded host functions' bits
        same(run(n, [&](float *out) { curlBoundedBricks(noise, den, bd, n, octave, mixed, nullptr, 0, out, bounds, flags); }),
             run(n, [&](float *out) { curlBricks(noise, den, bd, n, octave, mixed, out, bounds, flags); }), "curlBoundedBricks, nobs == 0");
        same(run(n, [&](float *out) { multibandCurlBoundedBricks(noise, den, bd, n, mixed, -16.0f, -1, 5, w, nullptr, 0, out, 0.18402f, bounds, flags); }),
             run(n, [&](float *out) { multibandCurlBricks(noise, den, bd, n, mixed, -16.0f, -1, 5, w, out, 0.18402f, bounds, flags); }),
             "multibandCurlBoundedBricks, nobs == 0");

        // which slots are written, in every component; the exact tier against the host's evaluator at the float coordinates
        size_t zeros = 0, others = 0;
        for (size_t i = 0; i < n; ++i) {
            const int bx = list[3 * i], by = list[3 * i + 1], bz = list[3 * i + 2];
            const bool in = bx >= 0 && bx < 5 && by >= 0 && by < 3 && bz >= 1 && bz < 4;
            for (int l = 0; l < 512; ++l) {
                const size_t e = 512 * i + l;
                for (size_t ch = 0; ch < 3; ++ch)
                    expect((bits(curl[ch * n * 512 + e]) != bits(kFill)) == in && (bits(mcurl[ch * n * 512 + e]) != bits(kFill)) == in,
                           "in-range slots", e);
                if (!in || flags != WN_GRID_EXACT) continue;
                const int idx[3] = {8 * bx + (l & 7), 8 * by + ((l >> 3) & 7), 8 * bz + (l >> 6)};
                float p[3];
                for (int a = 0; a < 3; ++a) {
                    float c = ((float)idx[a] / (float)den) * g.base_range;
                    c = c * g.octave_scale;
                    p[a] = c * g.post_scale;
                }
                float v[3];
                noise.evaluate3DCurlBounded(p, mixed, so.data(), nobs, v);
                for (size_t a = 0; a < 3; ++a)
                    expect(bits(v[a] * g.out_scale) == bits(curl[a * n * 512 + e]), "exact tier against evaluate3DCurlBounded", e);
                (v[0] == 0.0f && v[1] == 0.0f && v[2] == 0.0f ? zeros : others) += 1;
            }
        }
        if (flags == WN_GRID_EXACT) expect(zeros >= 512 && others >= 512, "the list holds inside samples and others", zeros);
    }
    wn_dev_free(bricks);
    printf("bricks %zu, mismatches %ld\n", n, mismatches);
    return mismatches ? 1 : 0;
}
