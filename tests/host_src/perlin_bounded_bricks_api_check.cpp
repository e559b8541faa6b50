// Host check of perlinCurlBoundedBricks (host/noise_grid.h) against the C ABI (include/wnoise_perlin_bounded_bricks.h): on a
// list of in-range and out-of-range bricks the host function leaves the bits that wn_perlin_curl_bounded_bricks leaves for
// the wn_grid the Python wrapper describes, untouched slots included in all three channels; null offsets mean
// perlin::default_curl_offsets(); class perlin and class PerlinNoise with the same seed give the same bits; no obstacle gives
// perlinCurlBricks' bits; and every in-range sample has the bits of class perlin's scalar member curl_bounded (the kernels'
// evaluators on the host) at the sample's float coordinates, for noise, turb and fractal_noise, with all three classes of
// samples present.
// Test infrastructure: built by tests/test_gpu_perlin_bounded_bricks.py with g++ -ffp-contract=off against libwnoise_host.so.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "noise_grid.h"
#include "perlin.h"
#include "wnoise_perlin_bounded_bricks.h"

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

// One call into 3 channel arrays of n slots that hold kFill everywhere.
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

int main()
{
    const perlin noise(12345);
    const PerlinNoise plain(12345);
    const wn_perm *pm = noise.perm();
    const int den = 385, octave = 4, depth = 5; // a non-dyadic step: cell faces inside the rows
    const int bounds[4] = {40, 24, 8, 32};      // 5 x 3 x 3 bricks in range
    const std::vector<int32_t> list = {0, 0, 1, 4, 2, 3, 2, 1, 2, -1, 0, 1, 5, 0, 1, 0, 0, 0, 0, 0, 4, 4, 2, 3, 3, 0, 2};
    const size_t n = list.size() / 3;
    void *bricks = nullptr;
    check(wn_dev_alloc(&bricks, list.size() * sizeof(int32_t)), "wn_dev_alloc");
    check(wn_copy_h2d(bricks, list.data(), list.size() * sizeof(int32_t), nullptr), "wn_copy_h2d");
    const int32_t *bd = static_cast<const int32_t *>(bricks);
    const int mixed[9] = {0, 0, 0, 1, 2, 3, -5, 7, 130};

    wn_grid g{};
    g.den = den;
    g.nx = bounds[0], g.ny = bounds[1], g.z0 = bounds[2], g.z1 = bounds[3];
    g.base_range = 4.0f;
    g.octave_scale = std::pow(2.0f, octave);
    g.post_scale = 1.0f;
    g.out_scale = 1.0f;

    // a sphere in the volume, a floor and a container, in units of the lattice's step
    const float h = (1.0f / (float)den) * g.base_range * g.octave_scale;
    wn_obstacle obs[3] = {};
    obs[0].kind = WN_OBSTACLE_SPHERE;
    obs[0].c[0] = 19.5f * h, obs[0].c[1] = 11.5f * h, obs[0].c[2] = 19.5f * h;
    obs[0].r = 7.0f * h, obs[0].d0 = 5.0f * h;
    obs[1].kind = WN_OBSTACLE_HALFSPACE;
    obs[1].c[1] = 1.0f;
    obs[1].r = 2.5f * h, obs[1].d0 = 3.0f * h;
    obs[2].kind = WN_OBSTACLE_CONTAINER;
    obs[2].c[0] = obs[0].c[0], obs[2].c[1] = obs[0].c[1], obs[2].c[2] = obs[0].c[2];
    obs[2].r = 28.0f * h, obs[2].d0 = 5.0f * h;

    const int kinds[3] = {WN_PERLIN_CURL_NOISE, WN_PERLIN_CURL_TURB, WN_PERLIN_CURL_FRACTAL};
    std::vector<float> abi[3];
    for (int k = 0; k < 3; ++k) {
        const int kind = kinds[k];
        abi[k] = run(n, [&](float *out) {
            check(wn_perlin_curl_bounded_bricks(pm, &g, kind, depth, mixed, obs, 3, bd, n, out, nullptr), "wn_perlin_curl_bounded_bricks");
        });
        same(abi[k], run(n, [&](float *out) { perlinCurlBoundedBricks(noise, den, bd, n, octave, obs, 3, out, kind, depth, mixed, bounds); }),
             "perlinCurlBoundedBricks");
        same(abi[k], run(n, [&](float *out) { perlinCurlBoundedBricks(plain, den, bd, n, octave, obs, 3, out, kind, depth, mixed, bounds); }),
             "perlinCurlBoundedBricks(PerlinNoise)");
    }
    // null offsets: the defaults; no obstacle: the unbounded host function's bits
    const std::vector<float> dflt = run(n, [&](float *out) {
        check(wn_perlin_curl_bounded_bricks(pm, &g, WN_PERLIN_CURL_TURB, depth, perlin::default_curl_offsets(), obs, 3, bd, n, out, nullptr),
              "wn_perlin_curl_bounded_bricks");
    });
    same(dflt, run(n, [&](float *out) { perlinCurlBoundedBricks(noise, den, bd, n, octave, obs, 3, out, WN_PERLIN_CURL_TURB, depth, nullptr, bounds); }),
         "perlinCurlBoundedBricks, default offsets");
    same(run(n, [&](float *out) { perlinCurlBricks(noise, den, bd, n, octave, out, WN_PERLIN_CURL_TURB, depth, mixed, bounds); }),
         run(n, [&](float *out) { perlinCurlBoundedBricks(noise, den, bd, n, octave, nullptr, 0, out, WN_PERLIN_CURL_TURB, depth, mixed, bounds); }),
         "perlinCurlBoundedBricks without obstacles");

    // which slots are written, in every channel; every in-range sample against the scalar member at the float coordinates
    long zeros = 0, moved = 0, live = 0;
    const std::vector<float> free_noise = run(n, [&](float *out) { perlinCurlBricks(noise, den, bd, n, octave, out, WN_PERLIN_CURL_NOISE, depth, mixed, bounds); });
    for (size_t i = 0; i < n; ++i) {
        const int bx = list[3 * i], by = list[3 * i + 1], bz = list[3 * i + 2];
        const bool in = bx >= 0 && bx < 5 && by >= 0 && by < 3 && bz >= 1 && bz < 4;
        for (int l = 0; l < 512; ++l) {
            const size_t e = 512 * i + l;
            for (int k = 0; k < 3; ++k)
                for (size_t ch = 0; ch < 3; ++ch) expect((bits(abi[k][ch * n * 512 + e]) != bits(kFill)) == in, "in-range slots", e);
            if (!in) continue;
            const int idx[3] = {8 * bx + (l & 7), 8 * by + ((l >> 3) & 7), 8 * bz + (l >> 6)};
            double q[3];
            for (int a = 0; a < 3; ++a) q[a] = (double)(((((float)idx[a] / (float)den) * g.base_range) * g.octave_scale) * g.post_scale);
            for (int k = 0; k < 3; ++k) {
                double v[3];
                noise.curl_bounded(q, kinds[k], depth, mixed, obs, 3, v);
                for (size_t a = 0; a < 3; ++a) expect(bits((float)v[a]) == bits(abi[k][a * n * 512 + e]), "against perlin::curl_bounded()", e);
            }
            ++live;
            zeros += abi[0][e] == 0.0f && abi[0][n * 512 + e] == 0.0f && abi[0][2 * n * 512 + e] == 0.0f;
            moved += bits(abi[0][e]) != bits(free_noise[e]);
        }
    }
    // the scene reaches the list: samples inside a solid, and samples whose velocity the ramp changed
    expect(zeros > live / 10 && moved > zeros + live / 10 && moved < live, "the classes of the scene", (size_t)zeros);
    wn_dev_free(bricks);
    printf("bricks %zu, mismatches %ld\n", n, mismatches);
    return mismatches ? 1 : 0;
}
