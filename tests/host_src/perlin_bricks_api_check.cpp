// Host check of perlinBricks, turbBricks, fractalBricks, perlinGradientBricks, turbGradientBricks, fractalGradientBricks and
// perlinCurlBricks (host/noise_grid.h) against the C ABI (include/wnoise_perlin_bricks.h): on a list of in-range and
// out-of-range bricks the host functions leave the bits that the wn_perlin_*_bricks calls leave for the wn_grid the Python
// wrappers describe, untouched slots included in every channel; null offsets mean perlin::default_curl_offsets(); class
// perlin and class PerlinNoise with the same seed give the same bits; and every in-range sample has the bits of class
// perlin's scalar members (gradient and curl members: the kernels' evaluators on the host) at the sample's float coordinates.
// Test infrastructure: built by tests/test_gpu_perlin_bricks.py with g++ -ffp-contract=off against libwnoise_host.so.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "noise_grid.h"
#include "perlin.h"
#include "wnoise_perlin_bricks.h"

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

// One call into ch channel arrays of n slots that hold kFill everywhere.
template <typename F>
static std::vector<float> run(size_t ch, size_t n, F call)
{
    std::vector<float> host(ch * 512 * n, kFill);
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
    wn_grid g0 = g; // turb's and fractal_noise's default lattice: octave 0
    g0.octave_scale = 1.0f;

    const std::vector<float> val = run(1, n, [&](float *out) { check(wn_perlin_bricks(pm, &g, bd, n, out, nullptr), "wn_perlin_bricks"); });
    same(val, run(1, n, [&](float *out) { perlinBricks(noise, den, bd, n, octave, out, bounds); }), "perlinBricks");
    same(val, run(1, n, [&](float *out) { perlinBricks(plain, den, bd, n, octave, out, bounds); }), "perlinBricks(PerlinNoise)");
    const std::vector<float> turb = run(1, n, [&](float *out) { check(wn_perlin_turb_bricks(pm, &g0, depth, bd, n, out, nullptr), "wn_perlin_turb_bricks"); });
    same(turb, run(1, n, [&](float *out) { turbBricks(noise, den, bd, n, out, depth, 0, bounds); }), "turbBricks");
    const std::vector<float> frac = run(1, n, [&](float *out) { check(wn_perlin_fractal_bricks(pm, &g0, bd, n, out, nullptr), "wn_perlin_fractal_bricks"); });
    same(frac, run(1, n, [&](float *out) { fractalBricks(noise, den, bd, n, out, 0, bounds); }), "fractalBricks");

    const std::vector<float> grad = run(4, n, [&](float *out) { check(wn_perlin_grad_bricks(pm, &g, bd, n, out, nullptr), "wn_perlin_grad_bricks"); });
    same(grad, run(4, n, [&](float *out) { perlinGradientBricks(noise, den, bd, n, octave, out, bounds); }), "perlinGradientBricks");
    const std::vector<float> tgrad = run(4, n, [&](float *out) { check(wn_perlin_turb_grad_bricks(pm, &g0, depth, bd, n, out, nullptr), "wn_perlin_turb_grad_bricks"); });
    same(tgrad, run(4, n, [&](float *out) { turbGradientBricks(noise, den, bd, n, out, depth, 0, bounds); }), "turbGradientBricks");
    const std::vector<float> fgrad = run(4, n, [&](float *out) { check(wn_perlin_fractal_grad_bricks(pm, &g0, bd, n, out, nullptr), "wn_perlin_fractal_grad_bricks"); });
    same(fgrad, run(4, n, [&](float *out) { fractalGradientBricks(noise, den, bd, n, out, 0, bounds); }), "fractalGradientBricks");

    const std::vector<float> curl = run(3, n, [&](float *out) {
        check(wn_perlin_curl_bricks(pm, &g, WN_PERLIN_CURL_NOISE, 0, mixed, bd, n, out, nullptr), "wn_perlin_curl_bricks");
    });
    same(curl, run(3, n, [&](float *out) { perlinCurlBricks(noise, den, bd, n, octave, out, WN_PERLIN_CURL_NOISE, 0, mixed, bounds); }), "perlinCurlBricks");
    const std::vector<float> tcurl = run(3, n, [&](float *out) {
        check(wn_perlin_curl_bricks(pm, &g, WN_PERLIN_CURL_TURB, depth, perlin::default_curl_offsets(), bd, n, out, nullptr), "wn_perlin_curl_bricks");
    });
    same(tcurl, run(3, n, [&](float *out) { perlinCurlBricks(plain, den, bd, n, octave, out, WN_PERLIN_CURL_TURB, depth, nullptr, bounds); }),
         "perlinCurlBricks, turb, default offsets");

    // which slots are written, in every channel; every in-range sample against the scalar members at the float coordinates
    for (size_t i = 0; i < n; ++i) {
        const int bx = list[3 * i], by = list[3 * i + 1], bz = list[3 * i + 2];
        const bool in = bx >= 0 && bx < 5 && by >= 0 && by < 3 && bz >= 1 && bz < 4;
        for (int l = 0; l < 512; ++l) {
            const size_t e = 512 * i + l;
            expect((bits(val[e]) != bits(kFill)) == in && (bits(turb[e]) != bits(kFill)) == in && (bits(frac[e]) != bits(kFill)) == in,
                   "in-range value slots", e);
            for (size_t ch = 0; ch < 4; ++ch)
                expect((bits(grad[ch * n * 512 + e]) != bits(kFill)) == in && (bits(tgrad[ch * n * 512 + e]) != bits(kFill)) == in &&
                           (bits(fgrad[ch * n * 512 + e]) != bits(kFill)) == in,
                       "in-range gradient slots", e);
            for (size_t ch = 0; ch < 3; ++ch)
                expect((bits(curl[ch * n * 512 + e]) != bits(kFill)) == in && (bits(tcurl[ch * n * 512 + e]) != bits(kFill)) == in,
                       "in-range curl slots", e);
            if (!in) continue;
            const int idx[3] = {8 * bx + (l & 7), 8 * by + ((l >> 3) & 7), 8 * bz + (l >> 6)};
            float p[3], p0[3];
            for (int a = 0; a < 3; ++a) {
                const float c = ((float)idx[a] / (float)den) * g.base_range;
                p0[a] = (c * g0.octave_scale) * g0.post_scale;
                p[a] = (c * g.octave_scale) * g.post_scale;
            }
            const point3 q(p[0], p[1], p[2]), q0(p0[0], p0[1], p0[2]);
            double gr[3], v[3];
            expect(bits((float)noise.noise(q)) == bits(val[e]), "perlinBricks against noise()", e);
            expect(bits((float)noise.turb(q0, depth)) == bits(turb[e]), "turbBricks against turb()", e);
            expect(bits((float)noise.fractal_noise(q0)) == bits(frac[e]), "fractalBricks against fractal_noise()", e);
            expect(bits((float)noise.noise_gradient(q, gr)) == bits(grad[e]), "perlinGradientBricks against noise_gradient(), value", e);
            for (size_t a = 0; a < 3; ++a) expect(bits((float)gr[a]) == bits(grad[(a + 1) * n * 512 + e]), "perlinGradientBricks against noise_gradient()", e);
            expect(bits((float)noise.turb_gradient(q0, gr, depth)) == bits(tgrad[e]), "turbGradientBricks against turb_gradient(), value", e);
            for (size_t a = 0; a < 3; ++a) expect(bits((float)gr[a]) == bits(tgrad[(a + 1) * n * 512 + e]), "turbGradientBricks against turb_gradient()", e);
            expect(bits((float)noise.fractal_noise_gradient(q0, gr)) == bits(fgrad[e]), "fractalGradientBricks against fractal_noise_gradient(), value", e);
            for (size_t a = 0; a < 3; ++a) expect(bits((float)gr[a]) == bits(fgrad[(a + 1) * n * 512 + e]), "fractalGradientBricks against fractal_noise_gradient()", e);
            noise.noise_curl(q, v, mixed);
            for (size_t a = 0; a < 3; ++a) expect(bits((float)v[a]) == bits(curl[a * n * 512 + e]), "perlinCurlBricks against noise_curl()", e);
            noise.turb_curl(q, v, depth);
            for (size_t a = 0; a < 3; ++a) expect(bits((float)v[a]) == bits(tcurl[a * n * 512 + e]), "perlinCurlBricks against turb_curl()", e);
        }
    }
    wn_dev_free(bricks);
    printf("bricks %zu, mismatches %ld\n", n, mismatches);
    return mismatches ? 1 : 0;
}
