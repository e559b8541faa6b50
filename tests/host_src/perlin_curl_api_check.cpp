// Host check of the curl members of class perlin (host/perlin.h) and class PerlinNoise (host/PerlinNoise.hpp) against the
// C ABI (include/wnoise_perlin_curl.h):
//  (1) noise_curl(x, y, z, v) / noise_curl(point3, v) -- evaluated on the host -- and the batched noise_curl(xyz, n, out3)
//      in double and float have the bits of wn_perlin_curl_points / _points_vec3, with explicit and default offsets;
//  (2) turb_curl, scalar and batched, has the bits of wn_perlin_curl_points_vec3 with WN_PERLIN_CURL_TURB (depths 0, 1, 7,
//      12);
//  (3) fractal_noise_curl likewise with WN_PERLIN_CURL_FRACTAL;
//  (4) PerlinNoise::noise_curl, scalar and batched, against wn_perlin_curl_points.
// Test infrastructure: built by tests/test_gpu_perlin_curl.py with g++ -ffp-contract=off against libwnoise_host.so.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "PerlinNoise.hpp"
#include "perlin.h"
#include "wnoise_perlin_curl.h"

static uint64_t bits(double d) { uint64_t b; memcpy(&b, &d, 8); return b; }

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

// The C ABI on device buffers: points uploaded, n records of three doubles back.
template <typename T, typename F>
static std::vector<double> via_abi(const std::vector<T> &pts, size_t n, F call)
{
    void *in = nullptr, *out = nullptr;
    check(wn_dev_alloc(&in, pts.size() * sizeof(T)), "wn_dev_alloc");
    check(wn_dev_alloc(&out, 3 * n * sizeof(double)), "wn_dev_alloc");
    check(wn_copy_h2d(in, pts.data(), pts.size() * sizeof(T), nullptr), "wn_copy_h2d");
    check(call(static_cast<const T *>(in), static_cast<double *>(out)), "curl entry point");
    std::vector<double> res(3 * n);
    check(wn_copy_d2h(res.data(), out, res.size() * sizeof(double), nullptr), "wn_copy_d2h");
    check(wn_stream_sync(nullptr), "wn_stream_sync");
    wn_dev_free(in);
    wn_dev_free(out);
    return res;
}

static void same(const std::vector<double> &a, const std::vector<double> &b, const char *what)
{
    for (size_t i = 0; i < a.size(); ++i) expect(bits(a[i]) == bits(b[i]), what, i / 3);
}

int main()
{
    const size_t n = 4000;
    std::mt19937 rng(31);
    std::uniform_real_distribution<double> u(-300.0, 300.0);
    std::vector<double> p64(3 * n);
    std::vector<float> p32(3 * n);
    for (size_t i = 0; i < 3 * n; ++i) {
        p64[i] = u(rng);
        p32[i] = (float)u(rng);
    }
    p64[0] = 3.0, p64[1] = -7.0, p64[2] = 11.0; // a lattice point
    p64[3] = -2.0;                               // a face
    p32[0] = 5.0f, p32[1] = -1.0f, p32[2] = 0.0f;
    p32[3] = -0.5f;
    const int off[9] = {-3, 260, 7, 511, -129, 1000, 40, 41, 42};
    const int32_t off32[9] = {-3, 260, 7, 511, -129, 1000, 40, 41, 42};
    const int32_t dflt[9] = {0, 0, 0, 85, 85, 85, 170, 170, 170};

    perlin noise(12345);
    const wn_perm *perm = noise.perm();
    std::vector<double> batched(3 * n);

    // (1) noise
    const std::vector<double> abi64 = via_abi(p64, n, [&](const double *in, double *out) { return wn_perlin_curl_points(perm, in, n, off32, out, nullptr); });
    const std::vector<double> abi32 = via_abi(p32, n, [&](const float *in, double *out) { return wn_perlin_curl_points_vec3(perm, in, n, WN_PERLIN_CURL_NOISE, 0, off32, out, nullptr); });
    const std::vector<double> abi64d = via_abi(p64, n, [&](const double *in, double *out) { return wn_perlin_curl_points(perm, in, n, dflt, out, nullptr); });
    noise.noise_curl(p64.data(), n, batched.data(), off);
    same(batched, abi64, "noise_curl batched (double)");
    noise.noise_curl(p32.data(), n, batched.data(), off);
    same(batched, abi32, "noise_curl batched (float)");
    noise.noise_curl(p64.data(), n, batched.data());
    same(batched, abi64d, "noise_curl batched (double, default offsets)");
    for (size_t i = 0; i < n; ++i) {
        double v[3];
        noise.noise_curl(p64[3 * i], p64[3 * i + 1], p64[3 * i + 2], v, off);
        for (int c = 0; c < 3; ++c) expect(bits(v[c]) == bits(abi64[3 * i + c]), "noise_curl", i);
        noise.noise_curl(p64[3 * i], p64[3 * i + 1], p64[3 * i + 2], v);
        for (int c = 0; c < 3; ++c) expect(bits(v[c]) == bits(abi64d[3 * i + c]), "noise_curl (default offsets)", i);
        const point3 q(p32[3 * i], p32[3 * i + 1], p32[3 * i + 2]);
        noise.noise_curl(q, v, off);
        for (int c = 0; c < 3; ++c) expect(bits(v[c]) == bits(abi32[3 * i + c]), "noise_curl(point3)", i);
    }

    // (2) turb
    for (int depth : {0, 1, 7, 12}) {
        const std::vector<double> abi = via_abi(p32, n, [&](const float *in, double *out) { return wn_perlin_curl_points_vec3(perm, in, n, WN_PERLIN_CURL_TURB, depth, off32, out, nullptr); });
        noise.turb_curl(p32.data(), n, batched.data(), depth, off);
        same(batched, abi, "turb_curl batched");
        for (size_t i = 0; i < n; ++i) {
            double v[3];
            const point3 q(p32[3 * i], p32[3 * i + 1], p32[3 * i + 2]);
            noise.turb_curl(q, v, depth, off);
            for (int c = 0; c < 3; ++c) expect(bits(v[c]) == bits(abi[3 * i + c]), "turb_curl", i);
        }
    }

    // (3) fractal_noise
    {
        const std::vector<double> abi = via_abi(p32, n, [&](const float *in, double *out) { return wn_perlin_curl_points_vec3(perm, in, n, WN_PERLIN_CURL_FRACTAL, 0, off32, out, nullptr); });
        noise.fractal_noise_curl(p32.data(), n, batched.data(), off);
        same(batched, abi, "fractal_noise_curl batched");
        for (size_t i = 0; i < n; ++i) {
            double v[3];
            const point3 q(p32[3 * i], p32[3 * i + 1], p32[3 * i + 2]);
            noise.fractal_noise_curl(q, v, off);
            for (int c = 0; c < 3; ++c) expect(bits(v[c]) == bits(abi[3 * i + c]), "fractal_noise_curl", i);
        }
    }

    // (4) PerlinNoise (the same table for the same seed)
    {
        PerlinNoise pn(12345);
        pn.noise_curl(p64.data(), n, batched.data(), off);
        same(batched, abi64, "PerlinNoise::noise_curl batched");
        for (size_t i = 0; i < n; ++i) {
            double v[3];
            pn.noise_curl(p64[3 * i], p64[3 * i + 1], p64[3 * i + 2], v, off);
            for (int c = 0; c < 3; ++c) expect(bits(v[c]) == bits(abi64[3 * i + c]), "PerlinNoise::noise_curl", i);
            pn.noise_curl(p64[3 * i], p64[3 * i + 1], p64[3 * i + 2], v);
            for (int c = 0; c < 3; ++c) expect(bits(v[c]) == bits(abi64d[3 * i + c]), "PerlinNoise::noise_curl (default offsets)", i);
        }
    }
    printf("points %zu, mismatches %ld\n", n, mismatches);
    return mismatches ? 1 : 0;
}
