// Host check of the gradient members of class perlin (host/perlin.h) and class PerlinNoise (host/PerlinNoise.hpp)
// against the C ABI (include/wnoise.h):
//  (1) noise_gradient(x, y, z, grad) / noise_gradient(point3, grad) -- evaluated on the host -- and the batched
//      noise_gradient(xyz, n, out4) in double and float have the bits of wn_perlin_grad_points / _points_vec3, and the
//      value those of noise();
//  (2) turb_gradient, scalar and batched, has the bits of wn_perlin_turb_grad_points (depths 0, 1, 7, 12) and its value
//      those of turb();
//  (3) fractal_noise_gradient likewise against wn_perlin_fractal_grad_points and fractal_noise();
//  (4) PerlinNoise::noise_gradient, scalar and batched, against wn_perlin_grad_points.
// Test infrastructure: built by tests/test_gpu_perlin_grad.py with g++ -ffp-contract=off against libwnoise_host.so.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "PerlinNoise.hpp"
#include "perlin.h"
#include "wnoise.h"

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

// The C ABI on device buffers: points uploaded, n records of four doubles back.
template <typename T, typename F>
static std::vector<double> via_abi(const std::vector<T> &pts, size_t n, F call)
{
    void *in = nullptr, *out = nullptr;
    check(wn_dev_alloc(&in, pts.size() * sizeof(T)), "wn_dev_alloc");
    check(wn_dev_alloc(&out, 4 * n * sizeof(double)), "wn_dev_alloc");
    check(wn_copy_h2d(in, pts.data(), pts.size() * sizeof(T), nullptr), "wn_copy_h2d");
    check(call(static_cast<const T *>(in), static_cast<double *>(out)), "gradient entry point");
    std::vector<double> res(4 * n);
    check(wn_copy_d2h(res.data(), out, res.size() * sizeof(double), nullptr), "wn_copy_d2h");
    check(wn_stream_sync(nullptr), "wn_stream_sync");
    wn_dev_free(in);
    wn_dev_free(out);
    return res;
}

static void same(const std::vector<double> &a, const std::vector<double> &b, const char *what)
{
    for (size_t i = 0; i < a.size(); ++i) expect(bits(a[i]) == bits(b[i]), what, i / 4);
}

int main()
{
    const size_t n = 4000;
    std::mt19937 rng(29);
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

    perlin noise(12345);
    const wn_perm *perm = noise.perm();

    // (1) noise
    const std::vector<double> abi64 = via_abi(p64, n, [&](const double *in, double *out) { return wn_perlin_grad_points(perm, in, n, out, nullptr); });
    const std::vector<double> abi32 = via_abi(p32, n, [&](const float *in, double *out) { return wn_perlin_grad_points_vec3(perm, in, n, out, nullptr); });
    std::vector<double> batched(4 * n);
    noise.noise_gradient(p64.data(), n, batched.data());
    same(batched, abi64, "noise_gradient batched (double)");
    noise.noise_gradient(p32.data(), n, batched.data());
    same(batched, abi32, "noise_gradient batched (float)");
    for (size_t i = 0; i < n; ++i) {
        double g[3];
        const double v = noise.noise_gradient(p64[3 * i], p64[3 * i + 1], p64[3 * i + 2], g);
        expect(bits(v) == bits(abi64[4 * i]) && bits(v) == bits(noise.noise(p64[3 * i], p64[3 * i + 1], p64[3 * i + 2])), "noise_gradient value", i);
        for (int c = 0; c < 3; ++c) expect(bits(g[c]) == bits(abi64[4 * i + 1 + c]), "noise_gradient gradient", i);
        const point3 q(p32[3 * i], p32[3 * i + 1], p32[3 * i + 2]);
        const double vq = noise.noise_gradient(q, g);
        expect(bits(vq) == bits(abi32[4 * i]) && bits(vq) == bits(noise.noise(q)), "noise_gradient(point3) value", i);
        for (int c = 0; c < 3; ++c) expect(bits(g[c]) == bits(abi32[4 * i + 1 + c]), "noise_gradient(point3) gradient", i);
    }

    // (2) turb
    for (int depth : {0, 1, 7, 12}) {
        const std::vector<double> abi = via_abi(p32, n, [&](const float *in, double *out) { return wn_perlin_turb_grad_points(perm, in, n, depth, out, nullptr); });
        noise.turb_gradient(p32.data(), n, batched.data(), depth);
        same(batched, abi, "turb_gradient batched");
        for (size_t i = 0; i < n; ++i) {
            double g[3];
            const point3 q(p32[3 * i], p32[3 * i + 1], p32[3 * i + 2]);
            const double v = noise.turb_gradient(q, g, depth);
            expect(bits(v) == bits(abi[4 * i]) && bits(v) == bits(noise.turb(q, depth)), "turb_gradient value", i);
            for (int c = 0; c < 3; ++c) expect(bits(g[c]) == bits(abi[4 * i + 1 + c]), "turb_gradient gradient", i);
        }
    }

    // (3) fractal_noise
    {
        const std::vector<double> abi = via_abi(p32, n, [&](const float *in, double *out) { return wn_perlin_fractal_grad_points(perm, in, n, out, nullptr); });
        noise.fractal_noise_gradient(p32.data(), n, batched.data());
        same(batched, abi, "fractal_noise_gradient batched");
        for (size_t i = 0; i < n; ++i) {
            double g[3];
            const point3 q(p32[3 * i], p32[3 * i + 1], p32[3 * i + 2]);
            const double v = noise.fractal_noise_gradient(q, g);
            expect(bits(v) == bits(abi[4 * i]) && bits(v) == bits(noise.fractal_noise(q)), "fractal_noise_gradient value", i);
            for (int c = 0; c < 3; ++c) expect(bits(g[c]) == bits(abi[4 * i + 1 + c]), "fractal_noise_gradient gradient", i);
        }
    }

    // (4) PerlinNoise (the same table for the same seed)
    {
        PerlinNoise pn(12345);
        pn.noise_gradient(p64.data(), n, batched.data());
        same(batched, abi64, "PerlinNoise::noise_gradient batched");
        for (size_t i = 0; i < n; ++i) {
            double g[3];
            const double v = pn.noise_gradient(p64[3 * i], p64[3 * i + 1], p64[3 * i + 2], g);
            expect(bits(v) == bits(abi64[4 * i]) && bits(v) == bits(pn.noise(p64[3 * i], p64[3 * i + 1], p64[3 * i + 2])), "PerlinNoise::noise_gradient value", i);
            for (int c = 0; c < 3; ++c) expect(bits(g[c]) == bits(abi64[4 * i + 1 + c]), "PerlinNoise::noise_gradient gradient", i);
        }
    }
    printf("points %zu, mismatches %ld\n", n, mismatches);
    return mismatches ? 1 : 0;
}
