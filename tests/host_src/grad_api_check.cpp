// Host check of the gradient members of class WaveletNoise (host/WaveletNoise.h) against the C ABI (include/wnoise.h):
//  (1) evaluate3DGradient(p, grad) -- evaluated on the host -- and the batched evaluate3DGradient(xyz, n, out4) have the
//      bits of wn_eval3d_grad_points, and the value those of evaluate3D(p);
//  (2) WMultibandNoiseGradient, scalar (a batch of one on the device) and batched, has the bits of
//      wn_multiband3d_grad_points and its value those of WMultibandNoise.
// Test infrastructure: built by tests/test_gpu_gradient.py with g++ -ffp-contract=off against libwnoise_host.so.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "WaveletNoise.h"
#include "wnoise.h"

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

// The C ABI on device buffers: n records of 4 floats.
template <typename F>
static std::vector<float> via_abi(const std::vector<float> &xyz, size_t n, F call)
{
    void *in = nullptr, *out = nullptr;
    check(wn_dev_alloc(&in, xyz.size() * sizeof(float)), "wn_dev_alloc");
    check(wn_dev_alloc(&out, 4 * n * sizeof(float)), "wn_dev_alloc");
    check(wn_copy_h2d(in, xyz.data(), xyz.size() * sizeof(float), nullptr), "wn_copy_h2d");
    check(call(static_cast<const float *>(in), static_cast<float *>(out)), "gradient entry point");
    std::vector<float> res(4 * n);
    check(wn_copy_d2h(res.data(), out, res.size() * sizeof(float), nullptr), "wn_copy_d2h");
    check(wn_stream_sync(nullptr), "wn_stream_sync");
    wn_dev_free(in);
    wn_dev_free(out);
    return res;
}

int main()
{
    WaveletNoise noise(128, 12345);
    noise.generateNoiseTile3D();
    const size_t n = 3000;
    std::mt19937 rng(17);
    std::uniform_real_distribution<float> u(-300.0f, 300.0f);
    std::vector<float> xyz(3 * n);
    for (auto &v : xyz) v = u(rng);
    xyz[0] = 0.5f; // a knot on every axis
    xyz[1] = -2.5f;
    xyz[2] = 127.5f;

    // (1) evaluate3DGradient
    const wn_tile *t = noise.tile(3);
    const std::vector<float> abi = via_abi(xyz, n, [&](const float *in, float *out) {
        return wn_eval3d_grad_points(t, in, n, out, nullptr);
    });
    std::vector<float> batched(4 * n);
    noise.evaluate3DGradient(xyz.data(), n, batched.data());
    for (size_t i = 0; i < n; ++i) {
        float g[3];
        const float v = noise.evaluate3DGradient(&xyz[3 * i], g);
        expect(bits(v) == bits(abi[4 * i]) && bits(v) == bits(noise.evaluate3D(&xyz[3 * i])), "evaluate3DGradient value", i);
        for (int c = 0; c < 3; ++c) expect(bits(g[c]) == bits(abi[4 * i + 1 + c]), "evaluate3DGradient gradient", i);
        for (int c = 0; c < 4; ++c) expect(bits(batched[4 * i + c]) == bits(abi[4 * i + c]), "evaluate3DGradient batched", i);
    }

    // (2) WMultibandNoiseGradient: five bands from first band -1, unequal weights
    const float w[5] = {1.0f, 0.5f, 2.0f, 1.0f, 0.25f};
    const std::vector<float> mabi = via_abi(xyz, n, [&](const float *in, float *out) {
        return wn_multiband3d_grad_points(t, in, n, -16.0f, -1, 5, w, 0.18402f, out, nullptr);
    });
    std::vector<float> mbatched(4 * n);
    noise.WMultibandNoiseGradient(xyz.data(), n, -16.0f, -1, 5, w, 0.18402f, mbatched.data());
    for (size_t i = 0; i < n; ++i) {
        for (int c = 0; c < 4; ++c) expect(bits(mbatched[4 * i + c]) == bits(mabi[4 * i + c]), "WMultibandNoiseGradient batched", i);
        if (i % 10) continue; // the scalar member is a launch each: a sample
        float g[3];
        const float v = noise.WMultibandNoiseGradient(&xyz[3 * i], -16.0f, -1, 5, w, g);
        expect(bits(v) == bits(mabi[4 * i]) && bits(v) == bits(noise.WMultibandNoise(&xyz[3 * i], -16.0f, -1, 5, w)),
               "WMultibandNoiseGradient value", i);
        for (int c = 0; c < 3; ++c) expect(bits(g[c]) == bits(mabi[4 * i + 1 + c]), "WMultibandNoiseGradient gradient", i);
    }
    printf("points %zu, mismatches %ld\n", n, mismatches);
    return mismatches ? 1 : 0;
}
