// Host check of the surface gradient members of class WaveletNoise (host/WaveletNoise.h) against the C ABI
// (include/wnoise.h):
//  (1) evaluate2DGradient(p, grad) -- evaluated on the host -- and the batched evaluate2DGradient(xy, n, out3) have the
//      bits of wn_eval2d_grad_points, and the value those of evaluate2D(p);
//  (2) evaluate3DProjectedGradient, scalar (on the host) and batched, has the bits of wn_eval3d_projected_grad_points
//      and its value those of evaluate3DProjected;
//  (3) WMultibandNoiseGradient with a normal, scalar (a batch of one on the device) and batched (one normal for all
//      points), has the bits of wn_multiband3d_projected_grad_points and its value those of WMultibandNoise(p, s,
//      normal, ...); with normal == nullptr it is the normal == NULL overload.
// Test infrastructure: built by tests/test_gpu_grad_surface.py with g++ -ffp-contract=off against libwnoise_host.so.
#include <cmath>
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

// The C ABI on device buffers: inputs uploaded, n records of `width` floats back.
template <typename F>
static std::vector<float> via_abi(const std::vector<float> &a, const std::vector<float> &b, size_t n, int width, F call)
{
    void *in = nullptr, *in2 = nullptr, *out = nullptr;
    check(wn_dev_alloc(&in, a.size() * sizeof(float)), "wn_dev_alloc");
    check(wn_dev_alloc(&in2, (b.empty() ? 1 : b.size()) * sizeof(float)), "wn_dev_alloc");
    check(wn_dev_alloc(&out, width * n * sizeof(float)), "wn_dev_alloc");
    check(wn_copy_h2d(in, a.data(), a.size() * sizeof(float), nullptr), "wn_copy_h2d");
    if (!b.empty()) check(wn_copy_h2d(in2, b.data(), b.size() * sizeof(float), nullptr), "wn_copy_h2d");
    check(call(static_cast<const float *>(in), static_cast<const float *>(in2), static_cast<float *>(out)), "gradient entry point");
    std::vector<float> res(width * n);
    check(wn_copy_d2h(res.data(), out, res.size() * sizeof(float), nullptr), "wn_copy_d2h");
    check(wn_stream_sync(nullptr), "wn_stream_sync");
    wn_dev_free(in);
    wn_dev_free(in2);
    wn_dev_free(out);
    return res;
}

int main()
{
    const size_t n = 2000;
    std::mt19937 rng(23);
    std::uniform_real_distribution<float> u(-300.0f, 300.0f), un(-1.0f, 1.0f);

    // (1) evaluate2DGradient
    WaveletNoise noise2(128, 12345);
    noise2.generateNoiseTile2D();
    std::vector<float> xy(2 * n);
    for (auto &v : xy) v = u(rng);
    xy[0] = 0.5f; // a knot on both axes
    xy[1] = -2.5f;
    const wn_tile *t2 = noise2.tile(2);
    const std::vector<float> abi2 = via_abi(xy, {}, n, 3, [&](const float *in, const float *, float *out) {
        return wn_eval2d_grad_points(t2, in, n, out, nullptr);
    });
    std::vector<float> batched2(3 * n);
    noise2.evaluate2DGradient(xy.data(), n, batched2.data());
    for (size_t i = 0; i < n; ++i) {
        float g[2];
        const float v = noise2.evaluate2DGradient(&xy[2 * i], g);
        expect(bits(v) == bits(abi2[3 * i]) && bits(v) == bits(noise2.evaluate2D(&xy[2 * i])), "evaluate2DGradient value", i);
        for (int c = 0; c < 2; ++c) expect(bits(g[c]) == bits(abi2[3 * i + 1 + c]), "evaluate2DGradient gradient", i);
        for (int c = 0; c < 3; ++c) expect(bits(batched2[3 * i + c]) == bits(abi2[3 * i + c]), "evaluate2DGradient batched", i);
    }

    // (2) evaluate3DProjectedGradient: one random unit normal per point
    WaveletNoise noise(128, 12345);
    noise.generateNoiseTile3D();
    std::vector<float> xyz(3 * n), nrm(3 * n);
    for (auto &v : xyz) v = u(rng);
    for (size_t i = 0; i < n; ++i) {
        float a = un(rng), b = un(rng), c = un(rng);
        const float l = std::sqrt(a * a + b * b + c * c) + 1e-3f;
        nrm[3 * i] = a / l;
        nrm[3 * i + 1] = b / l;
        nrm[3 * i + 2] = c / l;
    }
    const wn_tile *t3 = noise.tile(3);
    const std::vector<float> abi = via_abi(xyz, nrm, n, 4, [&](const float *in, const float *nr, float *out) {
        return wn_eval3d_projected_grad_points(t3, in, nr, n, out, nullptr);
    });
    std::vector<float> batched(4 * n);
    noise.evaluate3DProjectedGradient(xyz.data(), nrm.data(), n, batched.data());
    for (size_t i = 0; i < n; ++i) {
        float g[3];
        const float v = noise.evaluate3DProjectedGradient(&xyz[3 * i], &nrm[3 * i], g);
        expect(bits(v) == bits(abi[4 * i]) && bits(v) == bits(noise.evaluate3DProjected(&xyz[3 * i], &nrm[3 * i])),
               "evaluate3DProjectedGradient value", i);
        for (int c = 0; c < 3; ++c) expect(bits(g[c]) == bits(abi[4 * i + 1 + c]), "evaluate3DProjectedGradient gradient", i);
        for (int c = 0; c < 4; ++c) expect(bits(batched[4 * i + c]) == bits(abi[4 * i + c]), "evaluate3DProjectedGradient batched", i);
    }

    // (3) WMultibandNoiseGradient with one normal for all points: five bands from first band -1, unequal weights
    const float w[5] = {1.0f, 0.5f, 2.0f, 1.0f, 0.25f};
    const float one[3] = {0.6f, 0.0f, 0.8f};
    const std::vector<float> onev(one, one + 3);
    const std::vector<float> mabi = via_abi(xyz, onev, n, 4, [&](const float *in, const float *nr, float *out) {
        return wn_multiband3d_projected_grad_points(t3, in, nr, 1, n, -16.0f, -1, 5, w, 0.296f, out, nullptr);
    });
    std::vector<float> mbatched(4 * n);
    noise.WMultibandNoiseGradient(xyz.data(), one, true, n, -16.0f, -1, 5, w, 0.296f, mbatched.data());
    for (size_t i = 0; i < n; ++i) {
        for (int c = 0; c < 4; ++c) expect(bits(mbatched[4 * i + c]) == bits(mabi[4 * i + c]), "WMultibandNoiseGradient batched", i);
        if (i % 20) continue; // the scalar member is a launch each: a sample
        float g[3];
        const float v = noise.WMultibandNoiseGradient(&xyz[3 * i], -16.0f, one, -1, 5, w, g);
        expect(bits(v) == bits(mabi[4 * i]) && bits(v) == bits(noise.WMultibandNoise(&xyz[3 * i], -16.0f, one, -1, 5, w)),
               "WMultibandNoiseGradient value", i);
        for (int c = 0; c < 3; ++c) expect(bits(g[c]) == bits(mabi[4 * i + 1 + c]), "WMultibandNoiseGradient gradient", i);
        // normal == nullptr: the normal == NULL overload
        float g0[3], g1[3];
        const float v0 = noise.WMultibandNoiseGradient(&xyz[3 * i], -16.0f, nullptr, -1, 5, w, g0, 0.18402f);
        const float v1 = noise.WMultibandNoiseGradient(&xyz[3 * i], -16.0f, -1, 5, w, g1);
        expect(bits(v0) == bits(v1), "WMultibandNoiseGradient(nullptr) value", i);
        for (int c = 0; c < 3; ++c) expect(bits(g0[c]) == bits(g1[c]), "WMultibandNoiseGradient(nullptr) gradient", i);
    }
    printf("points %zu, mismatches %ld\n", n, mismatches);
    return mismatches ? 1 : 0;
}
