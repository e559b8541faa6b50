// Host check of the curl members of class WaveletNoise (host/WaveletNoise.h) against the C ABI (include/wnoise.h):
//  (1) evaluate3DCurl(p, offsets, v) -- evaluated on the host -- and the batched evaluate3DCurl(xyz, n, offsets, out3) have
//      the bits of wn_eval3d_curl_points, with explicit offsets and with the default ones (offsets == nullptr);
//  (2) WMultibandNoiseCurl, scalar (a batch of one on the device) and batched, has the bits of wn_multiband3d_curl_points.
// Test infrastructure: built by tests/test_gpu_curl.py with g++ -ffp-contract=off against libwnoise_host.so.
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

// The C ABI on device buffers: n records of 3 floats.
template <typename F>
static std::vector<float> via_abi(const std::vector<float> &xyz, size_t n, F call)
{
    void *in = nullptr, *out = nullptr;
    check(wn_dev_alloc(&in, xyz.size() * sizeof(float)), "wn_dev_alloc");
    check(wn_dev_alloc(&out, 3 * n * sizeof(float)), "wn_dev_alloc");
    check(wn_copy_h2d(in, xyz.data(), xyz.size() * sizeof(float), nullptr), "wn_copy_h2d");
    check(call(static_cast<const float *>(in), static_cast<float *>(out)), "curl entry point");
    std::vector<float> res(3 * n);
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
    const wn_tile *t = noise.tile(3);
    const int mixed[9] = {0, 0, 0, 1, 2, 3, -5, 7, 130};
    int def[9];
    noise.defaultCurlOffsets(def);
    const int want_def[9] = {0, 0, 0, 42, 42, 42, 85, 85, 85};
    for (int i = 0; i < 9; ++i) expect(def[i] == want_def[i], "defaultCurlOffsets", i);

    // (1) evaluate3DCurl: explicit offsets, then nullptr against the default ones through the ABI
    for (int pass = 0; pass < 2; ++pass) {
        const int *member_off = pass == 0 ? mixed : nullptr;
        const int *abi_off = pass == 0 ? mixed : def;
        const std::vector<float> abi = via_abi(xyz, n, [&](const float *in, float *out) {
            return wn_eval3d_curl_points(t, in, n, abi_off, out, nullptr);
        });
        std::vector<float> batched(3 * n);
        noise.evaluate3DCurl(xyz.data(), n, member_off, batched.data());
        for (size_t i = 0; i < n; ++i) {
            float v[3];
            noise.evaluate3DCurl(&xyz[3 * i], member_off, v);
            for (int c = 0; c < 3; ++c) {
                expect(bits(v[c]) == bits(abi[3 * i + c]), "evaluate3DCurl scalar", i);
                expect(bits(batched[3 * i + c]) == bits(abi[3 * i + c]), "evaluate3DCurl batched", i);
            }
        }
    }

    // (2) WMultibandNoiseCurl: five bands from first band -1, unequal weights
    const float w[5] = {1.0f, 0.5f, 2.0f, 1.0f, 0.25f};
    const std::vector<float> mabi = via_abi(xyz, n, [&](const float *in, float *out) {
        return wn_multiband3d_curl_points(t, in, n, mixed, -16.0f, -1, 5, w, 0.18402f, out, nullptr);
    });
    std::vector<float> mbatched(3 * n);
    noise.WMultibandNoiseCurl(xyz.data(), n, mixed, -16.0f, -1, 5, w, 0.18402f, mbatched.data());
    for (size_t i = 0; i < n; ++i) {
        for (int c = 0; c < 3; ++c) expect(bits(mbatched[3 * i + c]) == bits(mabi[3 * i + c]), "WMultibandNoiseCurl batched", i);
        if (i % 10) continue; // the scalar member is a launch each: a sample
        float v[3];
        noise.WMultibandNoiseCurl(&xyz[3 * i], mixed, -16.0f, -1, 5, w, v);
        for (int c = 0; c < 3; ++c) expect(bits(v[c]) == bits(mabi[3 * i + c]), "WMultibandNoiseCurl scalar", i);
    }
    printf("points %zu, mismatches %ld\n", n, mismatches);
    return mismatches ? 1 : 0;
}
