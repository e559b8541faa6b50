// Host check of the advection members of class WaveletNoise (host/WaveletNoise.h) against the C ABI
// (include/wnoise_advect.h):
//  (1) advectCurl(p, a, offsets, p_out, traj) -- traced on the host -- and the batched advectCurl(xyz, n, a, offsets, out,
//      traj) have the bits of wn_eval3d_curl_advect_points, final positions and trajectory, for the three methods, with
//      explicit offsets and with the default ones (offsets == nullptr), and in place;
//  (2) WMultibandNoiseAdvectCurl, scalar (a batch of one) and batched, has the bits of wn_multiband3d_curl_advect_points;
//  (3) a wn_advect the ABI refuses makes the members throw.
// Test infrastructure: built by tests/test_gpu_advect.py with g++ -ffp-contract=off against libwnoise_host.so.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <stdexcept>
#include <vector>

#include "WaveletNoise.h"
#include "wnoise_advect.h"

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

struct Traced {
    std::vector<float> out, traj;
};

// The C ABI on device buffers: n final positions and `snaps` snapshots of n positions.
template <typename F>
static Traced via_abi(const std::vector<float> &xyz, size_t n, size_t snaps, F call)
{
    void *in = nullptr, *out = nullptr, *traj = nullptr;
    check(wn_dev_alloc(&in, 3 * n * sizeof(float)), "wn_dev_alloc");
    check(wn_dev_alloc(&out, 3 * n * sizeof(float)), "wn_dev_alloc");
    check(wn_dev_alloc(&traj, snaps * 3 * n * sizeof(float)), "wn_dev_alloc");
    check(wn_copy_h2d(in, xyz.data(), 3 * n * sizeof(float), nullptr), "wn_copy_h2d");
    check(call(static_cast<const float *>(in), static_cast<float *>(out), static_cast<float *>(traj)), "advect entry point");
    Traced r{std::vector<float>(3 * n), std::vector<float>(snaps * 3 * n)};
    check(wn_copy_d2h(r.out.data(), out, r.out.size() * sizeof(float), nullptr), "wn_copy_d2h");
    check(wn_copy_d2h(r.traj.data(), traj, r.traj.size() * sizeof(float), nullptr), "wn_copy_d2h");
    check(wn_stream_sync(nullptr), "wn_stream_sync");
    wn_dev_free(in);
    wn_dev_free(out);
    wn_dev_free(traj);
    return r;
}

static void expect_equal(const std::vector<float> &a, const std::vector<float> &b, const char *what)
{
    expect(a.size() == b.size(), what, 0);
    for (size_t i = 0; i < a.size() && i < b.size(); ++i) expect(bits(a[i]) == bits(b[i]), what, i);
}

int main()
{
    WaveletNoise noise(128, 12345);
    noise.generateNoiseTile3D();
    const size_t n = 1500;
    std::mt19937 rng(19);
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

    // (1) advectCurl: five steps (more than one launch), a snapshot every second step
    for (int method = WN_ADVECT_EULER; method <= WN_ADVECT_RK4; ++method)
        for (int pass = 0; pass < 2; ++pass) {
            const wn_advect a = {method, 5, pass ? -0.37f : 0.37f, 0.75f, {0.1f, -0.2f, 0.05f}, 2};
            const size_t snaps = 5 / 2 + 1;
            const int *member_off = pass == 0 ? mixed : nullptr;
            const int *abi_off = pass == 0 ? mixed : def;
            const Traced abi = via_abi(xyz, n, snaps, [&](const float *in, float *out, float *traj) {
                return wn_eval3d_curl_advect_points(t, in, n, abi_off, &a, out, traj, nullptr);
            });
            Traced batched{std::vector<float>(3 * n), std::vector<float>(snaps * 3 * n)};
            noise.advectCurl(xyz.data(), n, a, member_off, batched.out.data(), batched.traj.data());
            expect_equal(batched.out, abi.out, "advectCurl batched");
            expect_equal(batched.traj, abi.traj, "advectCurl batched trajectory");
            for (size_t i = 0; i < n; ++i) {
                float p[3], path[3 * 3];
                noise.advectCurl(&xyz[3 * i], a, member_off, p, path);
                for (int c = 0; c < 3; ++c) {
                    expect(bits(p[c]) == bits(abi.out[3 * i + c]), "advectCurl scalar", i);
                    for (size_t s = 0; s < snaps; ++s)
                        expect(bits(path[3 * s + c]) == bits(abi.traj[(s * n + i) * 3 + c]), "advectCurl scalar trajectory", i);
                }
            }
            // no trajectory, in place
            wn_advect plain = a;
            plain.traj_every = 0;
            std::vector<float> moved = xyz;
            noise.advectCurl(moved.data(), n, plain, member_off, moved.data());
            expect_equal(moved, abi.out, "advectCurl in place");
        }

    // (2) WMultibandNoiseAdvectCurl: five bands from first band -1, unequal weights
    const float w[5] = {1.0f, 0.5f, 2.0f, 1.0f, 0.25f};
    const wn_advect am = {WN_ADVECT_RK4, 4, -0.02f, 1.0f, {0.0f, 0.0f, 0.0f}, 1};
    const Traced mabi = via_abi(xyz, n, 5, [&](const float *in, float *out, float *traj) {
        return wn_multiband3d_curl_advect_points(t, in, n, mixed, -16.0f, -1, 5, w, 0.18402f, &am, out, traj, nullptr);
    });
    Traced mb{std::vector<float>(3 * n), std::vector<float>(5 * 3 * n)};
    noise.WMultibandNoiseAdvectCurl(xyz.data(), n, am, mixed, -16.0f, -1, 5, w, 0.18402f, mb.out.data(), mb.traj.data());
    expect_equal(mb.out, mabi.out, "WMultibandNoiseAdvectCurl batched");
    expect_equal(mb.traj, mabi.traj, "WMultibandNoiseAdvectCurl batched trajectory");
    for (size_t i = 0; i < n; i += 50) { // the scalar member is a batch of one each: a sample
        float p[3], path[5 * 3];
        noise.WMultibandNoiseAdvectCurl(&xyz[3 * i], am, mixed, -16.0f, -1, 5, w, p, path);
        for (int c = 0; c < 3; ++c) {
            expect(bits(p[c]) == bits(mabi.out[3 * i + c]), "WMultibandNoiseAdvectCurl scalar", i);
            for (size_t s = 0; s < 5; ++s)
                expect(bits(path[3 * s + c]) == bits(mabi.traj[(s * n + i) * 3 + c]), "WMultibandNoiseAdvectCurl scalar trajectory", i);
        }
    }

    // (3) refused arguments throw
    const wn_advect bad = {7, 1, 0.1f, 1.0f, {0.0f, 0.0f, 0.0f}, 0};
    float p[3];
    int thrown = 0;
    try { noise.advectCurl(xyz.data(), bad, mixed, p); } catch (const std::runtime_error &) { ++thrown; }
    try { noise.advectCurl(xyz.data(), 4, bad, mixed, mb.out.data()); } catch (const std::runtime_error &) { ++thrown; }
    try { noise.WMultibandNoiseAdvectCurl(xyz.data(), bad, mixed, -16.0f, -1, 5, w, p); } catch (const std::runtime_error &) { ++thrown; }
    expect(thrown == 3, "refused wn_advect throws", (size_t)thrown);

    printf("points %zu, mismatches %ld\n", n, mismatches);
    return mismatches ? 1 : 0;
}
