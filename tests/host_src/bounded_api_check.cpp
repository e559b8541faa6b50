// Host check of the boundary members of class WaveletNoise (host/WaveletNoise.h) against the C ABI
// (include/wnoise_bounded.h):
//  (1) evaluate3DCurlBounded(p, offsets, obs, nobs, v) -- evaluated on the host -- and the batched form have the bits of
//      wn_eval3d_curl_bounded_points, with explicit offsets and with the default ones (offsets == nullptr); with nobs == 0
//      those of evaluate3DCurl;
//  (2) advectCurlBounded, scalar (traced on the host) and batched, has the bits of wn_eval3d_curl_bounded_advect_points,
//      final positions and trajectory, for the three methods, and in place;
//  (3) WMultibandNoiseCurlBounded and WMultibandNoiseAdvectCurlBounded, scalar (a batch of one) and batched, have the bits of
//      wn_multiband3d_curl_bounded_points / _advect_points;
//  (4) an obstacle list the ABI refuses makes the members throw.
// Test infrastructure: built by tests/test_gpu_bounded.py with g++ -ffp-contract=off against libwnoise_host.so.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <stdexcept>
#include <vector>

#include "WaveletNoise.h"
#include "wnoise_bounded.h"

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

// The C ABI on device buffers: n output triples and `snaps` snapshots of n positions.
template <typename F>
static Traced via_abi(const std::vector<float> &xyz, size_t n, size_t snaps, F call)
{
    void *in = nullptr, *out = nullptr, *traj = nullptr;
    check(wn_dev_alloc(&in, 3 * n * sizeof(float)), "wn_dev_alloc");
    check(wn_dev_alloc(&out, 3 * n * sizeof(float)), "wn_dev_alloc");
    check(wn_dev_alloc(&traj, (snaps ? snaps : 1) * 3 * n * sizeof(float)), "wn_dev_alloc");
    check(wn_copy_h2d(in, xyz.data(), 3 * n * sizeof(float), nullptr), "wn_copy_h2d");
    check(call(static_cast<const float *>(in), static_cast<float *>(out), static_cast<float *>(traj)), "bounded entry point");
    Traced r{std::vector<float>(3 * n), std::vector<float>(snaps * 3 * n)};
    check(wn_copy_d2h(r.out.data(), out, r.out.size() * sizeof(float), nullptr), "wn_copy_d2h");
    if (snaps) check(wn_copy_d2h(r.traj.data(), traj, r.traj.size() * sizeof(float), nullptr), "wn_copy_d2h");
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
    // a sphere, a ground plane and a container whose ramps overlap
    const wn_obstacle obs[3] = {{WN_OBSTACLE_SPHERE, {0.0f, 0.0f, 0.0f}, 120.0f, 80.0f, {0, 0}},
                                {WN_OBSTACLE_HALFSPACE, {0.0f, 1.0f, 0.0f}, -250.0f, 100.0f, {0, 0}},
                                {WN_OBSTACLE_CONTAINER, {0.0f, 0.0f, 0.0f}, 500.0f, 150.0f, {0, 0}}};

    // (1) evaluate3DCurlBounded
    size_t differs = 0;
    for (int pass = 0; pass < 2; ++pass) {
        const int *member_off = pass == 0 ? mixed : nullptr;
        const int *abi_off = pass == 0 ? mixed : def;
        const Traced abi = via_abi(xyz, n, 0, [&](const float *in, float *out, float *) {
            return wn_eval3d_curl_bounded_points(t, in, n, abi_off, obs, 3, out, nullptr);
        });
        std::vector<float> batched(3 * n), free_field(3 * n), none(3 * n);
        noise.evaluate3DCurlBounded(xyz.data(), n, member_off, obs, 3, batched.data());
        expect_equal(batched, abi.out, "evaluate3DCurlBounded batched");
        noise.evaluate3DCurl(xyz.data(), n, member_off, free_field.data());
        noise.evaluate3DCurlBounded(xyz.data(), n, member_off, nullptr, 0, none.data());
        expect_equal(none, free_field, "evaluate3DCurlBounded without obstacles");
        for (size_t i = 0; i < n; ++i) {
            float v[3];
            noise.evaluate3DCurlBounded(&xyz[3 * i], member_off, obs, 3, v);
            for (int c = 0; c < 3; ++c) {
                expect(bits(v[c]) == bits(abi.out[3 * i + c]), "evaluate3DCurlBounded scalar", i);
                differs += bits(v[c]) != bits(free_field[3 * i + c]);
            }
        }
    }
    expect(differs > n, "the obstacles change the field", differs);

    // (2) advectCurlBounded: five steps (more than one launch), a snapshot every second step
    for (int method = WN_ADVECT_EULER; method <= WN_ADVECT_RK4; ++method) {
        const wn_advect a = {method, 5, 0.37f, 0.75f, {0.1f, -0.2f, 0.05f}, 2};
        const size_t snaps = 5 / 2 + 1;
        const Traced abi = via_abi(xyz, n, snaps, [&](const float *in, float *out, float *traj) {
            return wn_eval3d_curl_bounded_advect_points(t, in, n, mixed, obs, 3, &a, out, traj, nullptr);
        });
        Traced batched{std::vector<float>(3 * n), std::vector<float>(snaps * 3 * n)};
        noise.advectCurlBounded(xyz.data(), n, a, mixed, obs, 3, batched.out.data(), batched.traj.data());
        expect_equal(batched.out, abi.out, "advectCurlBounded batched");
        expect_equal(batched.traj, abi.traj, "advectCurlBounded batched trajectory");
        for (size_t i = 0; i < n; ++i) {
            float p[3], path[3 * 3];
            noise.advectCurlBounded(&xyz[3 * i], a, mixed, obs, 3, p, path);
            for (int c = 0; c < 3; ++c) {
                expect(bits(p[c]) == bits(abi.out[3 * i + c]), "advectCurlBounded scalar", i);
                for (size_t s = 0; s < snaps; ++s)
                    expect(bits(path[3 * s + c]) == bits(abi.traj[(s * n + i) * 3 + c]), "advectCurlBounded scalar trajectory", i);
            }
        }
        wn_advect plain = a;
        plain.traj_every = 0;
        std::vector<float> moved = xyz;
        noise.advectCurlBounded(moved.data(), n, plain, mixed, obs, 3, moved.data());
        expect_equal(moved, abi.out, "advectCurlBounded in place");
    }

    // (3) the multiband members: five bands from first band -1, unequal weights
    const float w[5] = {1.0f, 0.5f, 2.0f, 1.0f, 0.25f};
    const Traced pabi = via_abi(xyz, n, 0, [&](const float *in, float *out, float *) {
        return wn_multiband3d_curl_bounded_points(t, in, n, mixed, -16.0f, -1, 5, w, 0.18402f, obs, 3, out, nullptr);
    });
    std::vector<float> mbp(3 * n);
    noise.WMultibandNoiseCurlBounded(xyz.data(), n, mixed, obs, 3, -16.0f, -1, 5, w, 0.18402f, mbp.data());
    expect_equal(mbp, pabi.out, "WMultibandNoiseCurlBounded batched");
    const wn_advect am = {WN_ADVECT_RK4, 4, -0.02f, 1.0f, {0.0f, 0.0f, 0.0f}, 1};
    const Traced mabi = via_abi(xyz, n, 5, [&](const float *in, float *out, float *traj) {
        return wn_multiband3d_curl_bounded_advect_points(t, in, n, mixed, -16.0f, -1, 5, w, 0.18402f, obs, 3, &am, out, traj,
                                                         nullptr);
    });
    Traced mb{std::vector<float>(3 * n), std::vector<float>(5 * 3 * n)};
    noise.WMultibandNoiseAdvectCurlBounded(xyz.data(), n, am, mixed, obs, 3, -16.0f, -1, 5, w, 0.18402f, mb.out.data(),
                                           mb.traj.data());
    expect_equal(mb.out, mabi.out, "WMultibandNoiseAdvectCurlBounded batched");
    expect_equal(mb.traj, mabi.traj, "WMultibandNoiseAdvectCurlBounded batched trajectory");
    for (size_t i = 0; i < n; i += 50) { // the scalar members are a batch of one each: a sample
        float v[3], p[3], path[5 * 3];
        noise.WMultibandNoiseCurlBounded(&xyz[3 * i], mixed, obs, 3, -16.0f, -1, 5, w, v);
        noise.WMultibandNoiseAdvectCurlBounded(&xyz[3 * i], am, mixed, obs, 3, -16.0f, -1, 5, w, p, path);
        for (int c = 0; c < 3; ++c) {
            expect(bits(v[c]) == bits(pabi.out[3 * i + c]), "WMultibandNoiseCurlBounded scalar", i);
            expect(bits(p[c]) == bits(mabi.out[3 * i + c]), "WMultibandNoiseAdvectCurlBounded scalar", i);
            for (size_t s = 0; s < 5; ++s)
                expect(bits(path[3 * s + c]) == bits(mabi.traj[(s * n + i) * 3 + c]),
                       "WMultibandNoiseAdvectCurlBounded scalar trajectory", i);
        }
    }

    // (4) refused obstacle lists throw
    const wn_obstacle bad[1] = {{WN_OBSTACLE_SPHERE, {0.0f, 0.0f, 0.0f}, 1.0f, 0.0f, {0, 0}}}; // d0 == 0
    const wn_advect a1 = {WN_ADVECT_RK4, 1, 0.1f, 1.0f, {0.0f, 0.0f, 0.0f}, 0};
    float p[3];
    int thrown = 0;
    try { noise.evaluate3DCurlBounded(xyz.data(), mixed, bad, 1, p); } catch (const std::runtime_error &) { ++thrown; }
    try { noise.evaluate3DCurlBounded(xyz.data(), 4, mixed, bad, 1, mbp.data()); } catch (const std::runtime_error &) { ++thrown; }
    try { noise.evaluate3DCurlBounded(xyz.data(), 4, mixed, obs, 17, mbp.data()); } catch (const std::runtime_error &) { ++thrown; }
    try { noise.WMultibandNoiseCurlBounded(xyz.data(), mixed, bad, 1, -16.0f, -1, 5, w, p); } catch (const std::runtime_error &) { ++thrown; }
    try { noise.advectCurlBounded(xyz.data(), a1, mixed, bad, 1, p); } catch (const std::runtime_error &) { ++thrown; }
    try { noise.advectCurlBounded(xyz.data(), 4, a1, mixed, bad, 1, mbp.data()); } catch (const std::runtime_error &) { ++thrown; }
    try { noise.WMultibandNoiseAdvectCurlBounded(xyz.data(), a1, mixed, bad, 1, -16.0f, -1, 5, w, p); } catch (const std::runtime_error &) { ++thrown; }
    expect(thrown == 7, "refused obstacle lists throw", (size_t)thrown);

    printf("points %zu, mismatches %ld\n", n, mismatches);
    return mismatches ? 1 : 0;
}
