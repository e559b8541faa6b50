// Host check of the bounded 2-D curl members of class WaveletNoise (host/WaveletNoise.h) against the C ABI
// (include/wnoise_bounded2d.h), with a disc, a half-plane and a container and a background stream:
//  (1) WMultibandNoise2DCurlBounded(p, ...) -- evaluated on the host -- and the batched form have the bits of
//      wn_multiband2d_curl_bounded_points; without obstacles and stream those of WMultibandNoise2DCurl;
//  (2) WMultibandNoise2DAdvectCurlBounded(p, a, ...) -- traced on the host -- and the batched form have the bits of
//      wn_multiband2d_curl_bounded_advect_points, final positions and trajectory, for the three methods, and in place;
//  (3) an obstacle list, a stream or a wn_advect2d the ABI refuses makes the members throw.
// Test infrastructure: built by tests/test_gpu_bounded2d.py with g++ -ffp-contract=off against libwnoise_host.so.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <stdexcept>
#include <vector>

#include "WaveletNoise.h"
#include "wnoise_bounded2d.h"

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

// The C ABI on device buffers: `out_floats` floats and `traj_floats` more.
template <typename F>
static Traced via_abi(const std::vector<float> &xy, size_t out_floats, size_t traj_floats, F call)
{
    void *in = nullptr, *out = nullptr, *traj = nullptr;
    check(wn_dev_alloc(&in, xy.size() * sizeof(float)), "wn_dev_alloc");
    check(wn_dev_alloc(&out, out_floats * sizeof(float)), "wn_dev_alloc");
    check(wn_dev_alloc(&traj, (traj_floats ? traj_floats : 1) * sizeof(float)), "wn_dev_alloc");
    check(wn_copy_h2d(in, xy.data(), xy.size() * sizeof(float), nullptr), "wn_copy_h2d");
    check(call(static_cast<const float *>(in), static_cast<float *>(out), static_cast<float *>(traj)), "bounded2d entry point");
    Traced r{std::vector<float>(out_floats), std::vector<float>(traj_floats)};
    check(wn_copy_d2h(r.out.data(), out, out_floats * sizeof(float), nullptr), "wn_copy_d2h");
    if (traj_floats) check(wn_copy_d2h(r.traj.data(), traj, traj_floats * sizeof(float), nullptr), "wn_copy_d2h");
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
    noise.generateNoiseTile2D();
    const size_t n = 1500;
    std::mt19937 rng(19);
    std::uniform_real_distribution<float> u(-300.0f, 300.0f);
    std::vector<float> xy(2 * n);
    for (auto &v : xy) v = u(rng);
    xy[0] = 0.5f; // a knot on both axes, inside the disc
    xy[1] = -2.5f;
    const wn_tile *t = noise.tile(2);
    const float w[5] = {1.0f, 0.5f, 2.0f, 1.0f, 0.25f};
    const float s = -2.5f, variance = 0.19686f; // three of five bands run
    const int first = -1, nb = 5;
    const wn_obstacle2d obs[3] = {{WN_OBSTACLE_SPHERE, {0.0f, 0.0f}, 120.0f, 80.0f, {0, 0, 0}},
                                  {WN_OBSTACLE_HALFSPACE, {0.0f, 2.0f}, -500.0f, 200.0f, {0, 0, 0}},
                                  {WN_OBSTACLE_CONTAINER, {0.0f, 0.0f}, 500.0f, 150.0f, {0, 0, 0}}};
    const float flow[2] = {0.3f, -0.2f};

    // (1) the velocity, with and without a stream
    size_t zeros = 0, changed = 0;
    for (const float *fl : {static_cast<const float *>(nullptr), flow}) {
        const Traced vabi = via_abi(xy, 2 * n, 0, [&](const float *in, float *out, float *) {
            return wn_multiband2d_curl_bounded_points(t, in, n, s, first, nb, w, variance, obs, 3, fl, out, nullptr);
        });
        std::vector<float> batched(2 * n);
        noise.WMultibandNoise2DCurlBounded(xy.data(), n, obs, 3, fl, s, first, nb, w, variance, batched.data());
        expect_equal(batched, vabi.out, "WMultibandNoise2DCurlBounded batched");
        for (size_t i = 0; i < n; ++i) {
            float v[2], plain[2];
            noise.WMultibandNoise2DCurlBounded(&xy[2 * i], obs, 3, fl, s, first, nb, w, v);
            noise.WMultibandNoise2DCurl(&xy[2 * i], s, first, nb, w, plain);
            expect(bits(v[0]) == bits(vabi.out[2 * i]) && bits(v[1]) == bits(vabi.out[2 * i + 1]),
                   "WMultibandNoise2DCurlBounded scalar", i);
            zeros += bits(v[0]) == 0 && bits(v[1]) == 0;
            changed += bits(v[0]) != bits(plain[0]) || bits(v[1]) != bits(plain[1]);
        }
    }
    expect(zeros >= 100 && changed >= 1000 && changed < 2 * n, "inside, near and far points", zeros);
    {   // no obstacle, no stream: the unbounded bits
        std::vector<float> bounded(2 * n), plain(2 * n);
        noise.WMultibandNoise2DCurlBounded(xy.data(), n, nullptr, 0, nullptr, s, first, nb, w, variance, bounded.data());
        noise.WMultibandNoise2DCurl(xy.data(), n, s, first, nb, w, variance, plain.data());
        expect_equal(bounded, plain, "no obstacle and no stream");
    }

    // (2) advection: two steps more than one launch integrates, a snapshot every second step
    for (int method = WN_ADVECT_EULER; method <= WN_ADVECT_RK4; ++method)
        for (int pass = 0; pass < 2; ++pass) {
            const int steps = wn_advect2d_launch_steps(method, nb) + 2;
            const float *fl = pass ? flow : nullptr;
            const wn_advect2d a = {method, steps, pass ? -0.002f : 0.002f, 0.75f, {0.1f, -0.2f}, 2};
            const size_t snaps = (size_t)steps / 2 + 1;
            const Traced abi = via_abi(xy, 2 * n, snaps * 2 * n, [&](const float *in, float *out, float *traj) {
                return wn_multiband2d_curl_bounded_advect_points(t, in, n, s, first, nb, w, variance, obs, 3, fl, &a, out, traj,
                                                                 nullptr);
            });
            Traced b{std::vector<float>(2 * n), std::vector<float>(snaps * 2 * n)};
            noise.WMultibandNoise2DAdvectCurlBounded(xy.data(), n, a, obs, 3, fl, s, first, nb, w, variance, b.out.data(),
                                                     b.traj.data());
            expect_equal(b.out, abi.out, "WMultibandNoise2DAdvectCurlBounded batched");
            expect_equal(b.traj, abi.traj, "WMultibandNoise2DAdvectCurlBounded batched trajectory");
            for (size_t i = 0; i < n; i += 3) {
                float p[2];
                std::vector<float> path(2 * snaps);
                noise.WMultibandNoise2DAdvectCurlBounded(&xy[2 * i], a, obs, 3, fl, s, first, nb, w, p, path.data());
                for (int c = 0; c < 2; ++c) {
                    expect(bits(p[c]) == bits(abi.out[2 * i + c]), "WMultibandNoise2DAdvectCurlBounded scalar", i);
                    for (size_t k = 0; k < snaps; ++k)
                        expect(bits(path[2 * k + c]) == bits(abi.traj[(k * n + i) * 2 + c]), "scalar trajectory", i);
                }
            }
            // no trajectory, in place
            wn_advect2d plain = a;
            plain.traj_every = 0;
            std::vector<float> moved = xy;
            noise.WMultibandNoise2DAdvectCurlBounded(moved.data(), n, plain, obs, 3, fl, s, first, nb, w, variance, moved.data());
            expect_equal(moved, abi.out, "WMultibandNoise2DAdvectCurlBounded in place");
        }

    // (3) refused arguments throw
    const wn_advect2d good = {WN_ADVECT_RK4, 1, 0.1f, 1.0f, {0.0f, 0.0f}, 0}, bad = {7, 1, 0.1f, 1.0f, {0.0f, 0.0f}, 0};
    wn_obstacle2d flat = obs[0];
    flat.r = 0.0f;
    const float nan_flow[2] = {NAN, 0.0f};
    float p[2];
    std::vector<float> four(8);
    int thrown = 0;
    auto throws = [&](auto &&call) { try { call(); } catch (const std::runtime_error &) { ++thrown; } };
    throws([&] { noise.WMultibandNoise2DCurlBounded(xy.data(), &flat, 1, nullptr, s, first, nb, w, p); });
    throws([&] { noise.WMultibandNoise2DCurlBounded(xy.data(), 4, &flat, 1, nullptr, s, first, nb, w, variance, four.data()); });
    throws([&] { noise.WMultibandNoise2DCurlBounded(xy.data(), obs, 17, nullptr, s, first, nb, w, p); });
    throws([&] { noise.WMultibandNoise2DCurlBounded(xy.data(), obs, 3, nan_flow, s, first, nb, w, p); });
    throws([&] { noise.WMultibandNoise2DCurlBounded(xy.data(), 4, obs, 3, nan_flow, s, first, nb, w, variance, four.data()); });
    throws([&] { noise.WMultibandNoise2DAdvectCurlBounded(xy.data(), bad, obs, 3, flow, s, first, nb, w, p); });
    throws([&] { noise.WMultibandNoise2DAdvectCurlBounded(xy.data(), 4, bad, obs, 3, flow, s, first, nb, w, variance, four.data()); });
    throws([&] { noise.WMultibandNoise2DAdvectCurlBounded(xy.data(), good, &flat, 1, flow, s, first, nb, w, p); });
    throws([&] { noise.WMultibandNoise2DAdvectCurlBounded(xy.data(), 4, good, &flat, 1, flow, s, first, nb, w, variance, four.data()); });
    expect(thrown == 9, "refused arguments throw", (size_t)thrown);

    printf("points %zu, mismatches %ld\n", n, mismatches);
    return mismatches ? 1 : 0;
}
