// Host check of the advection members of class perlin (host/perlin.h) and class PerlinNoise (host/PerlinNoise.hpp) against the
// C ABI (include/wnoise_perlin_advect.h):
//  (1) perlin::advect_curl(xyz, a, kind, depth, offsets, p_out, traj) -- traced on the host -- and the batched
//      advect_curl(xyz, n, a, kind, depth, offsets, out, traj) have the bits of wn_perlin_curl_advect_points, final positions
//      and trajectory, for the three kinds and the three methods, with explicit offsets and with the default ones
//      (offsets == nullptr), and in place; the point3 form is the scalar form at the float point widened to double;
//  (2) PerlinNoise::advect_curl, scalar and batched, has the bits of the ABI with WN_PERLIN_CURL_NOISE;
//  (3) a wn_advect or a kind the ABI refuses makes the members throw.
// Test infrastructure: built by tests/test_gpu_perlin_advect.py with g++ -ffp-contract=off against libwnoise_host.so.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <stdexcept>
#include <vector>

#include "PerlinNoise.hpp"
#include "perlin.h"
#include "wnoise_perlin_advect.h"

static uint64_t bits(double f) { uint64_t b; memcpy(&b, &f, 8); return b; }

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
    std::vector<double> out, traj;
};

// The C ABI on device buffers: n final positions and `snaps` snapshots of n positions.
static Traced via_abi(const wn_perm *perm, const std::vector<double> &xyz, size_t n, int kind, int depth, const int *off,
                      const wn_advect &a, size_t snaps)
{
    void *in = nullptr, *out = nullptr, *traj = nullptr;
    check(wn_dev_alloc(&in, 3 * n * sizeof(double)), "wn_dev_alloc");
    check(wn_dev_alloc(&out, 3 * n * sizeof(double)), "wn_dev_alloc");
    check(wn_dev_alloc(&traj, snaps * 3 * n * sizeof(double)), "wn_dev_alloc");
    check(wn_copy_h2d(in, xyz.data(), 3 * n * sizeof(double), nullptr), "wn_copy_h2d");
    check(wn_perlin_curl_advect_points(perm, static_cast<const double *>(in), n, kind, depth, reinterpret_cast<const int32_t *>(off),
                                       &a, static_cast<double *>(out), static_cast<double *>(traj), nullptr),
          "wn_perlin_curl_advect_points");
    Traced r{std::vector<double>(3 * n), std::vector<double>(snaps * 3 * n)};
    check(wn_copy_d2h(r.out.data(), out, r.out.size() * sizeof(double), nullptr), "wn_copy_d2h");
    check(wn_copy_d2h(r.traj.data(), traj, r.traj.size() * sizeof(double), nullptr), "wn_copy_d2h");
    check(wn_stream_sync(nullptr), "wn_stream_sync");
    wn_dev_free(in);
    wn_dev_free(out);
    wn_dev_free(traj);
    return r;
}

static void expect_equal(const std::vector<double> &a, const std::vector<double> &b, const char *what)
{
    expect(a.size() == b.size(), what, 0);
    for (size_t i = 0; i < a.size() && i < b.size(); ++i) expect(bits(a[i]) == bits(b[i]), what, i);
}

int main()
{
    const perlin noise(12345);
    const PerlinNoise plain_noise(12345);
    const size_t n = 600;
    std::mt19937 rng(19);
    std::uniform_real_distribution<double> u(-300.0, 300.0);
    std::vector<double> xyz(3 * n);
    for (auto &v : xyz) v = u(rng);
    xyz[0] = 3.0; // an integer, and the doubles just below two more: (float) of those lies in the next cell
    xyz[1] = std::nextafter(-17.0, -INFINITY);
    xyz[2] = std::nextafter(128.0, -INFINITY);
    const int wide[9] = {-3, 260, 7, 511, -129, 1000, 2, -300, 255};
    const int *def = perlin::default_curl_offsets();
    const size_t steps = 5, every = 2, snaps = steps / every + 1;
    static const int kinds[3][2] = {{WN_PERLIN_CURL_NOISE, 0}, {WN_PERLIN_CURL_TURB, 7}, {WN_PERLIN_CURL_FRACTAL, 0}};

    // (1) perlin::advect_curl: five steps, a snapshot every second step
    for (const auto &kd : kinds)
        for (int method = WN_ADVECT_EULER; method <= WN_ADVECT_RK4; ++method) {
            const int kind = kd[0], depth = kd[1], pass = method & 1;
            const wn_advect a = {method, (int)steps, pass ? -0.37f : 0.37f, 0.75f, {0.1f, -0.2f, 0.05f}, (int)every};
            const int *member_off = pass == 0 ? wide : nullptr;
            const Traced abi = via_abi(noise.perm(), xyz, n, kind, depth, pass == 0 ? wide : def, a, snaps);
            Traced batched{std::vector<double>(3 * n), std::vector<double>(snaps * 3 * n)};
            noise.advect_curl(xyz.data(), n, a, kind, depth, member_off, batched.out.data(), batched.traj.data());
            expect_equal(batched.out, abi.out, "advect_curl batched");
            expect_equal(batched.traj, abi.traj, "advect_curl batched trajectory");
            for (size_t i = 0; i < n; ++i) {
                double p[3], path[3 * snaps];
                noise.advect_curl(&xyz[3 * i], a, kind, depth, member_off, p, path);
                for (int c = 0; c < 3; ++c) {
                    expect(bits(p[c]) == bits(abi.out[3 * i + c]), "advect_curl scalar", i);
                    for (size_t s = 0; s < snaps; ++s)
                        expect(bits(path[3 * s + c]) == bits(abi.traj[(s * n + i) * 3 + c]), "advect_curl scalar trajectory", i);
                }
            }
            // no trajectory, in place
            wn_advect no_traj = a;
            no_traj.traj_every = 0;
            std::vector<double> moved = xyz;
            noise.advect_curl(moved.data(), n, no_traj, kind, depth, member_off, moved.data());
            expect_equal(moved, abi.out, "advect_curl in place");
            // the point3 form: the float point, widened
            for (size_t i = 0; i < 20; ++i) {
                const point3 q((float)xyz[3 * i], (float)xyz[3 * i + 1], (float)xyz[3 * i + 2]);
                const double wide_q[3] = {q.x(), q.y(), q.z()};
                double a3[3], b3[3];
                noise.advect_curl(q, no_traj, kind, depth, member_off, a3);
                noise.advect_curl(wide_q, no_traj, kind, depth, member_off, b3);
                for (int c = 0; c < 3; ++c) expect(bits(a3[c]) == bits(b3[c]), "advect_curl point3", i);
            }
        }

    // (2) PerlinNoise::advect_curl: noise potentials; the same seed gives the same table
    for (int pass = 0; pass < 2; ++pass) {
        const wn_advect a = {WN_ADVECT_RK4, (int)steps, pass ? -0.37f : 0.37f, 1.0f, {0.0f, 0.05f, 0.0f}, (int)every};
        const int *member_off = pass == 0 ? wide : nullptr;
        const Traced abi = via_abi(plain_noise.perm(), xyz, n, WN_PERLIN_CURL_NOISE, 0, pass == 0 ? wide : def, a, snaps);
        Traced batched{std::vector<double>(3 * n), std::vector<double>(snaps * 3 * n)};
        plain_noise.advect_curl(xyz.data(), n, a, member_off, batched.out.data(), batched.traj.data());
        expect_equal(batched.out, abi.out, "PerlinNoise::advect_curl batched");
        expect_equal(batched.traj, abi.traj, "PerlinNoise::advect_curl batched trajectory");
        for (size_t i = 0; i < n; ++i) {
            double p[3], path[3 * snaps];
            plain_noise.advect_curl(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], a, member_off, p, path);
            for (int c = 0; c < 3; ++c) {
                expect(bits(p[c]) == bits(abi.out[3 * i + c]), "PerlinNoise::advect_curl scalar", i);
                for (size_t s = 0; s < snaps; ++s)
                    expect(bits(path[3 * s + c]) == bits(abi.traj[(s * n + i) * 3 + c]), "PerlinNoise::advect_curl scalar trajectory", i);
            }
        }
    }

    // (3) refused arguments throw
    const wn_advect bad = {7, 1, 0.1f, 1.0f, {0.0f, 0.0f, 0.0f}, 0};
    const wn_advect good = {WN_ADVECT_RK4, 1, 0.1f, 1.0f, {0.0f, 0.0f, 0.0f}, 0};
    double p[3];
    std::vector<double> four(12);
    int thrown = 0;
    try { noise.advect_curl(xyz.data(), bad, WN_PERLIN_CURL_NOISE, 0, wide, p); } catch (const std::runtime_error &) { ++thrown; }
    try { noise.advect_curl(xyz.data(), 4, bad, WN_PERLIN_CURL_NOISE, 0, wide, four.data()); } catch (const std::runtime_error &) { ++thrown; }
    try { noise.advect_curl(xyz.data(), good, 3, 0, wide, p); } catch (const std::runtime_error &) { ++thrown; }
    try { noise.advect_curl(xyz.data(), 4, good, WN_PERLIN_CURL_TURB, -1, wide, four.data()); } catch (const std::runtime_error &) { ++thrown; }
    try { plain_noise.advect_curl(1.0, 2.0, 3.0, bad, wide, p); } catch (const std::runtime_error &) { ++thrown; }
    try { plain_noise.advect_curl(xyz.data(), 4, bad, wide, four.data()); } catch (const std::runtime_error &) { ++thrown; }
    expect(thrown == 6, "refused arguments throw", (size_t)thrown);

    printf("points %zu, mismatches %ld\n", n, mismatches);
    return mismatches ? 1 : 0;
}
