// Host check of the boundary members of class perlin (host/perlin.h) and class PerlinNoise (host/PerlinNoise.hpp) against each
// other and the C ABI (include/wnoise_perlin_bounded.h), on a scene with far, near and inside points:
//  (1) perlin::curl_potential and curl_bounded: the scalar members, evaluated on the host, have the bits of the batched ones,
//      which call wn_perlin_curl_potential_points_f64 / _f32 and wn_perlin_curl_bounded_points_f64 / _f32, for the three kinds,
//      with explicit offsets and with the default ones; without obstacles curl_bounded is the curl member;
//  (2) perlin::advect_curl_bounded, scalar and batched (wn_perlin_curl_bounded_advect_points_f64), final positions and
//      trajectory, for the three kinds and methods, and in place; without obstacles it is advect_curl;
//  (3) PerlinNoise's three members, scalar against batched;
//  (4) an obstacle list, a kind or a wn_advect the ABI refuses makes the members throw.
// Test infrastructure: built by tests/test_gpu_perlin_bounded.py with g++ -ffp-contract=off against libwnoise_host.so.
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
#include "wnoise_perlin_bounded.h"

static uint64_t bits(double f) { uint64_t b; memcpy(&b, &f, 8); return b; }

static long mismatches = 0;
static void expect(bool ok, const char *what, size_t i)
{
    if (!ok && mismatches++ < 10) printf("mismatch: %s at %zu\n", what, i);
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
    std::mt19937 rng(23);
    std::uniform_real_distribution<double> u(-300.0, 300.0);
    std::vector<double> xyz(3 * n);
    for (auto &v : xyz) v = u(rng);
    xyz[0] = 3.0;
    xyz[1] = std::nextafter(-17.0, -INFINITY);
    xyz[2] = std::nextafter(128.0, -INFINITY);
    std::vector<float> xyz32(xyz.begin(), xyz.end());
    const int wide[9] = {-3, 260, 7, 511, -129, 1000, 2, -300, 255};
    // a solid ball, a floor and a container, their ramps overlapping
    const wn_obstacle scene[3] = {{WN_OBSTACLE_SPHERE, {0.0f, 0.0f, 0.0f}, 120.0f, 80.0f, {0, 0}},
                                  {WN_OBSTACLE_HALFSPACE, {0.0f, 1.0f, 0.0f}, -250.0f, 100.0f, {0, 0}},
                                  {WN_OBSTACLE_CONTAINER, {0.0f, 0.0f, 0.0f}, 500.0f, 150.0f, {0, 0}}};
    const size_t steps = 5, every = 2, snaps = steps / every + 1;
    static const int kinds[3][2] = {{WN_PERLIN_CURL_NOISE, 0}, {WN_PERLIN_CURL_TURB, 7}, {WN_PERLIN_CURL_FRACTAL, 0}};
    size_t zero = 0, changed = 0;

    for (const auto &kd : kinds) {
        const int kind = kd[0], depth = kd[1];
        const int *off = kind == WN_PERLIN_CURL_TURB ? nullptr : wide;
        // (1) the point members.  Float points for every kind; double points for noise.
        std::vector<double> psi(3 * n), v(3 * n), free_v(3 * n), none(3 * n);
        noise.curl_potential(xyz32.data(), n, kind, depth, off, psi.data());
        noise.curl_bounded(xyz32.data(), n, kind, depth, off, scene, 3, v.data());
        noise.curl_bounded(xyz32.data(), n, kind, depth, off, nullptr, 0, none.data());
        if (kind == WN_PERLIN_CURL_NOISE) noise.noise_curl(xyz32.data(), n, free_v.data(), off);
        else if (kind == WN_PERLIN_CURL_TURB) noise.turb_curl(xyz32.data(), n, free_v.data(), depth, off);
        else noise.fractal_noise_curl(xyz32.data(), n, free_v.data(), off);
        expect_equal(none, free_v, "curl_bounded without obstacles");
        for (size_t i = 0; i < n; ++i) {
            const double q[3] = {xyz32[3 * i], xyz32[3 * i + 1], xyz32[3 * i + 2]};
            double a[3], b[3];
            noise.curl_potential(q, kind, depth, off, a);
            noise.curl_bounded(q, kind, depth, off, scene, 3, b);
            for (int c = 0; c < 3; ++c) {
                expect(bits(a[c]) == bits(psi[3 * i + c]), "curl_potential scalar", i);
                expect(bits(b[c]) == bits(v[3 * i + c]), "curl_bounded scalar", i);
            }
            zero += b[0] == 0.0 && b[1] == 0.0 && b[2] == 0.0;
            changed += bits(b[0]) != bits(free_v[3 * i]);
        }
        if (kind == WN_PERLIN_CURL_NOISE) {
            noise.curl_potential(xyz.data(), n, off, psi.data());
            noise.curl_bounded(xyz.data(), n, off, scene, 3, v.data());
            for (size_t i = 0; i < n; ++i) {
                double a[3], b[3];
                noise.curl_potential(&xyz[3 * i], kind, depth, off, a);
                noise.curl_bounded(&xyz[3 * i], kind, depth, off, scene, 3, b);
                for (int c = 0; c < 3; ++c) {
                    expect(bits(a[c]) == bits(psi[3 * i + c]), "curl_potential scalar, double points", i);
                    expect(bits(b[c]) == bits(v[3 * i + c]), "curl_bounded scalar, double points", i);
                }
            }
        }
        // (2) advection: five steps, a snapshot every second step
        for (int method = WN_ADVECT_EULER; method <= WN_ADVECT_RK4; ++method) {
            const wn_advect a = {method, (int)steps, (method & 1) ? -0.37f : 0.37f, 0.75f, {0.1f, -0.2f, 0.05f}, (int)every};
            std::vector<double> out(3 * n), traj(snaps * 3 * n);
            noise.advect_curl_bounded(xyz.data(), n, a, kind, depth, off, scene, 3, out.data(), traj.data());
            for (size_t i = 0; i < n; ++i) {
                double p[3], path[3 * snaps];
                noise.advect_curl_bounded(&xyz[3 * i], a, kind, depth, off, scene, 3, p, path);
                for (int c = 0; c < 3; ++c) {
                    expect(bits(p[c]) == bits(out[3 * i + c]), "advect_curl_bounded scalar", i);
                    for (size_t s = 0; s < snaps; ++s)
                        expect(bits(path[3 * s + c]) == bits(traj[(s * n + i) * 3 + c]), "advect_curl_bounded scalar trajectory", i);
                }
            }
            wn_advect no_traj = a;
            no_traj.traj_every = 0;
            std::vector<double> moved = xyz, free_out(3 * n), none_out(3 * n);
            noise.advect_curl_bounded(moved.data(), n, no_traj, kind, depth, off, scene, 3, moved.data());
            expect_equal(moved, out, "advect_curl_bounded in place");
            noise.advect_curl(xyz.data(), n, no_traj, kind, depth, off, free_out.data());
            noise.advect_curl_bounded(xyz.data(), n, no_traj, kind, depth, off, nullptr, 0, none_out.data());
            expect_equal(none_out, free_out, "advect_curl_bounded without obstacles");
        }
    }
    expect(zero >= 3 * n / 20 && changed >= 3 * n / 5, "the scene has inside and near points", zero);

    // (3) PerlinNoise: noise potentials; the same seed gives the same table
    {
        std::vector<double> psi(3 * n), v(3 * n), out(3 * n), traj(snaps * 3 * n);
        const wn_advect a = {WN_ADVECT_RK4, (int)steps, 0.37f, 1.0f, {0.0f, 0.05f, 0.0f}, (int)every};
        plain_noise.curl_potential(xyz.data(), n, psi.data());
        plain_noise.curl_bounded(xyz.data(), n, scene, 3, v.data(), wide);
        plain_noise.advect_curl_bounded(xyz.data(), n, a, wide, scene, 3, out.data(), traj.data());
        for (size_t i = 0; i < n; ++i) {
            double s[3], b[3], p[3], path[3 * snaps];
            plain_noise.curl_potential(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], s);
            plain_noise.curl_bounded(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], scene, 3, b, wide);
            plain_noise.advect_curl_bounded(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], a, wide, scene, 3, p, path);
            for (int c = 0; c < 3; ++c) {
                expect(bits(s[c]) == bits(psi[3 * i + c]), "PerlinNoise::curl_potential", i);
                expect(bits(b[c]) == bits(v[3 * i + c]), "PerlinNoise::curl_bounded", i);
                expect(bits(p[c]) == bits(out[3 * i + c]), "PerlinNoise::advect_curl_bounded", i);
                for (size_t k = 0; k < snaps; ++k)
                    expect(bits(path[3 * k + c]) == bits(traj[(k * n + i) * 3 + c]), "PerlinNoise::advect_curl_bounded trajectory", i);
            }
        }
    }

    // (4) refused arguments throw
    wn_obstacle flat = scene[0];
    flat.d0 = 0.0f;
    const wn_advect bad = {7, 1, 0.1f, 1.0f, {0.0f, 0.0f, 0.0f}, 0};
    const wn_advect good = {WN_ADVECT_RK4, 1, 0.1f, 1.0f, {0.0f, 0.0f, 0.0f}, 0};
    double p[3];
    std::vector<double> four(12);
    int thrown = 0;
    try { noise.curl_bounded(xyz.data(), WN_PERLIN_CURL_NOISE, 0, wide, &flat, 1, p); } catch (const std::runtime_error &) { ++thrown; }
    try { noise.curl_bounded(xyz.data(), 4, wide, &flat, 1, four.data()); } catch (const std::runtime_error &) { ++thrown; }
    try { noise.curl_bounded(xyz.data(), 4, wide, scene, 17, four.data()); } catch (const std::runtime_error &) { ++thrown; }
    try { noise.curl_bounded(xyz32.data(), 4, 3, 0, wide, scene, 3, four.data()); } catch (const std::runtime_error &) { ++thrown; }
    try { noise.curl_potential(xyz.data(), WN_PERLIN_CURL_TURB, -1, wide, p); } catch (const std::runtime_error &) { ++thrown; }
    try { noise.advect_curl_bounded(xyz.data(), bad, WN_PERLIN_CURL_NOISE, 0, wide, scene, 3, p); } catch (const std::runtime_error &) { ++thrown; }
    try { noise.advect_curl_bounded(xyz.data(), 4, good, WN_PERLIN_CURL_NOISE, 0, wide, &flat, 1, four.data()); } catch (const std::runtime_error &) { ++thrown; }
    try { plain_noise.curl_bounded(1.0, 2.0, 3.0, &flat, 1, p); } catch (const std::runtime_error &) { ++thrown; }
    try { plain_noise.advect_curl_bounded(xyz.data(), 4, bad, wide, scene, 3, four.data()); } catch (const std::runtime_error &) { ++thrown; }
    expect(thrown == 9, "refused arguments throw", (size_t)thrown);

    printf("points %zu, inside %zu, mismatches %ld\n", n, zero, mismatches);
    return mismatches ? 1 : 0;
}
