// wn_eval.hpp -- the per-sample evaluators in the reference's exact operation order, each stated once for the HIP kernels
// (csrc/) and for the host's wnhost_* functions (host/scalar_eval.cpp).  Both compilers build it with -ffp-contract=off:
// every product and sum below rounds once, as on the reference's baseline x86-64 build, so host and device return the
// same bits as the CPU classes.  Only <cmath> / <cstdint>: no HIP header, so that a plain C++ compiler can include it.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define WN_EVAL_FN __host__ __device__ __forceinline__
#define WN_UNROLL _Pragma("unroll")
#else
#define WN_EVAL_FN inline __attribute__((always_inline))
#define WN_UNROLL
#endif

namespace wn {

// n-1 when n is a power of two (indices wrap with a mask), else -1.
WN_EVAL_FN int pow2_mask(int n) { return (n > 0 && (n & (n - 1)) == 0) ? n - 1 : -1; }

// Non-negative modulo (WaveletNoise.cpp:31-34); `mask` = n-1 when n is a power of two, else -1.
WN_EVAL_FN int dmod(int x, int n, int mask)
{
    if (mask >= 0) return x & mask;
    int m = x % n;
    return m < 0 ? m + n : m;
}

// Quadratic B-spline weights (WaveletNoise.cpp:194-200).
WN_EVAL_FN void bspline(float p, int &mid, float &w0, float &w1, float &w2)
{
    const float pm = p - 0.5f;
    const float cm = ceilf(pm);
    mid = (int)cm;
    const float t = cm - pm;
    w0 = t * t / 2.0f;
    w2 = (1.0f - t) * (1.0f - t) / 2.0f;
    w1 = 1.0f - w0 - w2;
}

// bspline, and the derivatives of the three weights with respect to p (dt/dp = -1): d0 = -t, d1 = 2t - 1, d2 = 1 - t.
WN_EVAL_FN void bspline_grad(float p, int &mid, float w[3], float d[3])
{
    bspline(p, mid, w[0], w[1], w[2]);
    const float t = (float)mid - (p - 0.5f);
    d[0] = -t;
    d[1] = 2.0f * t - 1.0f;
    d[2] = 1.0f - t;
}

// WaveletNoise::evaluate2D, WaveletNoise.cpp:111-140 (f1 outer, f0 inner; weight = w0*w1).
// GRAD: beside the value's sum (unchanged: the same bits) the two derivative sums over the same 9 coefficients, tap
// weights d_x*w_y and w_x*d_y, each accumulated f1 -> f0, unfused; d/dx, d/dy go to g.
// PADDED: `coef` has row stride n+2 with two wrap-around columns (padded[y][x] = tile[y][x mod n] for x in [0, n+2)), the
// layout the 2-D multiband kernels stage in LDS: the three x taps of a row are adjacent; the values, the arithmetic and its
// order are those of the linear layout.
template <bool GRAD = false, bool PADDED = false>
WN_EVAL_FN float eval2d_exact(const float *coef, int n, int nmask, float px, float py, float *g = nullptr)
{
    if (n == 0) { // :112-114; the empty tile: 0 in every channel
        if constexpr (GRAD) g[0] = g[1] = 0.0f;
        return 0.0f;
    }
    int mx, my;
    float wx[3], wy[3], dx[3], dy[3];
    if constexpr (GRAD) {
        bspline_grad(px, mx, wx, dx);
        bspline_grad(py, my, wy, dy);
    } else {
        bspline(px, mx, wx[0], wx[1], wx[2]);
        bspline(py, my, wy[0], wy[1], wy[2]);
    }
    int cx[3], cy[3];
    WN_UNROLL
    for (int f = 0; f < 3; ++f) {
        cx[f] = dmod(mx + f - 1, n, nmask);
        cy[f] = dmod(my + f - 1, n, nmask) * (PADDED ? n + 2 : n);
    }
    float result = 0.0f, gx = 0.0f, gy = 0.0f;
    WN_UNROLL
    for (int fy = 0; fy < 3; ++fy)
        WN_UNROLL
        for (int fx = 0; fx < 3; ++fx) {
            const float weight = wx[fx] * wy[fy];
            const float c = PADDED ? coef[cx[0] + fx + cy[fy]] : coef[cx[fx] + cy[fy]];
            result += weight * c;
            if constexpr (GRAD) {
                gx += dx[fx] * wy[fy] * c;
                gy += wx[fx] * dy[fy] * c;
            }
        }
    if constexpr (GRAD) {
        g[0] = gx;
        g[1] = gy;
    }
    return result;
}

// WaveletNoise::evaluate3D, WaveletNoise.cpp:185-215 (f2 outer, f0 inner; weight=(w0*w1)*w2).
// PADDED: `coef` is wn_tile::dev_padded (row stride n+2 with two wrap-around columns), so the
// three x taps of every (y,z) row are adjacent and fetched with one 12-byte load; the values, the
// arithmetic and its order are those of the linear layout.
// POW2: the tile size is a power of two and the wrap a mask.  The general modulo behind a run-time test per index splits the
// nine loads into basic blocks (a branch per wrap); eval3d_exact tests once and calls the form that has none.
// GRAD: beside the value's sum (unchanged: the same bits) the three derivative sums over the same 27 coefficients, tap
// weights (d_x*w_y)*w_z, (w_x*d_y)*w_z and (w_x*w_y)*d_z, each accumulated f2 -> f1 -> f0, unfused; the gradient goes to g.
template <bool PADDED, bool POW2, bool GRAD>
WN_EVAL_FN float eval3d_exact_impl(const float *coef, int n, int nmask, float px, float py, float pz, float *g)
{
    int mx, my, mz;
    float wx[3], wy[3], wz[3], dx[3], dy[3], dz[3];
    if constexpr (GRAD) {
        bspline_grad(px, mx, wx, dx);
        bspline_grad(py, my, wy, dy);
        bspline_grad(pz, mz, wz, dz);
    } else {
        bspline(px, mx, wx[0], wx[1], wx[2]);
        bspline(py, my, wy[0], wy[1], wy[2]);
        bspline(pz, mz, wz[0], wz[1], wz[2]);
    }
    const int stride = PADDED ? n + 2 : n;
    int cx[3], cy[3], cz[3];
    WN_UNROLL
    for (int f = 0; f < 3; ++f) {
        cx[f] = POW2 ? ((mx + f - 1) & nmask) : dmod(mx + f - 1, n, -1);
        cy[f] = (POW2 ? ((my + f - 1) & nmask) : dmod(my + f - 1, n, -1)) * stride;
        cz[f] = (POW2 ? ((mz + f - 1) & nmask) : dmod(mz + f - 1, n, -1)) * stride * n;
    }
    float result = 0.0f, gx = 0.0f, gy = 0.0f, gz = 0.0f;
    WN_UNROLL
    for (int fz = 0; fz < 3; ++fz)
        WN_UNROLL
        for (int fy = 0; fy < 3; ++fy) {
            float c[3];
            if (PADDED) {
                __builtin_memcpy(c, coef + cx[0] + cy[fy] + cz[fz], sizeof(c)); // global_load_dwordx3
            } else {
                WN_UNROLL
                for (int fx = 0; fx < 3; ++fx) c[fx] = coef[cx[fx] + cy[fy] + cz[fz]];
            }
            WN_UNROLL
            for (int fx = 0; fx < 3; ++fx) {
                const float weight = wx[fx] * wy[fy] * wz[fz];
                result += weight * c[fx];
                if constexpr (GRAD) {
                    gx += dx[fx] * wy[fy] * wz[fz] * c[fx];
                    gy += wx[fx] * dy[fy] * wz[fz] * c[fx];
                    gz += wx[fx] * wy[fy] * dz[fz] * c[fx];
                }
            }
        }
    if constexpr (GRAD) {
        g[0] = gx;
        g[1] = gy;
        g[2] = gz;
    }
    return result;
}

template <bool PADDED = false>
WN_EVAL_FN float eval3d_exact(const float *coef, int n, int nmask, float px, float py, float pz)
{
    if (n == 0) return 0.0f; // :186-188
    return nmask >= 0 ? eval3d_exact_impl<PADDED, true, false>(coef, n, nmask, px, py, pz, nullptr)
                      : eval3d_exact_impl<PADDED, false, false>(coef, n, nmask, px, py, pz, nullptr);
}

// Returns the value, writes the gradient to g.
template <bool PADDED = false>
WN_EVAL_FN float eval3d_grad_exact(const float *coef, int n, int nmask, float px, float py, float pz, float g[3])
{
    if (n == 0) { // the empty tile: 0 in all four channels
        g[0] = g[1] = g[2] = 0.0f;
        return 0.0f;
    }
    return nmask >= 0 ? eval3d_exact_impl<PADDED, true, true>(coef, n, nmask, px, py, pz, g)
                      : eval3d_exact_impl<PADDED, false, true>(coef, n, nmask, px, py, pz, g);
}

// ---- WaveletNoise::evaluate3DProjected, WaveletNoise.cpp:218-265 -------------------------------------------------------
// Axis i of the data-dependent support box of the projected basis around p, :226-231.
WN_EVAL_FN void projected_box(const float p[3], const float nrm[3], int i, int lo[3], int hi[3])
{
    const float support = 3.0f * fabsf(nrm[i]) + 3.0f * sqrtf((1.0f - nrm[i] * nrm[i]) / 2.0f);
    lo[i] = (int)ceilf(p[i] - support);
    hi[i] = (int)floorf(p[i] + support);
}

// One axis of the projected basis at 0 < t < 3, :249-253: B(t), and B'(t) = t, t2 - t1, -t3 on the three pieces to d.
template <bool GRAD>
WN_EVAL_FN float projected_piece(float t, float *d)
{
    const float t1 = t - 1.0f, t2 = 2.0f - t, t3 = 3.0f - t;
    const float b = t < 1.0f ? (t * t / 2.0f) : (t < 2.0f ? (1.0f - (t1 * t1 + t2 * t2) / 2.0f) : (t3 * t3 / 2.0f));
    if constexpr (GRAD) *d = t < 1.0f ? t : (t < 2.0f ? t2 - t1 : -t3);
    return b;
}

// The value: `break` on the first axis outside the basis support, contributions <= 1e-6 skipped.
WN_EVAL_FN float projected_exact(const float *coef, int n, int nmask, const float p[3], const float nrm[3])
{
    if (n == 0) return 0.0f; // :219-221
    int lo[3], hi[3];
    WN_UNROLL
    for (int i = 0; i < 3; ++i) projected_box(p, nrm, i, lo, hi);
    float result = 0.0f;
    for (int c2 = lo[2]; c2 <= hi[2]; ++c2)
        for (int c1 = lo[1]; c1 <= hi[1]; ++c1)
            for (int c0 = lo[0]; c0 <= hi[0]; ++c0) {
                const float cf[3] = {(float)c0, (float)c1, (float)c2};
                float dot = 0.0f;
                WN_UNROLL
                for (int i = 0; i < 3; ++i) dot += nrm[i] * (p[i] - cf[i]);
                float weight = 1.0f;
                bool outside = false;
                WN_UNROLL
                for (int i = 0; i < 3; ++i) {
                    if (!outside) {
                        const float t = (cf[i] + nrm[i] * dot / 2.0f) - (p[i] - 1.5f);
                        if (t <= 0.0f || t >= 3.0f) {
                            weight = 0.0f;
                            outside = true;
                        } else {
                            weight *= projected_piece<false>(t, nullptr);
                        }
                    }
                }
                if ((double)weight > 1e-6) { // :257 compares against a double literal
                    const int idx = dmod(c0, n, nmask) + dmod(c1, n, nmask) * n + dmod(c2, n, nmask) * n * n;
                    result += weight * coef[idx];
                }
            }
    return result;
}

// evaluate3DProjected and its gradient with respect to p, the normal held fixed.  One pass over projected_exact's support
// box.  A cell with t_i = (c_i + n_i*dot/2) - (p_i - 1.5), dot = sum_k n_k (p_k - c_k), has weight prod_i B(t_i); with
// G_i = B'(t_i) prod_{k!=i} B(t_k) and S = sum_i n_i G_i, dt_i/dp_j = n_i n_j / 2 - delta_ij gives
// d weight / dp_j = (n_j/2) S - G_j.
//  - value: projected_exact's arithmetic, cell for cell (the same t, the same (B0*B1)*B2, the same weight > 1e-6 cut): its
//    bits.  Its per-axis `break` only ends a product that is then 0 and cut, so every axis's t is formed here up front.
//  - gradient: EVERY cell with 0 < t_i < 3 on all three axes, no 1e-6 cut (a cut sum would jump by up to ~1e-3 |c| when a
//    cell crosses the threshold; the uncut sum is C1).  G_i = (B'0*B1)*B2, (B0*B'1)*B2, (B0*B1)*B'2; S = (n0 G0 + n1 G1) +
//    n2 G2; each dweight_j * c accumulated in the box's order (c2 -> c1 -> c0), unfused.
// The box is the value's: no cell outside it has 0 < t < 3 on all three axes (its half-width 3|n_i| + 3 sqrt((1-n_i^2)/2)
// bounds |p_i - c_i| of every such cell).  Returns the value, writes the gradient to g.
WN_EVAL_FN float projected_grad_exact(const float *coef, int n, int nmask, const float p[3], const float nrm[3], float g[3])
{
    if (n == 0) { // the empty tile: 0 in all four channels
        g[0] = g[1] = g[2] = 0.0f;
        return 0.0f;
    }
    // per point, once: the box, p_i - 1.5f and n_j / 2
    int lo[3], hi[3];
    float pm[3], hn[3];
    WN_UNROLL
    for (int i = 0; i < 3; ++i) {
        projected_box(p, nrm, i, lo, hi);
        pm[i] = p[i] - 1.5f;
        hn[i] = nrm[i] / 2.0f;
    }
    float result = 0.0f, gx = 0.0f, gy = 0.0f, gz = 0.0f;
    for (int c2 = lo[2]; c2 <= hi[2]; ++c2)
        for (int c1 = lo[1]; c1 <= hi[1]; ++c1)
            for (int c0 = lo[0]; c0 <= hi[0]; ++c0) {
                const float cf[3] = {(float)c0, (float)c1, (float)c2};
                float dot = 0.0f;
                WN_UNROLL
                for (int i = 0; i < 3; ++i) dot += nrm[i] * (p[i] - cf[i]);
                float b[3], d[3];
                bool inside = true;
                WN_UNROLL
                for (int i = 0; i < 3; ++i) {
                    const float t = (cf[i] + nrm[i] * dot / 2.0f) - pm[i];
                    inside = inside && t > 0.0f && t < 3.0f;
                    b[i] = projected_piece<true>(t, &d[i]);
                }
                if (inside) {
                    const float c = coef[dmod(c0, n, nmask) + dmod(c1, n, nmask) * n + dmod(c2, n, nmask) * n * n];
                    const float weight = b[0] * b[1] * b[2];
                    if ((double)weight > 1e-6) result += weight * c;
                    const float g0 = d[0] * b[1] * b[2], g1 = b[0] * d[1] * b[2], g2 = b[0] * b[1] * d[2];
                    const float s = nrm[0] * g0 + nrm[1] * g1 + nrm[2] * g2;
                    gx += (hn[0] * s - g0) * c;
                    gy += (hn[1] * s - g1) * c;
                    gz += (hn[2] * s - g2) * c;
                }
            }
    g[0] = gx;
    g[1] = gy;
    g[2] = gz;
    return result;
}

// WMultibandNoise (paper Appendix 2): sum_b w[b] * f(q_b), q_b = 2 * p * 2^(first_band+b), divided by out_div when
// apply_div.  f is evaluate3D (PROJECTED false: the normal == NULL branch, nrm unused) or evaluate3DProjected(q_b, nrm).
// GRAD: also the gradient with respect to p to g: band b adds (w[b] * (2 * 2^(first_band+b))) * grad f(q_b) (the chain
// rule of q_b), divided like the value, whose bits do not change.  `a` carries coef, n, nmask and the bands of
// wn::multiband_bands.  (The value arm reads w[b] before f and the gradient arm after it: the kernels' code depends on that order.)
template <bool PADDED, bool PROJECTED, bool GRAD, typename A>
WN_EVAL_FN float multiband_exact(const A &a, const float p[3], const float *nrm, float *g)
{
    float v = 0.0f, gx = 0.0f, gy = 0.0f, gz = 0.0f;
    for (int b = 0; b < a.nbands; ++b) {
        const float s = a.band_scale[b];
        const float q[3] = {2.0f * p[0] * s, 2.0f * p[1] * s, 2.0f * p[2] * s};
        if constexpr (GRAD) {
            float gb[3];
            const float e = PROJECTED ? projected_grad_exact(a.coef, a.n, a.nmask, q, nrm, gb)
                                      : eval3d_grad_exact<PADDED>(a.coef, a.n, a.nmask, q[0], q[1], q[2], gb);
            v += a.band_w[b] * e;
            const float f = a.band_w[b] * (2.0f * s);
            gx += f * gb[0];
            gy += f * gb[1];
            gz += f * gb[2];
        } else {
            v += a.band_w[b] * (PROJECTED ? projected_exact(a.coef, a.n, a.nmask, q, nrm)
                                          : eval3d_exact<PADDED>(a.coef, a.n, a.nmask, q[0], q[1], q[2]));
        }
    }
    if (a.apply_div) {
        v /= a.out_div;
        if constexpr (GRAD) {
            gx /= a.out_div;
            gy /= a.out_div;
            gz /= a.out_div;
        }
    }
    if constexpr (GRAD) {
        g[0] = gx;
        g[1] = gy;
        g[2] = gz;
    }
    return v;
}

// ---- WMultibandNoise with a footprint per sample (include/wnoise_footprint.h) -------------------------------------------
// The paper's loop stops at the first band with s + firstBand + b >= 0, s = log2 of the SAMPLE's footprint: here s is an
// argument of the evaluation, not of the call.  FootprintBands carries what does not depend on the sample: all nbands
// bands (band_scale[b] = 2^(first_band+b), band_w[b] = w[b], unfaded), first_band as a float, the fade switch, and the
// division of multiband_exact -- out_div = sqrtf(sum over ALL nbands of w^2 * var_per_band), applied when that sum is
// non-zero, whatever the sample's own band count.
constexpr int kFootprintMaxBands = 8;
struct FootprintBands {
    int nbands; // all of them: the sample's s decides how many run
    float first_f;
    int fade;
    float band_scale[kFootprintMaxBands], band_w[kFootprintMaxBands];
    float out_div;
    int apply_div;
};

// nbands in 0 .. kFootprintMaxBands and w valid (or nbands == 0): the callers check.
inline void footprint_bands_fill(int first_band, int nbands, const float *w, float var_per_band, int fade, FootprintBands *a)
{
    float variance = 0.0f;
    for (int b = 0; b < nbands; ++b) variance += w[b] * w[b];
    a->nbands = nbands;
    a->first_f = (float)first_band;
    a->fade = fade ? 1 : 0;
    for (int b = 0; b < nbands; ++b) {
        a->band_scale[b] = ldexpf(1.0f, first_band + b);
        a->band_w[b] = w[b];
    }
    a->apply_div = variance != 0.0f;
    a->out_div = a->apply_div ? sqrtf(variance * var_per_band) : 1.0f;
}

// t_b = (s + first_band) + b, in this association: the expression wn::multiband_bands evaluates.  Band b runs iff t_b < 0
// (a NaN or +inf s: no band; -inf: all of them); t_b does not decrease with b, so the first band that fails ends the loop.
template <typename A>
WN_EVAL_FN float footprint_t(const A &a, float s, int b)
{
    return (s + a.first_f) + (float)b;
}

// multiband_exact with the band limit taken from the sample's footprint s.  Band b runs while t_b < 0 and enters with the
// one float product wb = w[b] * f_b: f_b = 1.0f without fade (the paper's hard cut), fminf(1.0f, -t_b) with it -- the
// finest surviving band fades in linearly over one octave of footprint instead of popping.  The value adds wb * e_b, the
// gradient (wb * (2 * 2^(first_band+b))) * grad e_b; the fade does not depend on p, so that is the gradient of the faded
// sum.  Band order, the unfused arithmetic and the division are multiband_exact's: where f_b == 1 for every band that runs
// (every sample without fade; with it, integer-valued s) the bits are those of multiband_exact at s.  No band: 0 (divided
// like any other sum).  `a` carries coef, n, nmask and a FootprintBands.
template <bool PADDED, bool PROJECTED, bool GRAD, typename A>
WN_EVAL_FN float multiband_footprint_exact(const A &a, const float p[3], const float *nrm, float s, float *g)
{
    float v = 0.0f, gx = 0.0f, gy = 0.0f, gz = 0.0f;
    for (int b = 0; b < a.nbands; ++b) {
        const float t = footprint_t(a, s, b);
        if (!(t < 0.0f)) break;
        const float wb = a.band_w[b] * (a.fade ? fminf(1.0f, -t) : 1.0f);
        const float bs = a.band_scale[b];
        const float q[3] = {2.0f * p[0] * bs, 2.0f * p[1] * bs, 2.0f * p[2] * bs};
        if constexpr (GRAD) {
            float gb[3];
            const float e = PROJECTED ? projected_grad_exact(a.coef, a.n, a.nmask, q, nrm, gb)
                                      : eval3d_grad_exact<PADDED>(a.coef, a.n, a.nmask, q[0], q[1], q[2], gb);
            v += wb * e;
            const float f = wb * (2.0f * bs);
            gx += f * gb[0];
            gy += f * gb[1];
            gz += f * gb[2];
        } else {
            v += wb * (PROJECTED ? projected_exact(a.coef, a.n, a.nmask, q, nrm)
                                 : eval3d_exact<PADDED>(a.coef, a.n, a.nmask, q[0], q[1], q[2]));
        }
    }
    if (a.apply_div) {
        v /= a.out_div;
        if constexpr (GRAD) {
            gx /= a.out_div;
            gy /= a.out_div;
            gz /= a.out_div;
        }
    }
    if constexpr (GRAD) {
        g[0] = gx;
        g[1] = gy;
        g[2] = gz;
    }
    return v;
}

// ---- 2-D WMultibandNoise (include/wnoise_multiband2d.h; absent from the reference) ----------------------------------------
// multiband_footprint_exact on a 2-D tile: band b runs while t_b = footprint_t(a, s, b) < 0 and enters with the one float
// product wb = w[b] * f_b (f_b = 1.0f without fade, fminf(1.0f, -t_b) with it); the value adds wb * evaluate2D(q_b), the
// gradient with respect to p (wb * (2 * 2^(first_band+b))) * grad evaluate2D(q_b), q_b = 2 * p * 2^(first_band+b); band
// order, the unfused arithmetic and the division by out_div (when apply_div) are multiband_footprint_exact's.  The uniform-s
// entry points are this function at the call's s with fade 0, so a footprint sample whose active bands all have f_b == 1
// has the bits of the uniform call at its s by construction.  No active band, or an empty tile: 0 in every channel.
// `a` carries n, nmask and a FootprintBands; `coef` is passed beside it because the kernels that stage the tile in LDS
// read it there (PADDED: the padded layout of eval2d_exact).
template <bool GRAD, bool PADDED = false, typename A>
WN_EVAL_FN float multiband2d_footprint_exact(const A &a, const float *coef, const float p[2], float s, float *g)
{
    float v = 0.0f, gx = 0.0f, gy = 0.0f;
    for (int b = 0; b < a.nbands; ++b) {
        const float t = footprint_t(a, s, b);
        if (!(t < 0.0f)) break;
        const float wb = a.band_w[b] * (a.fade ? fminf(1.0f, -t) : 1.0f);
        const float bs = a.band_scale[b];
        const float qx = 2.0f * p[0] * bs, qy = 2.0f * p[1] * bs;
        if constexpr (GRAD) {
            float gb[2];
            const float e = eval2d_exact<true, PADDED>(coef, a.n, a.nmask, qx, qy, gb);
            v += wb * e;
            const float f = wb * (2.0f * bs);
            gx += f * gb[0];
            gy += f * gb[1];
        } else {
            v += wb * eval2d_exact<false, PADDED>(coef, a.n, a.nmask, qx, qy);
        }
    }
    if (a.apply_div) {
        v /= a.out_div;
        if constexpr (GRAD) {
            gx /= a.out_div;
            gy /= a.out_div;
        }
    }
    if constexpr (GRAD) {
        g[0] = gx;
        g[1] = gy;
    }
    return v;
}

// The curl of the stream function psi = multiband2d_footprint_exact<GRAD = true> at the call-wide footprint s with fade 0
// (include/wnoise_curl2d.h): v = (d psi/dy, -d psi/dx).  The band loop, the chain-rule factor and the division are that
// function's (fade 0: wb = w[b] * 1.0f = w[b] exactly; a.fade is not read); the value sum is not formed.  v[0] has the bits of
// its d/dy channel, v[1] those of its d/dx channel with the sign flipped.  No active band, or an empty tile: v = 0.
// first_band = -1, nbands = 1, w = {1}, var_per_band = 1: q = 2 * p * 2^-1 = p exactly and out_div = 1, the curl of plain
// evaluate2D(p).
template <bool PADDED = false, typename A>
WN_EVAL_FN void multiband2d_curl_exact(const A &a, const float *coef, const float p[2], float s, float v[2])
{
    float gx = 0.0f, gy = 0.0f;
    for (int b = 0; b < a.nbands; ++b) {
        const float t = footprint_t(a, s, b);
        if (!(t < 0.0f)) break;
        const float bs = a.band_scale[b];
        float gb[2];
        eval2d_exact<true, PADDED>(coef, a.n, a.nmask, 2.0f * p[0] * bs, 2.0f * p[1] * bs, gb);
        const float f = a.band_w[b] * (2.0f * bs);
        gx += f * gb[0];
        gy += f * gb[1];
    }
    if (a.apply_div) {
        gx /= a.out_div;
        gy /= a.out_div;
    }
    v[0] = gy;
    v[1] = -gx;
}

// ---- curl of a vector potential of three whole-cell shifts of one tile (absent from the reference) ---------------------
// Psi = (psi0, psi1, psi2), psi_k = evaluate3D of the tile T_k[z][y][x] = C[Mod(z+oz_k)][Mod(y+oy_k)][Mod(x+ox_k)];
// v = curl Psi = (d psi2/dy - d psi1/dz, d psi0/dz - d psi2/dx, d psi1/dx - d psi0/dy).  The shifts are whole cells, so the
// three potentials share mids, weights and derivatives (bspline_grad once per axis) and differ in the coefficients read.
// `off`: the nine offsets (x, y, z of psi0, psi1, psi2), each already reduced to [0, n) with dmod.

// The two derivative sums that the curl needs of potential K (psi0: d/dy, d/dz; psi1: d/dx, d/dz; psi2: d/dx, d/dy): the
// sums of eval3d_exact_impl<.., GRAD> for those channels -- the same tap weights, f2 -> f1 -> f0, unfused -- over the
// coefficients at the offset indices: the bits of that evaluator on T_K.
template <bool PADDED, bool POW2, int K>
WN_EVAL_FN void curl_potential_sums(const float *coef, int n, int nmask, const int *off, int mx, int my, int mz,
                                    const float *wx, const float *wy, const float *wz, const float *dx, const float *dy,
                                    const float *dz, float &s0, float &s1)
{
    const int stride = PADDED ? n + 2 : n;
    int cx[3], cy[3], cz[3];
    WN_UNROLL
    for (int f = 0; f < 3; ++f) {
        cx[f] = POW2 ? ((mx + f - 1 + off[3 * K]) & nmask) : dmod(mx + f - 1 + off[3 * K], n, -1);
        cy[f] = (POW2 ? ((my + f - 1 + off[3 * K + 1]) & nmask) : dmod(my + f - 1 + off[3 * K + 1], n, -1)) * stride;
        cz[f] = (POW2 ? ((mz + f - 1 + off[3 * K + 2]) & nmask) : dmod(mz + f - 1 + off[3 * K + 2], n, -1)) * stride * n;
    }
    float a0 = 0.0f, a1 = 0.0f;
    WN_UNROLL
    for (int fz = 0; fz < 3; ++fz)
        WN_UNROLL
        for (int fy = 0; fy < 3; ++fy) {
            float c[3];
            if (PADDED) {
                __builtin_memcpy(c, coef + cx[0] + cy[fy] + cz[fz], sizeof(c)); // the x taps stay adjacent under an x offset
            } else {
                WN_UNROLL
                for (int fx = 0; fx < 3; ++fx) c[fx] = coef[cx[fx] + cy[fy] + cz[fz]];
            }
            WN_UNROLL
            for (int fx = 0; fx < 3; ++fx) {
                if constexpr (K == 0) {
                    a0 += wx[fx] * dy[fy] * wz[fz] * c[fx];
                    a1 += wx[fx] * wy[fy] * dz[fz] * c[fx];
                } else if constexpr (K == 1) {
                    a0 += dx[fx] * wy[fy] * wz[fz] * c[fx];
                    a1 += wx[fx] * wy[fy] * dz[fz] * c[fx];
                } else {
                    a0 += dx[fx] * wy[fy] * wz[fz] * c[fx];
                    a1 += wx[fx] * dy[fy] * wz[fz] * c[fx];
                }
            }
        }
    s0 = a0;
    s1 = a1;
}

// The six sums at one point: s = {d psi0/dy, d psi0/dz, d psi1/dx, d psi1/dz, d psi2/dx, d psi2/dy}; an empty tile: 0.
template <bool PADDED = false>
WN_EVAL_FN void eval3d_curl_sums(const float *coef, int n, int nmask, const int *off, float px, float py, float pz, float s[6])
{
    if (n == 0) {
        WN_UNROLL
        for (int i = 0; i < 6; ++i) s[i] = 0.0f;
        return;
    }
    int mx, my, mz;
    float wx[3], wy[3], wz[3], dx[3], dy[3], dz[3];
    bspline_grad(px, mx, wx, dx);
    bspline_grad(py, my, wy, dy);
    bspline_grad(pz, mz, wz, dz);
    if (nmask >= 0) {
        curl_potential_sums<PADDED, true, 0>(coef, n, nmask, off, mx, my, mz, wx, wy, wz, dx, dy, dz, s[0], s[1]);
        curl_potential_sums<PADDED, true, 1>(coef, n, nmask, off, mx, my, mz, wx, wy, wz, dx, dy, dz, s[2], s[3]);
        curl_potential_sums<PADDED, true, 2>(coef, n, nmask, off, mx, my, mz, wx, wy, wz, dx, dy, dz, s[4], s[5]);
    } else {
        curl_potential_sums<PADDED, false, 0>(coef, n, nmask, off, mx, my, mz, wx, wy, wz, dx, dy, dz, s[0], s[1]);
        curl_potential_sums<PADDED, false, 1>(coef, n, nmask, off, mx, my, mz, wx, wy, wz, dx, dy, dz, s[2], s[3]);
        curl_potential_sums<PADDED, false, 2>(coef, n, nmask, off, mx, my, mz, wx, wy, wz, dx, dy, dz, s[4], s[5]);
    }
}

// Each component of the curl is one float subtraction of two of the six sums.
WN_EVAL_FN void curl_of_sums(const float s[6], float v[3])
{
    v[0] = s[5] - s[3];
    v[1] = s[1] - s[4];
    v[2] = s[2] - s[0];
}

// curl at one point: every component has the bits of the subtraction of two channels of eval3d_grad_exact on the shifted
// tiles.
template <bool PADDED = false>
WN_EVAL_FN void eval3d_curl_exact(const float *coef, int n, int nmask, const int *off, float px, float py, float pz, float v[3])
{
    float s[6];
    eval3d_curl_sums<PADDED>(coef, n, nmask, off, px, py, pz, s);
    curl_of_sums(s, v);
}

// curl of the potentials psi_k = WMultibandNoise (normal == NULL branch) of T_k, with respect to p: each of the six sums
// accumulates (w[b] * (2 * 2^(first_band+b))) * its band's sum over the active bands and is divided by out_div when
// apply_div, as multiband_exact<.., GRAD> does for its gradient channels; then the subtractions.  The offsets are the same
// in every band.  `a` carries coef, n, nmask, off and the bands of wn::multiband_bands.  No active band: 0.
template <bool PADDED, typename A>
WN_EVAL_FN void multiband_curl_exact(const A &a, const float p[3], float v[3])
{
    float acc[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (int b = 0; b < a.nbands; ++b) {
        const float s = a.band_scale[b];
        float sb[6];
        eval3d_curl_sums<PADDED>(a.coef, a.n, a.nmask, a.off, 2.0f * p[0] * s, 2.0f * p[1] * s, 2.0f * p[2] * s, sb);
        const float f = a.band_w[b] * (2.0f * s);
        WN_UNROLL
        for (int i = 0; i < 6; ++i) acc[i] += f * sb[i];
    }
    if (a.apply_div) {
        WN_UNROLL
        for (int i = 0; i < 6; ++i) acc[i] /= a.out_div;
    }
    curl_of_sums(acc, v);
}

// ---- solid boundaries of that curl field (include/wnoise_bounded.h; absent from the reference) -----------------------------
// Bridson, Houriham and Nordenstam 2007: the potential is faded to zero towards a solid by a smooth ramp A of the distance
// to it, and the velocity is the curl of the faded potential, v = curl(A Psi) = A curl Psi + grad A x Psi: still
// divergence-free, and on a solid A -> 0 and grad A is parallel to the normal, so the normal component of v vanishes.
// O is wn_obstacle (kind, c[3], r, d0), or wn_obstacle2d (c[2]) for the 2-D field further down; this header includes neither.
// The wavelet fields are float32, the Perlin field float64; everything is unfused.
constexpr int kMaxObstacles = 16; // WN_MAX_OBSTACLES
constexpr int kObstacleSphere = 0, kObstacleContainer = 1, kObstacleHalfspace = 2;

// What is wrong with an obstacle list (the checks of include/wnoise_bounded.h and wnoise_bounded2d.h), or nullptr.  D: the
// dimension, 3 (wn_obstacle) or 2 (wn_obstacle2d: c has two components, and a sphere is a disc, a half-space a half-plane).
template <int D = 3, typename O>
inline const char *obstacle_fault(const O *obs, int nobs)
{
    static_assert(D == 2 || D == 3, "a plane or a volume");
    if (nobs < 0 || nobs > kMaxObstacles) return "nobs must be in 0..16";
    if (nobs && !obs) return "obstacles_host is NULL";
    for (int j = 0; j < nobs; ++j) {
        const O &o = obs[j];
        if (o.kind < kObstacleSphere || o.kind > kObstacleHalfspace) return "an obstacle's kind must be 0, 1 or 2";
        bool finite = std::isfinite(o.r) && std::isfinite(o.d0), zero = true;
        for (int c = 0; c < D; ++c) {
            finite = finite && std::isfinite(o.c[c]);
            zero = zero && o.c[c] == 0.0f;
        }
        if (!finite) return "an obstacle's c, r and d0 must be finite";
        if (!(o.d0 > 0.0f)) return "an obstacle's d0 must be > 0";
        if (o.kind != kObstacleHalfspace && !(o.r > 0.0f)) return "a sphere's or container's r must be > 0";
        if (o.kind == kObstacleHalfspace && zero) return "a half-space's normal must not be zero";
        for (const int r : o.reserved)
            if (r != 0) return "an obstacle's reserved fields must be 0";
    }
    return nullptr;
}

// The signed distance d of x to obstacle o (positive in the fluid) and its gradient nrm, in the scalar type T of the point:
// float for the wavelet fields (sqrtf), double for the Perlin field (include/wnoise_perlin_bounded.h: c, r and d0 are widened
// from float, which is exact, sqrt and / are IEEE double).
//     sphere, container  dx = x - c, l = sqrt((dx0*dx0 + dx1*dx1) + dx2*dx2), m = dx / l (0 when l == 0);
//                        sphere: d = l - r, nrm = m; container: d = r - l, nrm = -m
//     half-space         d = ((n0*x0 + n1*x1) + n2*x2) - o, nrm = n as given (not normalised: d is linear with gradient n)
// D == 2: the same with the third component dropped, l = sqrt(dx0*dx0 + dx1*dx1) and d = (n0*x0 + n1*x1) - o.
WN_EVAL_FN float ramp_sqrt(float x) { return sqrtf(x); }
WN_EVAL_FN double ramp_sqrt(double x) { return sqrt(x); }

template <int D = 3, typename T, typename O>
WN_EVAL_FN T obstacle_distance(const O &o, const T x[D], T nrm[D])
{
    if (o.kind == kObstacleHalfspace) {
        WN_UNROLL
        for (int c = 0; c < D; ++c) nrm[c] = (T)o.c[c];
        T dot = (T)o.c[0] * x[0] + (T)o.c[1] * x[1];
        if constexpr (D == 3) dot = dot + (T)o.c[2] * x[2];
        return dot - (T)o.r;
    }
    T dx[D];
    WN_UNROLL
    for (int c = 0; c < D; ++c) dx[c] = x[c] - (T)o.c[c];
    T l2 = dx[0] * dx[0] + dx[1] * dx[1];
    if constexpr (D == 3) l2 = l2 + dx[2] * dx[2];
    const T l = ramp_sqrt(l2);
    const bool solid = o.kind == kObstacleSphere;
    WN_UNROLL
    for (int c = 0; c < D; ++c) {
        const T m = l == T(0) ? T(0) : dx[c] / l;
        nrm[c] = solid ? m : -m;
    }
    return solid ? l - (T)o.r : (T)o.r - l;
}

// Where x lies, and for a near point the product A of the obstacles' ramps and its gradient G, in the type T of the point.
//     inside  some obstacle has d <= 0: v = 0
//     far     every obstacle has d >= d0: the unbounded field (A = 1, G = 0; the potential values are not needed)
//     near    every other point.  Obstacles in list order, those with d >= d0 skipped; Bridson's quintic of r = d / d0,
//             alpha = r * (1.875 + r2 * (-1.25 + r2 * 0.375)), r2 = r * r, and its derivative
//             dalpha = (1.875 * (q * q)) / d0, q = 1 - r2 (the constants are exact in float); per component
//             G = G * alpha + (A * dalpha) * nrm, then A = A * alpha.  Overlapping ramps multiply: A stays C1 across
//             every d = d0.
constexpr int kBoundFar = 0, kBoundNear = 1, kBoundInside = 2;
template <int D = 3, typename T, typename O>
WN_EVAL_FN int obstacle_ramp(const O *obs, int nobs, const T x[D], T &A, T G[D])
{
    A = T(1);
    WN_UNROLL
    for (int c = 0; c < D; ++c) G[c] = T(0);
    int where = kBoundFar;
    for (int j = 0; j < nobs; ++j) {
        T nrm[D];
        const T d = obstacle_distance<D>(obs[j], x, nrm);
        const T d0 = (T)obs[j].d0;
        if (d <= T(0)) return kBoundInside;
        if (d >= d0) continue;
        where = kBoundNear;
        const T r = d / d0;
        const T r2 = r * r;
        const T alpha = r * (T(1.875) + r2 * (T(-1.25) + r2 * T(0.375)));
        const T q = T(1) - r2;
        const T dalpha = (T(1.875) * (q * q)) / d0;
        const T ad = A * dalpha;
        WN_UNROLL
        for (int c = 0; c < D; ++c) G[c] = G[c] * alpha + ad * nrm[c];
        A = A * alpha;
    }
    return where;
}

// The three potential values at one point: psi[K] is the value sum of eval3d_exact_impl -- tap weight (w_x*w_y)*w_z,
// f2 -> f1 -> f0, unfused -- over the coefficients at potential K's offset indices: the bits of eval3d_exact on T_K.
template <bool PADDED, bool POW2, int K>
WN_EVAL_FN float curl_potential_value(const float *coef, int n, int nmask, const int *off, int mx, int my, int mz,
                                      const float *wx, const float *wy, const float *wz)
{
    const int stride = PADDED ? n + 2 : n;
    int cx[3], cy[3], cz[3];
    WN_UNROLL
    for (int f = 0; f < 3; ++f) {
        cx[f] = POW2 ? ((mx + f - 1 + off[3 * K]) & nmask) : dmod(mx + f - 1 + off[3 * K], n, -1);
        cy[f] = (POW2 ? ((my + f - 1 + off[3 * K + 1]) & nmask) : dmod(my + f - 1 + off[3 * K + 1], n, -1)) * stride;
        cz[f] = (POW2 ? ((mz + f - 1 + off[3 * K + 2]) & nmask) : dmod(mz + f - 1 + off[3 * K + 2], n, -1)) * stride * n;
    }
    float result = 0.0f;
    WN_UNROLL
    for (int fz = 0; fz < 3; ++fz)
        WN_UNROLL
        for (int fy = 0; fy < 3; ++fy) {
            float c[3];
            if (PADDED) {
                __builtin_memcpy(c, coef + cx[0] + cy[fy] + cz[fz], sizeof(c));
            } else {
                WN_UNROLL
                for (int fx = 0; fx < 3; ++fx) c[fx] = coef[cx[fx] + cy[fy] + cz[fz]];
            }
            WN_UNROLL
            for (int fx = 0; fx < 3; ++fx) {
                const float weight = wx[fx] * wy[fy] * wz[fz];
                result += weight * c[fx];
            }
        }
    return result;
}

template <bool PADDED = false>
WN_EVAL_FN void eval3d_potential_values(const float *coef, int n, int nmask, const int *off, float px, float py, float pz,
                                        float psi[3])
{
    if (n == 0) {
        psi[0] = psi[1] = psi[2] = 0.0f;
        return;
    }
    int mx, my, mz;
    float wx[3], wy[3], wz[3];
    bspline(px, mx, wx[0], wx[1], wx[2]);
    bspline(py, my, wy[0], wy[1], wy[2]);
    bspline(pz, mz, wz[0], wz[1], wz[2]);
    if (nmask >= 0) {
        psi[0] = curl_potential_value<PADDED, true, 0>(coef, n, nmask, off, mx, my, mz, wx, wy, wz);
        psi[1] = curl_potential_value<PADDED, true, 1>(coef, n, nmask, off, mx, my, mz, wx, wy, wz);
        psi[2] = curl_potential_value<PADDED, true, 2>(coef, n, nmask, off, mx, my, mz, wx, wy, wz);
    } else {
        psi[0] = curl_potential_value<PADDED, false, 0>(coef, n, nmask, off, mx, my, mz, wx, wy, wz);
        psi[1] = curl_potential_value<PADDED, false, 1>(coef, n, nmask, off, mx, my, mz, wx, wy, wz);
        psi[2] = curl_potential_value<PADDED, false, 2>(coef, n, nmask, off, mx, my, mz, wx, wy, wz);
    }
}

// The same of WMultibandNoise potentials: multiband_exact's value arm on T_K -- psi[K] += w[b] * (band b's value at
// q_b = 2 * p * 2^(first_band+b)), divided by out_div when apply_div.  No active band: 0.
template <bool PADDED, typename A>
WN_EVAL_FN void multiband_potential_values(const A &a, const float p[3], float psi[3])
{
    float acc[3] = {0.0f, 0.0f, 0.0f};
    for (int b = 0; b < a.nbands; ++b) {
        const float s = a.band_scale[b];
        float vb[3];
        eval3d_potential_values<PADDED>(a.coef, a.n, a.nmask, a.off, 2.0f * p[0] * s, 2.0f * p[1] * s, 2.0f * p[2] * s, vb);
        WN_UNROLL
        for (int k = 0; k < 3; ++k) acc[k] += a.band_w[b] * vb[k];
    }
    WN_UNROLL
    for (int k = 0; k < 3; ++k) psi[k] = a.apply_div ? acc[k] / a.out_div : acc[k];
}

// The bounded velocity at p from `where`, A, G of obstacle_ramp: curl(v) writes the unbounded curl c (its entry point's
// bits), values(psi) the potential values.  inside: 0.  far: c, and values is not called.  near:
// v = A * c + G x Psi, e.g. v0 = A * c0 + (G1 * psi2 - G2 * psi1), each operation rounded on its own.
template <typename T, typename Curl, typename Values>
WN_EVAL_FN void bounded_velocity(int where, T A, const T G[3], T v[3], const Curl &curl, const Values &values)
{
    if (where == kBoundInside) {
        v[0] = v[1] = v[2] = T(0);
        return;
    }
    curl(v);
    if (where == kBoundFar) return;
    T psi[3];
    values(psi);
    const T x0 = G[1] * psi[2] - G[2] * psi[1];
    const T x1 = G[2] * psi[0] - G[0] * psi[2];
    const T x2 = G[0] * psi[1] - G[1] * psi[0];
    v[0] = A * v[0] + x0;
    v[1] = A * v[1] + x1;
    v[2] = A * v[2] + x2;
}

// eval3d_curl_exact / multiband_curl_exact with the obstacles obs[0 .. nobs): nobs == 0 and far points carry their bits.
template <bool PADDED = false, typename O>
WN_EVAL_FN void eval3d_curl_bounded_exact(const float *coef, int n, int nmask, const int *off, const O *obs, int nobs,
                                          const float p[3], float v[3])
{
    float A, G[3];
    const int where = obstacle_ramp(obs, nobs, p, A, G);
    bounded_velocity(
        where, A, G, v, [&](float *c) { eval3d_curl_exact<PADDED>(coef, n, nmask, off, p[0], p[1], p[2], c); },
        [&](float *psi) { eval3d_potential_values<PADDED>(coef, n, nmask, off, p[0], p[1], p[2], psi); });
}

template <bool PADDED, typename E, typename O>
WN_EVAL_FN void multiband_curl_bounded_exact(const E &a, const O *obs, int nobs, const float p[3], float v[3])
{
    float A, G[3];
    const int where = obstacle_ramp(obs, nobs, p, A, G);
    bounded_velocity(
        where, A, G, v, [&](float *c) { multiband_curl_exact<PADDED>(a, p, c); },
        [&](float *psi) { multiband_potential_values<PADDED>(a, p, psi); });
}

// ---- solid boundaries and a background stream for the 2-D curl field (include/wnoise_bounded2d.h; absent from the reference) --
// In two dimensions the faded potential is a scalar: v = (d(A psi_t)/dy, -d(A psi_t)/dx) with psi_t the stream function of
// multiband2d_curl_exact plus, when flow != nullptr, the uniform stream psi_bg = ux * py - uy * px (Bridson's remedy: inside
// the potential the ramp bends the stream around a solid with the noise).  `where`, A, G: obstacle_ramp<2> at p.
//     psi, gx, gy   the three channels of multiband2d_footprint_exact<GRAD = true> at s with fade 0
//     flow          psi_t = psi + (ux * py - uy * px),  gx_t = gx - uy,  gy_t = gy + ux   (flow == nullptr: skipped)
//     inside        v = (0, 0), nothing is evaluated
//     far           v = (gy_t, -gx_t)
//     near          v0 = A * gy_t + G1 * psi_t,  v1 = -(A * gx_t + G0 * psi_t)
// `wide` picks the evaluator walk: true forms the value sum beside the two derivative sums, false is multiband2d_curl_exact
// alone, whose channels have the same bits as the derivative sums of the former (fade 0: the weight is w[b] * 1.0f).  A caller
// passes wide = true wherever psi is read (near, or flow != nullptr); it may pass true elsewhere too, and the kernels do so
// for a whole wave when any of its lanes needs it: no wave walks the nine taps twice.  The bits do not depend on `wide`.
template <bool PADDED = false, typename A>
WN_EVAL_FN void multiband2d_curl_bounded_at(const A &a, const float *coef, int where, float ramp, const float G[2],
                                            const float *flow, bool wide, const float p[2], float s, float v[2])
{
    if (where == kBoundInside) {
        v[0] = v[1] = 0.0f;
        return;
    }
    if (!wide) { // far, no stream: the unbounded field
        multiband2d_curl_exact<PADDED>(a, coef, p, s, v);
        return;
    }
    float g[2];
    float psi = multiband2d_footprint_exact<true, PADDED>(a, coef, p, s, g);
    if (flow) {
        const float a0 = flow[0] * p[1];
        const float a1 = flow[1] * p[0];
        psi = psi + (a0 - a1);
        g[0] = g[0] - flow[1];
        g[1] = g[1] + flow[0];
    }
    if (where == kBoundFar) {
        v[0] = g[1];
        v[1] = -g[0];
        return;
    }
    const float t0 = ramp * g[1];
    const float u0 = G[1] * psi;
    const float t1 = ramp * g[0];
    const float u1 = G[0] * psi;
    v[0] = t0 + u0;
    v[1] = -(t1 + u1);
}

// multiband2d_curl_exact with the obstacles obs[0 .. nobs) and the stream `flow` ({ux, uy}, or nullptr): nobs == 0 with
// flow == nullptr, and far points with flow == nullptr, carry its bits.  `a` must have fade == 0.
template <bool PADDED = false, typename A, typename O>
WN_EVAL_FN void multiband2d_curl_bounded_exact(const A &a, const float *coef, const O *obs, int nobs, const float *flow,
                                               const float p[2], float s, float v[2])
{
    float ramp, G[2];
    const int where = obstacle_ramp<2>(obs, nobs, p, ramp, G);
    multiband2d_curl_bounded_at<PADDED>(a, coef, where, ramp, G, flow, where == kBoundNear || flow != nullptr, p, s, v);
}

// ---- one explicit time step of a particle through a velocity field (include/wnoise_advect.h; absent from the reference) --
// METHOD: WN_ADVECT_EULER / _MIDPOINT / _RK4 (0, 1, 2).  D: the dimension, 3 (include/wnoise_advect.h,
// include/wnoise_perlin_advect.h) or 2 (include/wnoise_curl2d.h).  T: float (the wavelet potentials) or double (the Perlin
// potentials).  velocity(q, v) writes the field's v(q); the stage velocity is
// k(q) = gain * v(q) + drift, one multiply, then one add per component.  h2 = T(0.5) * h and h6 = h / T(6) come from the
// caller, formed once.  Every product and every sum below rounds on its own (in T, unfused), so p' has the bits of the same
// operations written out with separately rounded arithmetic of that type around the field's own entry point:
//     Euler     p' = p + h * k(p)
//     midpoint  p' = p + h * k(p + h2 * k1),                                  k1 = k(p)
//     RK4       p' = p + h6 * (((k1 + 2 * k2) + 2 * k3) + k4),                k2 = k(p + h2 * k1), k3 = k(p + h2 * k2),
//                                                                              k4 = k(p + h * k3)
// RK4 keeps one running sum of the stage velocities beside p and the stage point.
template <int METHOD, int D = 3, typename T, typename V>
WN_EVAL_FN void advect_step(T p[D], T h, T h2, T h6, T gain, const T drift[D], const V &velocity)
{
    static_assert(METHOD >= 0 && METHOD <= 2, "Euler, midpoint or RK4");
    static_assert(D == 2 || D == 3, "a plane or a volume");
    auto stage = [&](const T q[D], T k[D]) {
        T v[D];
        velocity(q, v);
        WN_UNROLL
        for (int c = 0; c < D; ++c) k[c] = gain * v[c] + drift[c];
    };
    auto from_p = [&](T f, const T k[D], T q[D]) {
        WN_UNROLL
        for (int c = 0; c < D; ++c) q[c] = p[c] + f * k[c];
    };
    T k[D], q[D];
    stage(p, k);
    if constexpr (METHOD == 1) {
        from_p(h2, k, q);
        stage(q, k);
    } else if constexpr (METHOD == 2) {
        T sum[D];
        WN_UNROLL
        for (int c = 0; c < D; ++c) sum[c] = k[c];
        from_p(h2, k, q);
        stage(q, k);
        WN_UNROLL
        for (int c = 0; c < D; ++c) sum[c] = sum[c] + T(2) * k[c];
        from_p(h2, k, q);
        stage(q, k);
        WN_UNROLL
        for (int c = 0; c < D; ++c) sum[c] = sum[c] + T(2) * k[c];
        from_p(h, k, q);
        stage(q, k);
        WN_UNROLL
        for (int c = 0; c < D; ++c) k[c] = sum[c] + k[c];
    }
    from_p(METHOD == 2 ? h6 : h, k, p);
}

// ---- Perlin improved noise, fp64 (perlin.h:18-31, 42-62) ------------------------------------------
WN_EVAL_FN double pfade(double t) { return t * t * t * (t * (t * 6 - 15) + 10); }
WN_EVAL_FN double plerp(double t, double a, double b) { return a + t * (b - a); }
WN_EVAL_FN double pgrad(int hash, double x, double y, double z)
{
    const int h = hash & 15;
    const double u = h < 8 ? x : y;
    const double v = h < 4 ? y : ((h == 12 || h == 14) ? x : z);
    return ((h & 1) == 0 ? u : -u) + ((h & 2) == 0 ? v : -v);
}

// `perm` is the 512-entry table (values 0..255; every index the algorithm forms is <= 511, perlin.h:55-61): bytes in LDS
// or global memory on the device, the reference's `const int *` on the host.
template <typename Table>
WN_EVAL_FN double perlin_exact(const Table perm, double x, double y, double z)
{
    const double fx = floor(x), fy = floor(y), fz = floor(z);
    const int X = (int)fx & 255, Y = (int)fy & 255, Z = (int)fz & 255;
    x -= fx;
    y -= fy;
    z -= fz;
    const double u = pfade(x), v = pfade(y), w = pfade(z);
    const int A = perm[X] + Y, AA = perm[A] + Z, AB = perm[A + 1] + Z;
    const int B = perm[X + 1] + Y, BA = perm[B] + Z, BB = perm[B + 1] + Z;
    const double x00 = plerp(u, pgrad(perm[AA], x, y, z), pgrad(perm[BA], x - 1, y, z));
    const double x10 = plerp(u, pgrad(perm[AB], x, y - 1, z), pgrad(perm[BB], x - 1, y - 1, z));
    const double x01 = plerp(u, pgrad(perm[AA + 1], x, y, z - 1), pgrad(perm[BA + 1], x - 1, y, z - 1));
    const double x11 = plerp(u, pgrad(perm[AB + 1], x, y - 1, z - 1), pgrad(perm[BB + 1], x - 1, y - 1, z - 1));
    return plerp(w, plerp(v, x00, x10), plerp(v, x01, x11));
}

// RTOW turb on a float vec3 (absent from the reference): weight halves, point doubles in float.
template <typename Table>
WN_EVAL_FN double perlin_turb(const Table perm, float x, float y, float z, int depth)
{
    double accum = 0.0, weight = 1.0;
    for (int i = 0; i < depth; ++i) {
        accum += weight * perlin_exact(perm, (double)x, (double)y, (double)z);
        weight *= 0.5;
        x *= 2.0f;
        y *= 2.0f;
        z *= 2.0f;
    }
    return fabs(accum);
}

// perlin::fractal_noise, perlin.h:75-90 (float point times double frequency).
template <typename Table>
WN_EVAL_FN double perlin_fractal(const Table perm, float x, float y, float z)
{
    double result = 0.0, amplitude = 1.0, frequency = 1.0, max_value = 0.0;
    for (int i = 0; i < 6; ++i) {
        result += perlin_exact(perm, x * frequency, y * frequency, z * frequency) * amplitude;
        max_value += amplitude;
        amplitude *= 0.5;
        frequency *= 2.0;
    }
    return result / max_value;
}

// ---- analytic gradient of Perlin noise, turb and fractal_noise (absent from the reference) -----------------------------
// noise(p) = trilinear blend, weights fade(xf), fade(yf), fade(zf), of the eight corner dot products a_c = G_c . (p - c),
// c = cx + 2 cy + 4 cz in the value's order (AA, BA, AB, BB, AA+1, ...).  With u, v, w the fades and x00 .. x11, y0, y1 the
// value's own intermediates:
//     d/dx = T_x + fade'(xf) * lerp(w, lerp(v, a1 - a0, a3 - a2), lerp(v, a5 - a4, a7 - a6))
//     d/dy = T_y + fade'(yf) * lerp(w, x10 - x00, x11 - x01)
//     d/dz = T_z + fade'(zf) * (y1 - y0)
// T_k is the trilinear blend of the eight G_c[k].  The order of the gradient channels is this library's to define (the
// reference has none): the corner components are blended over z, then y -- P0_k, P1_k of perlin_corner_blend, constant
// along a run of x samples inside one cell, so the dense-grid run kernel forms them once per cell and row -- and over x
// last, T_k = plerp(u, P0_k, P1_k).  Every product and sum unfused, as everywhere in this file.
WN_EVAL_FN double pfade_d(double t) // fade'(t) = 30 t^2 (t - 1)^2
{
    const double s = t * (t - 1.0);
    return 30.0 * (s * s);
}

// grad()'s corner vector G (perlin.h:26-31): pgrad(hash, x, y, z) = G . (x, y, z), components in {-1, 0, 1}.
// u = h < 8 ? x : y carries the sign of bit 0, v = h < 4 ? y : (h == 12 || h == 14 ? x : z) that of bit 1.
constexpr int pgrad_component(int h, int k)
{
    const int uk = h < 8 ? 0 : 1, vk = h < 4 ? 1 : ((h == 12 || h == 14) ? 0 : 2);
    return (uk == k ? ((h & 1) ? -1 : 1) : 0) + (vk == k ? ((h & 2) ? -1 : 1) : 0);
}
// component + 1 of the 16 hashes, two bits each: one shift and mask instead of a tree of selects
constexpr uint32_t pgrad_lut(int k)
{
    uint32_t lut = 0;
    for (int h = 0; h < 16; ++h) lut |= (uint32_t)(pgrad_component(h, k) + 1) << (2 * h);
    return lut;
}
WN_EVAL_FN double pgrad_decode(uint32_t lut, int hash) { return (double)((int)((lut >> (2 * (hash & 15))) & 3u) - 1); }

// The corner vectors of one cell blended over z, then y: P0 for the corners at cx = 0, P1 for cx = 1.
WN_EVAL_FN void perlin_corner_blend(const int h[8], double v, double w, double P0[3], double P1[3])
{
    constexpr uint32_t lut[3] = {pgrad_lut(0), pgrad_lut(1), pgrad_lut(2)};
    WN_UNROLL
    for (int k = 0; k < 3; ++k) {
        double G[8];
        WN_UNROLL
        for (int c = 0; c < 8; ++c) G[c] = pgrad_decode(lut[k], h[c]);
        P0[k] = plerp(v, plerp(w, G[0], G[4]), plerp(w, G[2], G[6]));
        P1[k] = plerp(v, plerp(w, G[1], G[5]), plerp(w, G[3], G[7]));
    }
}

// One sample from its eight corner dot products: returns the value in perlin_exact's operations (the same bits), writes
// the gradient to g.  du, dv, dw = fade'(xf), fade'(yf), fade'(zf).
WN_EVAL_FN double perlin_sample_grad(const double a[8], double u, double v, double w, double du, double dv, double dw,
                                     const double P0[3], const double P1[3], double g[3])
{
    const double x00 = plerp(u, a[0], a[1]), x10 = plerp(u, a[2], a[3]);
    const double x01 = plerp(u, a[4], a[5]), x11 = plerp(u, a[6], a[7]);
    const double y0 = plerp(v, x00, x10), y1 = plerp(v, x01, x11);
    const double dx = plerp(w, plerp(v, a[1] - a[0], a[3] - a[2]), plerp(v, a[5] - a[4], a[7] - a[6]));
    const double dy = plerp(w, x10 - x00, x11 - x01);
    g[0] = plerp(u, P0[0], P1[0]) + du * dx;
    g[1] = plerp(u, P0[1], P1[1]) + dv * dy;
    g[2] = plerp(u, P0[2], P1[2]) + dw * (y1 - y0);
    return plerp(w, y0, y1);
}

// perlin::noise and its gradient: returns the value (perlin_exact's bits), writes d/dx, d/dy, d/dz to g.
template <typename Table>
WN_EVAL_FN double perlin_grad_exact(const Table perm, double x, double y, double z, double g[3])
{
    const double fx = floor(x), fy = floor(y), fz = floor(z);
    const int X = (int)fx & 255, Y = (int)fy & 255, Z = (int)fz & 255;
    x -= fx;
    y -= fy;
    z -= fz;
    const double u = pfade(x), v = pfade(y), w = pfade(z);
    const int A = perm[X] + Y, AA = perm[A] + Z, AB = perm[A + 1] + Z;
    const int B = perm[X + 1] + Y, BA = perm[B] + Z, BB = perm[B + 1] + Z;
    const int h[8] = {(int)perm[AA],     (int)perm[BA],     (int)perm[AB],     (int)perm[BB],
                      (int)perm[AA + 1], (int)perm[BA + 1], (int)perm[AB + 1], (int)perm[BB + 1]};
    const double a[8] = {pgrad(h[0], x, y, z),         pgrad(h[1], x - 1, y, z),
                         pgrad(h[2], x, y - 1, z),     pgrad(h[3], x - 1, y - 1, z),
                         pgrad(h[4], x, y, z - 1),     pgrad(h[5], x - 1, y, z - 1),
                         pgrad(h[6], x, y - 1, z - 1), pgrad(h[7], x - 1, y - 1, z - 1)};
    double P0[3], P1[3];
    perlin_corner_blend(h, v, w, P0, P1);
    return perlin_sample_grad(a, u, v, w, pfade_d(x), pfade_d(y), pfade_d(z), P0, P1, g);
}

// turb and its gradient with respect to the float point.  Octave i evaluates noise at 2^i p (an exact doubling) with weight
// 2^-i: the chain-rule factor 2^-i * 2^i is exactly 1, so the gradient is the plain sum of the octaves' noise gradients, in
// octave order, times sigma = -1 where the value's own accumulated sum is negative and +1 otherwise.  Not differentiable
// where that sum is 0 (the kink of |.|): sigma = +1 there.  depth == 0: 0 in all four channels.
template <typename Table>
WN_EVAL_FN double perlin_turb_grad(const Table perm, float x, float y, float z, int depth, double g[3])
{
    double accum = 0.0, weight = 1.0, gx = 0.0, gy = 0.0, gz = 0.0;
    for (int i = 0; i < depth; ++i) {
        double gn[3];
        accum += weight * perlin_grad_exact(perm, (double)x, (double)y, (double)z, gn);
        gx += gn[0];
        gy += gn[1];
        gz += gn[2];
        weight *= 0.5;
        x *= 2.0f;
        y *= 2.0f;
        z *= 2.0f;
    }
    const bool negative = accum < 0.0;
    g[0] = negative ? -gx : gx;
    g[1] = negative ? -gy : gy;
    g[2] = negative ? -gz : gz;
    return fabs(accum);
}

// fractal_noise and its gradient: amplitude 2^-i times frequency 2^i is exactly 1, so the gradient is the plain sum of the
// six octaves' noise gradients divided by the value's max_value.
template <typename Table>
WN_EVAL_FN double perlin_fractal_grad(const Table perm, float x, float y, float z, double g[3])
{
    double result = 0.0, amplitude = 1.0, frequency = 1.0, max_value = 0.0, gx = 0.0, gy = 0.0, gz = 0.0;
    for (int i = 0; i < 6; ++i) {
        double gn[3];
        result += perlin_grad_exact(perm, x * frequency, y * frequency, z * frequency, gn) * amplitude;
        gx += gn[0];
        gy += gn[1];
        gz += gn[2];
        max_value += amplitude;
        amplitude *= 0.5;
        frequency *= 2.0;
    }
    g[0] = gx / max_value;
    g[1] = gy / max_value;
    g[2] = gz / max_value;
    return result / max_value;
}

// ---- turb and fractal_noise with the octave limit taken from a footprint per sample (include/wnoise_perlin_footprint.h) ----
// Clamping the octave sum by the filter width is the classical way to antialias Perlin noise.  For a sample with footprint s
// (log2 of the footprint in the noise space of p) and octave i in 0 .. octaves-1:
//     t_i = (s + bias) + (float)i, in float and in this association;
//     octave i is active iff t_i < 0; t_i does not decrease with i, so the first octave that fails ends the loop
//         (a NaN or +inf s: no octave; -inf: all of them);
//     f_i = 1.0f with fade == 0 (a hard cut), fminf(1.0f, -t_i) with fade != 0: the finest surviving octave fades in over
//         one octave of footprint.
// Octave i has cells of size 2^-i: bias = 0 cuts an octave when the footprint reaches one cell, bias = -1 at two cells --
// the rule wn_multiband3d_footprint_points applies to its bands (band b has cells of 2^-(b+1) in p; it runs while
// s + b < 0).  Where f_i == 1 for every active octave the products with f_i are exact: a turb sample with k active octaves
// then has the bits of perlin_turb / perlin_turb_grad at depth k, a fractal sample with octaves == 6 and all six active
// those of perlin_fractal / perlin_fractal_grad.
constexpr int kPerlinFootprintMaxOctaves = 16; // depth / octaves of the footprint entry points: 0 .. 16

WN_EVAL_FN float perlin_footprint_t(float s, float bias, int i) { return (s + bias) + (float)i; }
WN_EVAL_FN double perlin_footprint_factor(float t, int fade) { return (double)(fade ? fminf(1.0f, -t) : 1.0f); }
// the number of active octaves (what the sorted kernel bins by; the evaluators below run the same test octave by octave)
WN_EVAL_FN int perlin_footprint_count(float s, float bias, int octaves)
{
    int k = 0;
    while (k < octaves && perlin_footprint_t(s, bias, k) < 0.0f) ++k;
    return k;
}

// perlin_turb's arithmetic (the float point doubles per octave, weight halves) with accum += (weight * f_i) * noise; the
// value is fabs(accum).  GRAD: g += f_i * grad noise in octave order, times perlin_turb_grad's sign rule on the value's own
// accum.  No active octave: +0 in all four channels.
template <bool GRAD, typename Table>
WN_EVAL_FN double perlin_turb_footprint(const Table perm, float x, float y, float z, int depth, float s, float bias, int fade,
                                        double *g)
{
    double accum = 0.0, weight = 1.0, gx = 0.0, gy = 0.0, gz = 0.0;
    for (int i = 0; i < depth; ++i) {
        const float t = perlin_footprint_t(s, bias, i);
        if (!(t < 0.0f)) break;
        const double f = perlin_footprint_factor(t, fade);
        if constexpr (GRAD) {
            double gn[3];
            accum += (weight * f) * perlin_grad_exact(perm, (double)x, (double)y, (double)z, gn);
            gx += f * gn[0];
            gy += f * gn[1];
            gz += f * gn[2];
        } else {
            accum += (weight * f) * perlin_exact(perm, (double)x, (double)y, (double)z);
        }
        weight *= 0.5;
        x *= 2.0f;
        y *= 2.0f;
        z *= 2.0f;
    }
    if constexpr (GRAD) {
        const bool negative = accum < 0.0;
        g[0] = negative ? -gx : gx;
        g[1] = negative ? -gy : gy;
        g[2] = negative ? -gz : gz;
    }
    return fabs(accum);
}

// perlin_fractal's arithmetic (float point times double frequency) for `octaves` octaves with
// result += noise * (amplitude * f_i).  max_value is the sum of the amplitudes of ALL `octaves` octaves, however many run
// (as out_div of multiband_footprint_exact: dropping an octave drops its energy, nothing is renormalised); every partial
// sum of it is exact.  Value: result / max_value; GRAD: (sum_i f_i * grad noise) / max_value.  octaves == 0: 0 in every
// channel and no division.
template <bool GRAD, typename Table>
WN_EVAL_FN double perlin_fractal_footprint(const Table perm, float x, float y, float z, int octaves, float s, float bias,
                                           int fade, double *g)
{
    double result = 0.0, amplitude = 1.0, frequency = 1.0, max_value = 0.0, gx = 0.0, gy = 0.0, gz = 0.0;
    int i = 0;
    for (; i < octaves; ++i) {
        const float t = perlin_footprint_t(s, bias, i);
        if (!(t < 0.0f)) break;
        const double f = perlin_footprint_factor(t, fade);
        if constexpr (GRAD) {
            double gn[3];
            result += perlin_grad_exact(perm, x * frequency, y * frequency, z * frequency, gn) * (amplitude * f);
            gx += f * gn[0];
            gy += f * gn[1];
            gz += f * gn[2];
        } else {
            result += perlin_exact(perm, x * frequency, y * frequency, z * frequency) * (amplitude * f);
        }
        max_value += amplitude;
        amplitude *= 0.5;
        frequency *= 2.0;
    }
    for (; i < octaves; ++i) { // the octaves that do not run still count
        max_value += amplitude;
        amplitude *= 0.5;
    }
    if (octaves <= 0) {
        if constexpr (GRAD) g[0] = g[1] = g[2] = 0.0;
        return 0.0;
    }
    if constexpr (GRAD) {
        g[0] = gx / max_value;
        g[1] = gy / max_value;
        g[2] = gz / max_value;
    }
    return result / max_value;
}

// ---- curl of three Perlin potentials (include/wnoise_perlin_curl.h; absent from the reference) --------------------------
// psi_k is noise / the signed turb sum / fractal_noise with the cell index shifted by off[3k .. 3k+2] (any integers, taken
// & 255).  Of each potential's gradient two partials enter the curl; s holds the six in the order
//     {d psi0/dy, d psi0/dz, d psi1/dx, d psi1/dz, d psi2/dx, d psi2/dy}.
// One octave at the double point (x, y, z): floor, fractional parts, fade and fade' once, the hashes three times, each
// partial from perlin_sample_grad's own expression (the third partial is unused and not computed).
// ADD: s += the octave's partials (turb, fractal_noise); else s = them (noise).
// VALUES: the value perlin_sample_grad returns -- perlin_exact's bits on the shifted hashes -- enters psi as well:
// psi[k] = value (noise), psi[k] += weight * value (ADD: perlin_turb's accum += weight * noise, and perlin_fractal's
// result += noise * amplitude, the same product).  Without VALUES the value is not computed and psi is not read.  The
// partials are the same expressions either way, so their bits do not depend on the flag.
template <bool ADD, bool VALUES = false, typename Table>
WN_EVAL_FN void perlin_curl_octave(const Table perm, double x, double y, double z, const int *off, double s[6],
                                   double *psi = nullptr, double weight = 1.0)
{
    const double fx = floor(x), fy = floor(y), fz = floor(z);
    const int X = (int)fx & 255, Y = (int)fy & 255, Z = (int)fz & 255;
    x -= fx;
    y -= fy;
    z -= fz;
    const double u = pfade(x), v = pfade(y), w = pfade(z);
    const double du = pfade_d(x), dv = pfade_d(y), dw = pfade_d(z);
    WN_UNROLL
    for (int k = 0; k < 3; ++k) {
        const int Xk = (X + (off[3 * k] & 255)) & 255, Yk = (Y + (off[3 * k + 1] & 255)) & 255,
                  Zk = (Z + (off[3 * k + 2] & 255)) & 255;
        const int A = perm[Xk] + Yk, AA = perm[A] + Zk, AB = perm[A + 1] + Zk;
        const int B = perm[Xk + 1] + Yk, BA = perm[B] + Zk, BB = perm[B + 1] + Zk;
        const int h[8] = {(int)perm[AA],     (int)perm[BA],     (int)perm[AB],     (int)perm[BB],
                          (int)perm[AA + 1], (int)perm[BA + 1], (int)perm[AB + 1], (int)perm[BB + 1]};
        const double a[8] = {pgrad(h[0], x, y, z),         pgrad(h[1], x - 1, y, z),
                             pgrad(h[2], x, y - 1, z),     pgrad(h[3], x - 1, y - 1, z),
                             pgrad(h[4], x, y, z - 1),     pgrad(h[5], x - 1, y, z - 1),
                             pgrad(h[6], x, y - 1, z - 1), pgrad(h[7], x - 1, y - 1, z - 1)};
        double P0[3], P1[3], g[3];
        perlin_corner_blend(h, v, w, P0, P1);
        const double value = perlin_sample_grad(a, u, v, w, du, dv, dw, P0, P1, g);
        const double first = g[k == 0 ? 1 : 0], second = g[k == 2 ? 1 : 2];
        s[2 * k] = ADD ? s[2 * k] + first : first;
        s[2 * k + 1] = ADD ? s[2 * k + 1] + second : second;
        if constexpr (VALUES) psi[k] = ADD ? psi[k] + weight * value : value;
    }
}

// v = (d psi2/dy - d psi1/dz, d psi0/dz - d psi2/dx, d psi1/dx - d psi0/dy): one subtraction per component.
WN_EVAL_FN void perlin_curl_of(const double s[6], double v[3])
{
    v[0] = s[5] - s[3];
    v[1] = s[1] - s[4];
    v[2] = s[2] - s[0];
}

// The three fields as one walk over their octaves, which gives the curl and, with VALUES, the potential values
// Psi = (psi0, psi1, psi2) as well (include/wnoise_perlin_bounded.h).
//
// The curl of three perlin::noise potentials: each component has the bits of the subtraction of two perlin_grad_exact
// channels on the shifted cells; psi_k those of perlin_exact on them.
template <bool VALUES, typename Table>
WN_EVAL_FN void perlin_curl_walk(const Table perm, double x, double y, double z, const int *off, double v[3], double *psi)
{
    double s[6];
    perlin_curl_octave<false, VALUES>(perm, x, y, z, off, s, psi);
    perlin_curl_of(s, v);
}

// ... of three turb potentials WITHOUT the final fabs (|.| is not differentiable, and the curl of |S| is not
// divergence-free where S = 0): psi_k = sum_i 2^-i noise_k(2^i p), accumulated as perlin_turb accumulates it.  Each
// partial is the plain sum of the octaves' noise partials in octave order, as in perlin_turb_grad, without its sign.  The
// offsets act on every octave's own cell index.  depth == 0: 0 in all three components and in Psi.
template <bool VALUES, typename Table>
WN_EVAL_FN void perlin_turb_curl_walk(const Table perm, float x, float y, float z, int depth, const int *off, double v[3],
                                      double *psi)
{
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double weight = 1.0;
    if constexpr (VALUES) psi[0] = psi[1] = psi[2] = 0.0;
    for (int i = 0; i < depth; ++i) {
        perlin_curl_octave<true, VALUES>(perm, (double)x, (double)y, (double)z, off, s, psi, weight);
        if constexpr (VALUES) weight *= 0.5;
        x *= 2.0f;
        y *= 2.0f;
        z *= 2.0f;
    }
    perlin_curl_of(s, v);
}

// ... of three fractal_noise potentials: each partial is (sum of the six octaves' noise partials) / max_value, as
// perlin_fractal_grad forms it; psi_k is perlin_fractal's result / max_value.
template <bool VALUES, typename Table>
WN_EVAL_FN void perlin_fractal_curl_walk(const Table perm, float x, float y, float z, const int *off, double v[3], double *psi)
{
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double amplitude = 1.0, frequency = 1.0, max_value = 0.0;
    if constexpr (VALUES) psi[0] = psi[1] = psi[2] = 0.0;
    for (int i = 0; i < 6; ++i) {
        perlin_curl_octave<true, VALUES>(perm, x * frequency, y * frequency, z * frequency, off, s, psi, amplitude);
        max_value += amplitude;
        amplitude *= 0.5;
        frequency *= 2.0;
    }
    WN_UNROLL
    for (int j = 0; j < 6; ++j) s[j] = s[j] / max_value;
    if constexpr (VALUES) {
        WN_UNROLL
        for (int k = 0; k < 3; ++k) psi[k] = psi[k] / max_value;
    }
    perlin_curl_of(s, v);
}

// The curl alone (wn_perlin_curl_points, _points_vec3, the grids' generic kernel, advection): the walks without values.
template <typename Table>
WN_EVAL_FN void perlin_curl_exact(const Table perm, double x, double y, double z, const int *off, double v[3])
{
    perlin_curl_walk<false>(perm, x, y, z, off, v, nullptr);
}
template <typename Table>
WN_EVAL_FN void perlin_turb_curl(const Table perm, float x, float y, float z, int depth, const int *off, double v[3])
{
    perlin_turb_curl_walk<false>(perm, x, y, z, depth, off, v, nullptr);
}
template <typename Table>
WN_EVAL_FN void perlin_fractal_curl(const Table perm, float x, float y, float z, const int *off, double v[3])
{
    perlin_fractal_curl_walk<false>(perm, x, y, z, off, v, nullptr);
}

// ---- solid boundaries of that curl field (include/wnoise_perlin_bounded.h; absent from the reference) -------------------
// `kind`: 0 noise, 1 turb, 2 fractal_noise (WN_PERLIN_CURL_*).  The point type P is double (wn_perlin_curl_points: noise
// only) or float (wn_perlin_curl_points_vec3: noise widens it, turb and fractal_noise take it as it is).
template <int KIND, bool VALUES, typename P, typename Table>
WN_EVAL_FN void perlin_curl_kind_walk(const Table perm, P x, P y, P z, int depth, const int *off, double v[3], double *psi)
{
    static_assert(KIND >= 0 && KIND <= 2, "noise, turb or fractal_noise");
    if constexpr (KIND == 0) perlin_curl_walk<VALUES>(perm, (double)x, (double)y, (double)z, off, v, psi);
    else if constexpr (KIND == 1) perlin_turb_curl_walk<VALUES>(perm, (float)x, (float)y, (float)z, depth, off, v, psi);
    else perlin_fractal_curl_walk<VALUES>(perm, (float)x, (float)y, (float)z, off, v, psi);
}

// The potential values alone: the walk above with its partials unused.
template <int KIND, typename P, typename Table>
WN_EVAL_FN void perlin_curl_potential(const Table perm, P x, P y, P z, int depth, const int *off, double psi[3])
{
    double v[3];
    perlin_curl_kind_walk<KIND, true>(perm, x, y, z, depth, off, v, psi);
}

// The bounded velocity at the point the evaluator receives: the ramp (obstacle_ramp in double) at that point widened to
// double, then bounded_velocity around ONE walk.  An inside point evaluates nothing; every other point takes the VALUES
// walk, whose partials are those of the plain walk, so a far point and nobs == 0 carry the unbounded entry point's bits and
// a near point composes the bits of the curl and potential entry points.  The value costs two lerps and one product-sum per
// potential and octave beside the six partials, which is why a far lane is not given a walk of its own.
template <int KIND, typename P, typename Table, typename O>
WN_EVAL_FN void perlin_curl_bounded(const Table perm, P x, P y, P z, int depth, const int *off, const O *obs, int nobs,
                                    double v[3])
{
    const double q[3] = {(double)x, (double)y, (double)z};
    double A, G[3], walked[3];
    const int where = obstacle_ramp(obs, nobs, q, A, G);
    bounded_velocity(
        where, A, G, v, [&](double *c) { perlin_curl_kind_walk<KIND, true>(perm, x, y, z, depth, off, c, walked); },
        [&](double *psi) {
            WN_UNROLL
            for (int k = 0; k < 3; ++k) psi[k] = walked[k];
        });
}

// ---- the texture adaptors' per-point arithmetic (texture.h:37-43, 67-107) ----------------------------------------------
// wavelet_texture's coordinate scaling, texture.h:71-80: (float)(p * scale) * (octave_scale * 2.0f)
template <typename A>
WN_EVAL_FN float wavelet_texture_coord(const A &a, float p)
{
    float c = (float)((double)p * a.scale);
    c *= a.octave_mul;
    return c;
}

// wavelet_texture's grey level of a normalised noise value v, texture.h:104-106
WN_EVAL_FN float wavelet_texture_grey(double v)
{
    const double q = v / 4.0;
    const double c = (q < -1.0) ? -1.0 : ((1.0 < q) ? 1.0 : q); // std::clamp
    return (float)(0.5 * (1.0 + c));
}

// wavelet_texture::value, texture.h:67-107.  `A` carries coef, n, nmask, mode (3: evaluate3D branch,
// 2: evaluate2D branch, 0: no tile -> texture.h:100-102), scale (double), octave_mul (octave_scale * 2.0f,
// :77-80) and inv_stddev (1/sqrt(0.18402f) or 1/sqrt(0.19686f), :84,98).
template <bool PADDED, typename A>
WN_EVAL_FN float wavelet_texture_value(const A &a, float px, float py, float pz)
{
    double v = 0.0;
    if (a.mode == 3) {
        v = (double)eval3d_exact<PADDED>(a.coef, a.n, a.nmask, wavelet_texture_coord(a, px), wavelet_texture_coord(a, py),
                                         wavelet_texture_coord(a, pz));
        v *= (double)a.inv_stddev;
    } else if (a.mode == 2) {
        v = (double)eval2d_exact(a.coef, a.n, a.nmask, wavelet_texture_coord(a, px), wavelet_texture_coord(a, py));
        v *= (double)a.inv_stddev;
    }
    return wavelet_texture_grey(v);
}

// wavelet_multiband_texture (absent from the reference): texture.h:71-75's coordinate without the octave multiply,
// pos = (float)((double)p * scale) per axis; WMultibandNoise(pos, s) as multiband_footprint_exact forms it, promoted to
// double; wavelet_texture's grey level.  s is the footprint in noise space (after scale).  An empty tile: 0.5.
// `a` carries coef, n, nmask, a FootprintBands and scale (double).
template <bool PADDED, typename A>
WN_EVAL_FN float wavelet_multiband_texture_value(const A &a, float px, float py, float pz, float s)
{
    const float pos[3] = {(float)((double)px * a.scale), (float)((double)py * a.scale), (float)((double)pz * a.scale)};
    return wavelet_texture_grey((double)multiband_footprint_exact<PADDED, false, false>(a, pos, nullptr, s, nullptr));
}

// noise_texture::value, texture.h:37-43: scaled_p = p * scale * octave_scale in float (vec3 * float,
// vec3.h:82-84), noise in fp64, 0.5 * (1 + n).
template <typename Table>
WN_EVAL_FN float noise_texture_value(const Table perm, float fscale, float octave_scale, float px, float py, float pz)
{
    const float sx = (fscale * px) * octave_scale;
    const float sy = (fscale * py) * octave_scale;
    const float sz = (fscale * pz) * octave_scale;
    double v = perlin_exact(perm, (double)sx, (double)sy, (double)sz);
    v = 0.5 * (1.0 + v);
    return (float)v;
}

// noise_multiband_texture (absent from the reference): the point scaled per axis in float, pos = fscale * p, as
// noise_texture_value scales it but without the octave factor; n = perlin_fractal_footprint(pos, s); 0.5 * (1 + n).  s is
// the footprint in noise space (after scale).
template <typename Table>
WN_EVAL_FN float noise_multiband_texture_value(const Table perm, float fscale, int octaves, float bias, int fade, float px,
                                               float py, float pz, float s)
{
    const double n = perlin_fractal_footprint<false>(perm, fscale * px, fscale * py, fscale * pz, octaves, s, bias, fade, nullptr);
    return (float)(0.5 * (1.0 + n));
}

} // namespace wn
