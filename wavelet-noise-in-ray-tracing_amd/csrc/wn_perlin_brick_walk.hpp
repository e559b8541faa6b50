// wn_perlin_brick_walk.hpp -- what the Perlin brick kernels share between a brick's triple and its finish: the octave
// tabulation, the wave-uniform segment loop over the x cells and the per-potential corner / sample body, as a function
// template over the field.  wn_perlin_bounded_bricks.hip (the curl with solid boundaries, which also needs the potential
// values) calls it.  wn_perlin_bricks.hip (value, gradient and curl bricks) takes the enumerators and the axis slice from
// here and holds the same walk as text of its own: calling the template from its nine kernels changes their register
// allocation and costs the turb and fractal_noise curl their second wave per SIMD.  A change to the walk is
// made in both places.  The field is a compile-time parameter:
//     kValue    1 sum per sample    the value
//     kGrad     4                   value, d/dx, d/dy, d/dz
//     kCurl     6                   the two partials of each of the three shifted potentials, wn::perlin_curl_octave's order
//     kCurlPsi  9                   those six, then the three potential values psi0, psi1, psi2, accumulated as
//                                   wn::perlin_curl_octave<.., VALUES = true> accumulates them (psi + weight * value)
// The frame is that of wn_perlin_bricks.hip's header comment: one wave per brick, lane ly + 8 lz owns the row of 8 x samples,
// lanes 0..23 tabulate one octave of the brick's axis indices in the wave's LDS slice, the x-cell walk is wave-uniform, the
// sums are fp64 in the reference's accumulation order, unfused.  Each kernel keeps what is its own: the LDS it declares, the
// brick loop, the finish and the stores.
#pragma once

#include "wn_perlin_frame.hpp"
#include "wn_brick_list.hpp"

#include <type_traits>

namespace wn {

enum { kValue = 0, kGrad = 1, kCurl = 2, kCurlPsi = 3 }; // the field of a walk
constexpr int field_sums(int field) { return field == kValue ? 1 : (field == kGrad ? 4 : (field == kCurl ? 6 : 9)); } // running sums per sample
constexpr int field_potentials(int field) { return (field == kCurl || field == kCurlPsi) ? 3 : 1; }

constexpr int kBrickAxisEntries = 3 * kBrickEdge; // x, y, z indices of a brick

// A wave's axis tables of one octave: entries 0..7 x, 8..15 y, 16..23 z.
struct BrickAxisSlice {
    RunAxisEntryD e[kBrickAxisEntries];
    uint8_t cell[kBrickAxisEntries];
};

// The first checks of wn_perlin_curl_bricks and of wn_perlin_curl_bounded_bricks, in this order and with these messages: kind,
// turb's depth, the table (check_perm names the dense entry point's checks, "perlin curl grid"), the grid, the offsets.
inline int perlin_curl_bricks_checks(const wn_perm *perm, const wn_grid *grid, int kind, int depth, const int32_t *offsets9_host)
{
    if (kind < kNoise || kind > kFractal) return fail(WN_ERR_INVALID, "kind must be 0 (noise), 1 (turb) or 2 (fractal_noise)");
    if (kind == kTurb && depth < 0) return fail(WN_ERR_INVALID, "depth must be >= 0");
    int rc = check_perm(perm, "perlin curl grid");
    if (rc) return rc;
    GridArgs checked;
    if ((rc = check_grid(grid, true, &checked)) != WN_OK) return rc;
    if (!offsets9_host) return fail(WN_ERR_INVALID, "offsets9_host is NULL");
    return WN_OK;
}

#if defined(__HIPCC__)
// The `depth` octaves of brick (bx, by, bz) for the row of lane = ly + 8 lz, or for its NQ samples from x sample q0 (q0 is
// wave-uniform; the octaves are tabulated again for each part of a row): s[j][q] is running sum j of x sample q0 + q, zeroed
// here; amp_sum is fractal_noise's max_value (the sum of the octaves' amplitudes), which the finish divides by.  `off`: the
// nine offsets of the curl fields, each in 0..255 (not read by kValue and kGrad).  perm: the table in LDS; ax: the wave's own
// slice.  Every branch on the x cells is a scalar branch.
template <int FIELD, int KIND, int NQ = kBrickEdge>
__device__ __forceinline__ void perlin_brick_walk(const uint8_t *const perm, BrickAxisSlice &ax, const GridArgs &g, const float den,
                                                  const int *const off, const int depth, const int lane, const int ly, const int lz,
                                                  const int bx, const int by, const int bz,
                                                  double (&s)[field_sums(FIELD)][NQ], double &amp_sum, const int q0 = 0)
{
    constexpr int NS = field_sums(FIELD), NP = field_potentials(FIELD);
    constexpr bool kIsCurl = FIELD == kCurl || FIELD == kCurlPsi;
    // lanes 0..23: the walker of axis index lane & 7 of axis lane >> 3 (z indices are absolute: g.z0 == 0)
    const int first = (lane < kBrickEdge) ? bx : ((lane < 2 * kBrickEdge) ? by : bz);
    RunOctaveWalker<KIND> walker{grid_coord(g, den, kBrickEdge * first + ly)};

#pragma unroll
    for (int j = 0; j < NS; ++j)
#pragma unroll
        for (int q = 0; q < NQ; ++q) s[j][q] = 0.0;
    double weight = 1.0; // turb weight / fractal amplitude
    amp_sum = 0.0;

#pragma nounroll
    for (int oc = 0; oc < depth; ++oc) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); // the previous octave's (brick's) reads are done
        if (lane < kBrickAxisEntries)
            walker.step([&](int cell, double f) {
                ax.e[lane] = RunAxisEntryD::of(f);
                ax.cell[lane] = (uint8_t)cell;
            });
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");

        const RunAxisEntryD ye = ax.e[kBrickEdge + ly], ze = ax.e[2 * kBrickEdge + lz];
        const int Y = ax.cell[kBrickEdge + ly], Z = ax.cell[2 * kBrickEdge + lz];
        const double v = ye.fade, w = ze.fade, dv = ye.dfade, dw = ze.dfade;
        // the 8 x cells: the same for every lane, held on the scalar side
        const uint32_t *const xc = reinterpret_cast<const uint32_t *>(ax.cell);
        const uint64_t cells = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)xc[1]) << 32) |
                               (uint32_t)__builtin_amdgcn_readfirstlane((int)xc[0]);
        auto cell_at = [&](int q) { return (int)((cells >> (8 * q)) & 255u); };

        // Segments of the rows that stay inside one cell: todo, X and `mine` are wave-uniform.  At a step of <= 1/8
        // cell per sample a brick row is one segment and the loop takes one trip (the BASELINE lattice, and every
        // octave of turb(7) on the 1/128 lattice but the last two).
        uint32_t todo = ((1u << NQ) - 1u) << q0; // samples not yet computed
        do {
            const int X = cell_at(__ffs((int)todo) - 1);
            uint32_t mine = 0;
#pragma unroll
            for (int q = 0; q < NQ; ++q) mine |= (((todo >> (q0 + q)) & 1u) && cell_at(q0 + q) == X) ? (1u << (q0 + q)) : 0u;

            auto potential = [&](auto kc) __attribute__((always_inline)) {
                constexpr int k = decltype(kc)::value;
                // the corner state of the cell (of potential k)
                int h[8];
                double K[8], P0[3] = {0.0, 0.0, 0.0}, P1[3] = {0.0, 0.0, 0.0};
                uint32_t mm[8], tt[8];
                if (kIsCurl)
                    run_hash_corners(perm, (X + off[3 * k]) & 255, (Y + off[3 * k + 1]) & 255, (Z + off[3 * k + 2]) & 255, h);
                else run_hash_corners(perm, X, Y, Z, h);
                run_corner_entries(h, ye.f, ze.f, K, mm, tt);
                if (FIELD != kValue) {
                    __builtin_amdgcn_sched_barrier(0); // the corner blend's decoded components after the entries
                    perlin_corner_blend(h, v, w, P0, P1);
                }
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    if ((mine >> (q0 + q)) & 1u) {
                        const RunAxisEntryD xe = ax.e[q0 + q]; // one address for the wave: a broadcast read
                        double gr[8], gn[3];
                        run_corner_gradients(K, mm, tt, xe.f, gr);
                        // the value's lerps and the partials; what a field does not read falls away at compile time
                        const double nv = perlin_sample_grad(gr, xe.fade, v, w, xe.dfade, dv, dw, P0, P1, gn);
                        if (kIsCurl) {
                            const double one = gn[k == 0 ? 1 : 0], two = gn[k == 2 ? 1 : 2];
                            double &sa = s[(2 * k) % NS][q], &sb = s[(2 * k + 1) % NS][q];
                            sa = (KIND == kNoise) ? one : sa + one;
                            sb = (KIND == kNoise) ? two : sb + two;
                            if (FIELD == kCurlPsi) {
                                double &sp = s[(6 + k) % NS][q];
                                sp = (KIND == kNoise) ? nv : sp + weight * nv;
                            }
                        } else {
                            double &sv = s[0][q];
                            sv = (KIND == kNoise) ? nv : ((KIND == kTurb) ? sv + weight * nv : sv + nv * weight);
                            if (FIELD == kGrad) {
#pragma unroll
                                for (int c = 0; c < 3; ++c) {
                                    double &sg = s[(1 + c) % NS][q];
                                    sg = (KIND == kNoise) ? gn[c] : sg + gn[c];
                                }
                            }
                        }
                    }
                    if (FIELD != kValue || (q & 1)) __builtin_amdgcn_sched_barrier(0); // one sample (value: two) at a time
                }
            };
            potential(std::integral_constant<int, 0>{});
            if (NP == 3) {
                potential(std::integral_constant<int, 1>{});
                potential(std::integral_constant<int, 2>{});
            }
            todo &= ~mine;
        } while (todo != 0u);
        amp_sum += weight;
        weight *= 0.5;
    }
}

// Four consecutive samples of a lane's row in CH channels: one float4 per channel, or scalars.
template <int CH>
__device__ __forceinline__ void perlin_brick_store4(float *const dst, const size_t chan, const int vec4_ok, const float (&fin)[CH][4])
{
#pragma unroll
    for (int ch = 0; ch < CH; ++ch) {
        float *const d = dst + ch * chan;
        if (vec4_ok) *reinterpret_cast<v4f *>(d) = v4f{fin[ch][0], fin[ch][1], fin[ch][2], fin[ch][3]};
        else {
#pragma unroll
            for (int q = 0; q < 4; ++q) d[q] = fin[ch][q];
        }
    }
}

// A lane's row of CH channels as two float4 of its slot per channel (each channel leaves as one contiguous 2-KiB wave
// store), or as scalars where the output is not 16-byte aligned.  dst: the row's first sample in channel 0; chan: floats
// between channels.
template <int CH>
__device__ __forceinline__ void perlin_brick_store(float *const dst, const size_t chan, const int vec4_ok, const float (&fin)[CH][kBrickEdge])
{
#pragma unroll
    for (int ch = 0; ch < CH; ++ch) {
        float *const d = dst + ch * chan;
        if (vec4_ok) {
            *reinterpret_cast<v4f *>(d) = v4f{fin[ch][0], fin[ch][1], fin[ch][2], fin[ch][3]};
            *reinterpret_cast<v4f *>(d + 4) = v4f{fin[ch][4], fin[ch][5], fin[ch][6], fin[ch][7]};
        } else {
#pragma unroll
            for (int q = 0; q < kBrickEdge; ++q) d[q] = fin[ch][q];
        }
    }
}
#endif

} // namespace wn
