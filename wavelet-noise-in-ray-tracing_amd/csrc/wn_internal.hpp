// wn_internal.hpp -- shared between the C-ABI translation units of libwnoise_hip.so.
// gfx950 only; compiled with -ffp-contract=off (fused multiply-adds appear only where a kernel
// asks for them with __builtin_fmaf).
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "wn_advect.hpp" // a particle's trace and its chain of launches, shared with host/scalar_eval.cpp
#include "wn_eval.hpp"   // dmod, pow2_mask, bspline and the exact evaluators, shared with host/scalar_eval.cpp
#include "wnoise.h"
#include "wnoise_advect.h"

typedef float v4f __attribute__((ext_vector_type(4)));

struct wn_tile {
    int n = 0;          // even tile size (0 = empty tile)
    int dims = 0;       // 2 or 3
    size_t count = 0;   // n^dims
    float *dev = nullptr;
    // 3-D tiles also keep a copy whose rows carry two wrap-around columns (row stride n+2,
    // padded[x] = tile[x mod n] for x in [0, n+2)): the three x taps of a scattered point are then
    // always adjacent and come with ONE 12-byte load (9 gathers per point instead of 27)
    float *dev_padded = nullptr;
    int device = 0;
};

struct wn_perm {
    int host[512];
    uint8_t *dev = nullptr; // 512 bytes: values 0..255 (perlin.h:35-38)
    int device = 0;
};

struct wn_timer {
    hipEvent_t start = nullptr, stop = nullptr;
};

namespace wn {

void set_error(const char *fmt, ...);
int fail(int code, const char *fmt, ...);
int hip_fail(hipError_t e, const char *what);
int require_device();

inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

// The HIP runtime draws from the C library's global rand() state while it launches kernels
// (measured on ROCm 7.2: 100 launches shift the caller's rand() sequence).  The reference's
// renderer is deterministic only through the unseeded global rand() (main.cpp:184-185,
// rtweekend.h:37-40), so every ABI entry point parks the caller's random state and lets HIP
// consume a private one; the caller's stream is exactly what it would be without the library.
// Depth-counted under a mutex: the state is parked by the first ABI call that enters the library
// (from any thread) and restored by the last one that leaves.
class RandStateGuard {
  public:
    RandStateGuard();
    ~RandStateGuard();
    RandStateGuard(const RandStateGuard &) = delete;
    RandStateGuard &operator=(const RandStateGuard &) = delete;
};
#define WN_ENTRY() ::wn::RandStateGuard wn_rand_state_guard_

#define WN_HIP(call)                                            \
    do {                                                        \
        hipError_t _e = (call);                                 \
        if (_e != hipSuccess) return ::wn::hip_fail(_e, #call); \
    } while (0)

#define WN_LAUNCH_CHECK(name)                                    \
    do {                                                         \
        hipError_t _e = hipGetLastError();                       \
        if (_e != hipSuccess) return ::wn::hip_fail(_e, name);   \
    } while (0)

// Grid coordinate arguments shared by all dense-grid kernels (mirror of wn_grid plus the
// derived slab extent).
struct GridArgs {
    int den, nx, ny, z0, nz; // nz = planes in this call
    float base_range, octave_scale, post_scale;
    int z_const_mode;
    float z_const;
    float out_scale;
};

int check_grid(const wn_grid *g, bool needs_z, GridArgs *out);

// 1/den when den is a power of two (then i * (1/den) == i / den exactly), else 0: see lattice_coord_fast.
inline float inv_den_of(int den) { return ((den & (den - 1)) == 0) ? 1.0f / (float)den : 0.0f; }

// Per-device facts, kept in mutex-protected tables keyed by the device ordinal (a host may drive
// several devices from several threads).
int current_device();
int device_compute_units(int dev);
// Opt `kernel` in to `bytes` of dynamic LDS on device `dev` (needed beyond 64 KiB), once per
// (kernel, device).  false = the runtime refused: the caller falls back to another kernel.
bool ensure_dynamic_lds(const void *kernel, int dev, size_t bytes);
// WN_ERR_INVALID unless the handle (tile / perm) lives on the current device.
int check_handle_device(int handle_device, const char *what);
// The first checks of a batched entry point (`entry` names it in the message): a HIP device, then a handle that lives on
// the current device; a tile that is not empty must also have `dims` dimensions.
int check_tile(const wn_tile *tile, int dims, const char *entry);
int check_perm(const wn_perm *perm, const char *entry);

// Rows of nx floats from `out` all start 16-byte aligned: float4 stores.
inline bool vec4_ok(const float *out, int nx) { return nx % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0; }

// 256-lane workgroups for a grid-stride loop over `total` items: at least one, at most `cap`.
constexpr size_t kStrideBlockCap = 256u * 8u * 8u;
inline int stride_blocks(size_t total, size_t cap = kStrideBlockCap)
{
    const size_t b = (total + 255) / 256;
    return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

// One band's lattice step (cells per sample) and the bounds that the dense-grid planners derive from it.
struct LatticeStep {
    double step;  // base_range * oscale * post_scale / den
    double pmax;  // bound on a coordinate, + 1
    double slack; // fp32 rounding of a coordinate (4 ulp of pmax), + the planner's margin
    // cells whose basis functions reach `samples` consecutive samples
    long long extent(int samples) const { return (long long)floor((samples - 1) * step + slack) + 1 + 3; }
    // 4 consecutive samples span <= 2 mids
    bool two_mids() const { return 3.0 * step + slack <= 1.0; }
};

// false when the step of the band at `oscale` is not finite or negative (signed_step: its magnitude is used), or when a
// coordinate could pass 1e6 cells (mids stay far inside the int / float-exact range).  pmax covers indices up to
// max(nx, ny, |z0| + nz), and |z_const| on top when with_z_const; margin_cells is added to slack.
inline bool lattice_step(const GridArgs &g, float oscale, bool with_z_const, bool signed_step, double margin_cells,
                         LatticeStep *ls)
{
    double step = (double)g.base_range * (double)oscale * (double)g.post_scale / g.den;
    if (signed_step) step = fabs(step);
    if (!(step >= 0.0) || !std::isfinite(step)) return false;
    const double imax = fmax(fmax((double)g.nx, (double)g.ny), fabs((double)g.z0) + g.nz);
    const double pmax = step * imax + (with_z_const ? fabs((double)g.z_const) : 0.0) + 1.0;
    if (pmax > 1.0e6) return false;
    *ls = LatticeStep{step, pmax, pmax * 4.8e-7 + margin_cells};
    return true;
}

// WMultibandNoise (Cook & DeRose, Appendix 2): bands run while s + first_band + b < 0, band b at 2^(first_band+b) with
// weight w_host[b]; the variance sums ALL nbands.  The argument structs of the multiband kernels carry Bands as a base
// (wn::multiband_exact reads it).  multiband_bands checks nbands / w_host, then fills nbands (the active bands),
// band_scale, band_w, apply_div and out_div.
constexpr int kMaxBands = 8;
struct Bands {
    int nbands;
    float band_scale[kMaxBands], band_w[kMaxBands]; // 2^(first_band+b) and w_host[b] of the active bands
    float out_div;
    int apply_div;

    // A multiband call in which no band contributes runs the exact kernels on one band of weight 0: the result,
    // 0 (/ out_div) * out_scale in every channel, is evaluated on the device.
    void zero_band_if_none()
    {
        if (nbands != 0) return;
        nbands = 1;
        band_scale[0] = 1.0f;
        band_w[0] = 0.0f;
    }
};
inline int multiband_bands(float s, int first_band, int nbands, const float *w_host, float var_per_band, Bands *a)
{
    if (nbands < 0 || nbands > kMaxBands)
        return fail(WN_ERR_INVALID, "nbands must be in 0..%d (got %d)", kMaxBands, nbands);
    if (nbands && !w_host) return fail(WN_ERR_INVALID, "w_host is NULL");
    int active = 0;
    while (active < nbands && s + (float)first_band + (float)active < 0.0f) ++active;
    float variance = 0.0f;
    for (int b = 0; b < nbands; ++b) variance += w_host[b] * w_host[b];
    a->nbands = active;
    for (int b = 0; b < active; ++b) {
        a->band_scale[b] = ldexpf(1.0f, first_band + b);
        a->band_w[b] = w_host[b];
    }
    a->apply_div = variance != 0.0f;
    a->out_div = a->apply_div ? sqrtf(variance * var_per_band) : 1.0f;
    return WN_OK;
}

// What wn::eval3d_curl_exact / multiband_curl_exact read (wn_wavelet_curl.hip, wn_wavelet_advect.hip).
struct CurlEval : Bands {
    const float *coef;
    int n, nmask;
    int off[9]; // (x, y, z) of psi0, psi1, psi2, each in [0, n)
    int mb;     // 0: evaluate3D potentials; 1: WMultibandNoise potentials (nbands may be 0: no band is active)
};

// The first checks of a curl entry point, then the tile's fields of CurlEval (its padded copy when it has one) and the
// offsets reduced with the reference's Mod.
inline int curl_eval_args(const wn_tile *tile, const int32_t *offsets9_host, const char *entry, CurlEval *e)
{
    const int rc = check_tile(tile, 3, entry);
    if (rc) return rc;
    if (!offsets9_host) return fail(WN_ERR_INVALID, "%s: offsets9_host is NULL", entry);
    *e = CurlEval{};
    e->coef = tile->dev_padded ? tile->dev_padded : tile->dev;
    e->n = tile->n;
    e->nmask = pow2_mask(tile->n);
    for (int i = 0; i < 9; ++i) e->off[i] = tile->n > 0 ? dmod(offsets9_host[i], tile->n, e->nmask) : 0;
    return WN_OK;
}

// f(PADDED, MB) as std::bool_constant for the four forms of a kernel that evaluates a CurlEval: the tile's padded copy or
// its linear one, WMultibandNoise potentials or evaluate3D's.
template <typename F>
inline void with_curl_form(const wn_tile *tile, const CurlEval &e, const F &f)
{
    if (e.mb) {
        if (tile->dev_padded) f(std::true_type{}, std::true_type{});
        else f(std::false_type{}, std::true_type{});
    } else {
        if (tile->dev_padded) f(std::true_type{}, std::false_type{});
        else f(std::false_type{}, std::false_type{});
    }
}

// The checks of an advection call's wn_advect or wn_advect2d: the same fields, a drift of three or two components.
template <typename A>
inline int check_advect(const A *a)
{
    if (!a) return fail(WN_ERR_INVALID, "wn_advect is NULL");
    if (a->method < WN_ADVECT_EULER || a->method > WN_ADVECT_RK4)
        return fail(WN_ERR_INVALID, "wn_advect.method must be 0 (Euler), 1 (midpoint) or 2 (RK4) (got %d)", a->method);
    if (a->steps < 0) return fail(WN_ERR_INVALID, "wn_advect.steps must be >= 0 (got %d)", a->steps);
    if (a->traj_every < 0) return fail(WN_ERR_INVALID, "wn_advect.traj_every must be >= 0 (got %d)", a->traj_every);
    bool finite = std::isfinite(a->h) && std::isfinite(a->gain);
    for (const float d : a->drift) finite = finite && std::isfinite(d);
    if (!finite) return fail(WN_ERR_INVALID, "wn_advect.h, gain and drift must be finite");
    return WN_OK;
}

// The checks of an advection call's three buffers of n particles of D components of T, after check_advect; in_name and
// out_name are the entry point's parameter names.  out may be in itself, and may not overlap it otherwise.
template <typename T, int D>
inline int check_advect_buffers(const T *in_dev, const T *out_dev, const T *traj_dev, size_t n, int traj_every,
                                const char *in_name, const char *out_name)
{
    if (!in_dev || !out_dev) return fail(WN_ERR_INVALID, "%s / %s is NULL", in_name, out_name);
    if (traj_every && !traj_dev) return fail(WN_ERR_INVALID, "traj_dev is NULL with traj_every = %d", traj_every);
    const uintptr_t in_b = reinterpret_cast<uintptr_t>(in_dev), out_b = reinterpret_cast<uintptr_t>(out_dev);
    const size_t bytes = D * n * sizeof(T);
    if (in_b != out_b && in_b < out_b + bytes && out_b < in_b + bytes)
        return fail(WN_ERR_INVALID, "%s overlaps %s without being equal to it", out_name, in_name);
    return WN_OK;
}

// The *_try functions below launch their kernel when the lattice is in its regime and return WN_OK (or the launch's
// error); outside it they launch nothing and return kDeclined, and the caller offers the lattice to the next kernel.
constexpr int kDeclined = -1;

// wn_wavelet_strip.hip: the strip-march kernel.
int strip_try(const wn_tile *tile, const GridArgs &g, float *out_dev, hipStream_t stream);

// wn_wavelet_multiband.hip: the plane-pipeline kernel, for lattices of 1..5 bands (g carries the bands' common
// post_scale; oscale / weights per band; out_div = sqrt(sum w^2 * variance)) with at least min_bricks_per_cu bricks of
// 512 x 8 x 8 samples per compute unit.
int multiband_try(const wn_tile *tile, const GridArgs &g, int nbands, const float *oscale, const float *weights,
                  float out_div, float *out_dev, hipStream_t stream, int min_bricks_per_cu);

// wn_wavelet_exact.hip: bit-exact dense 3-D grids with the coefficient box staged in LDS.
int exact_lds_try(const wn_tile *tile, const GridArgs &g, float *out_dev, hipStream_t stream);

// wn_tilegen.hip: the filter half of generateNoiseTile2D/3D on the device.
int tilegen_filter(wn_tile *t, const float *field_dev, hipStream_t stream);
// wn_tilegen.hip: (re)build t->dev_padded from t->dev (no-op for 2-D tiles).
int tile_build_padded(wn_tile *t, hipStream_t stream);

} // namespace wn

// ---------------------------------------------------------------------------------------------
// device helpers
// ---------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
namespace wn {

// Lattice coordinate of index i (experient/main.cpp:20-26): ((float(i)/den)*range)*octave*post,
// one float rounding per operation, division IEEE-correct (hipcc default
// -fhip-fp32-correctly-rounded-divide-sqrt).
__device__ __forceinline__ float lattice_coord(int i, float den, float range, float oscale,
                                               float post)
{
    float c = ((float)i / den) * range;
    c = c * oscale;
    c = c * post;
    return c;
}

// The lattice of the sample-per-lane grid kernels (den = (float)g.den): the coordinate of index i along x or y, of plane z
// of the call (g.z0 + z, or z_const in z_const_mode), and of sample e of nx * ny * nz (2-D: nx * ny) samples, x fastest.
__device__ __forceinline__ float grid_coord(const GridArgs &g, float den, int i)
{
    return lattice_coord(i, den, g.base_range, g.octave_scale, g.post_scale);
}

__device__ __forceinline__ float grid_zcoord(const GridArgs &g, float den, int z)
{
    return g.z_const_mode ? g.z_const : grid_coord(g, den, g.z0 + z);
}

__device__ __forceinline__ void lattice_index(const GridArgs &g, size_t e, int &x, int &y, int &z)
{
    x = (int)(e % g.nx);
    const size_t r = e / g.nx;
    y = (int)(r % g.ny);
    z = (int)(r / g.ny);
}

__device__ __forceinline__ void lattice_point(const GridArgs &g, float den, int x, int y, int z, float p[3])
{
    p[0] = grid_coord(g, den, x);
    p[1] = grid_coord(g, den, y);
    p[2] = grid_zcoord(g, den, z);
}

__device__ __forceinline__ void lattice_point(const GridArgs &g, float den, size_t e, float p[3])
{
    int x, y, z;
    lattice_index(g, e, x, y, z);
    lattice_point(g, den, x, y, z, p);
}

__device__ __forceinline__ void lattice_point2d(const GridArgs &g, float den, size_t e, float &px, float &py)
{
    px = grid_coord(g, den, (int)(e % g.nx));
    py = grid_coord(g, den, (int)(e / g.nx));
}

// lattice_coord with the division replaced by an exact multiply when den is a power of two (inv_den = inv_den_of(den)).
__device__ __forceinline__ float lattice_coord_fast(int i, float den, float inv_den, float range, float oscale,
                                                    float post)
{
    const float fi = (float)i;
    float c = ((inv_den != 0.0f) ? fi * inv_den : fi / den) * range;
    c = c * oscale;
    c = c * post;
    return c;
}

// Workgroup barrier that waits for the wave's LDS accesses only: no vmcnt drain of its outstanding global loads and stores.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

} // namespace wn
#endif
