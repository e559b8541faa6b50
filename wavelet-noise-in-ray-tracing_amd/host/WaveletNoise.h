// WaveletNoise.h -- the reference's class WaveletNoise (WaveletNoise.h:20-59) over the MI355X
// C ABI.  Same constructor, member names and signatures, so callers written against the
// reference (texture.h, experient/main.cpp) compile unchanged; the work is done by HIP kernels.
//
//   generateNoiseTile2D/3D : Gaussian field drawn from the member mt19937 / normal_distribution
//                            exactly as the reference draws it (libstdc++ stream), filter passes
//                            on the GPU (wn_tile_generate_from_field); coefficients stay
//                            resident in HBM and are mirrored for getNoiseCoefficients().
//   evaluate2D/3D/3DProjected(p) : one sample, on the host from the mirrored coefficients (scalar_eval.h,
//                            bit-identical to the reference and to the kernels; WN_SCALAR_ON_DEVICE=1: one
//                            request to the resident scalar kernel, ~2.6 us); the batched overloads below
//                            are the GPU path.
#ifndef WAVELET_NOISE_H
#define WAVELET_NOISE_H

#include <cstddef>
#include <iostream>
#include <limits>
#include <random>
#include <string>
#include <vector>

struct wn_tile;   // include/wnoise.h
struct wn_advect; // include/wnoise_advect.h
struct wn_advect2d; // include/wnoise_curl2d.h
struct wn_obstacle; // include/wnoise_bounded.h
struct wn_obstacle2d; // include/wnoise_bounded2d.h

// Statistical analysis structure (WaveletNoise.h:11-18)
struct DataStats {
    float avg = 0.0f;
    float var = 0.0f;
    float min_val = std::numeric_limits<float>::max();
    float max_val = std::numeric_limits<float>::lowest();
    long long count_nan_inf = 0;
    float energy = 0.0f; // Sum of squares
};

class WaveletNoise {
  public:
    WaveletNoise(int tileSize, unsigned int seed = 0); // WaveletNoise.cpp:20-26
    ~WaveletNoise();
    WaveletNoise(const WaveletNoise &) = delete;
    WaveletNoise &operator=(const WaveletNoise &) = delete;

    void generateNoiseTile2D(); // WaveletNoise.cpp:69-108
    void generateNoiseTile3D(); // WaveletNoise.cpp:142-183

    float evaluate2D(const float p[2]) const;                                  // :111-140
    float evaluate3D(const float p[3]) const;                                  // :185-215
    float evaluate3DProjected(const float p[3], const float normal[3]) const;  // :218-265

    DataStats calculateStats(const std::vector<float> &data, const std::string &name) const; // :268-288
    const std::vector<float> &getNoiseCoefficients() const;
    int getTileSize() const;

    // ---- additive: batched forms of the same members (host pointers; n points) ----------------
    void evaluate2D(const float *xy, size_t n, float *out) const;
    void evaluate3D(const float *xyz, size_t n, float *out) const;
    void evaluate3DProjected(const float *xyz, const float *normals, size_t n, float *out) const;
    // Cook & DeRose Appendix 2 WMultibandNoise (normal == NULL branch); absent from the reference.
    float WMultibandNoise(const float p[3], float s, int firstBand, int nbands, const float *w,
                          float variance = 0.18402f) const;
    void WMultibandNoise(const float *xyz, size_t n, float s, int firstBand, int nbands,
                         const float *w, float variance, float *out) const;
    // The paper's full signature: normal != nullptr makes every band WProjectedNoise (evaluate3DProjected) and
    // normalises with 0.296; normal == nullptr is the overload above with the paper's 0.210 replaced by `variance`.
    float WMultibandNoise(const float p[3], float s, const float *normal, int firstBand, int nbands,
                          const float *w, float variance = 0.296f) const;
    // Analytic gradients (absent from the reference).  evaluate3DGradient returns evaluate3D(p) (the same bits) and writes
    // its gradient to grad: on the host (scalar_eval.h), bit-identical to wn_eval3d_grad_points.  The batched forms write n
    // records {value, d/dx, d/dy, d/dz} to out4.  WMultibandNoiseGradient: WMultibandNoise (normal == NULL) and its gradient
    // with respect to p, one point as a batch of one on the device.
    float evaluate3DGradient(const float p[3], float grad[3]) const;
    void evaluate3DGradient(const float *xyz, size_t n, float *out4) const;
    float WMultibandNoiseGradient(const float p[3], float s, int firstBand, int nbands, const float *w, float grad[3],
                                  float variance = 0.18402f) const;
    void WMultibandNoiseGradient(const float *xyz, size_t n, float s, int firstBand, int nbands, const float *w,
                                 float variance, float *out4) const;
    // evaluate2DGradient returns evaluate2D(p) and writes d/dx, d/dy to grad, on the host (bit-identical to
    // wn_eval2d_grad_points); the batched form writes n records {value, d/dx, d/dy} to out3.  evaluate3DProjectedGradient:
    // evaluate3DProjected(p, normal) and its gradient with respect to p, the normal held fixed (the gradient of the sum
    // without the value's 1e-6 cut, include/wnoise.h), on the host (bit-identical to wn_eval3d_projected_grad_points); the
    // batched form takes one normal per point and writes n records {value, d/dx, d/dy, d/dz} to out4.
    float evaluate2DGradient(const float p[2], float grad[2]) const;
    void evaluate2DGradient(const float *xy, size_t n, float *out3) const;
    float evaluate3DProjectedGradient(const float p[3], const float normal[3], float grad[3]) const;
    void evaluate3DProjectedGradient(const float *xyz, const float *normals, size_t n, float *out4) const;
    // WMultibandNoise(p, s, normal, ...) and its gradient with respect to p: normal != nullptr makes every band
    // evaluate3DProjected (wn_multiband3d_projected_grad_points, a batch of one on the device); normal == nullptr is the
    // overload above with `variance` passed on.  The batched form takes one normal per point, or one for all points when
    // oneNormal; normals == nullptr is the batched overload above.
    float WMultibandNoiseGradient(const float p[3], float s, const float *normal, int firstBand, int nbands, const float *w,
                                  float grad[3], float variance = 0.296f) const;
    void WMultibandNoiseGradient(const float *xyz, const float *normals, bool oneNormal, size_t n, float s, int firstBand,
                                 int nbands, const float *w, float variance, float *out4) const;
    // WMultibandNoise with the band limit taken from a footprint PER SAMPLE (include/wnoise_footprint.h; absent from the
    // reference): band b of a sample runs while (s + firstBand) + b < 0, s = log2 of that sample's footprint, with the
    // weight w[b] (fade == false: the paper's hard cut) or w[b] * min(1, -((s + firstBand) + b)) (fade: the finest
    // surviving band fades in over one octave of footprint).  The batched forms take one s per point and optional normals
    // (nullptr: bands are evaluate3D; else evaluate3DProjected with one normal per point, or one for all when oneNormal)
    // and run on the device (wn_multiband3d[_projected]_footprint[_grad]_points); out4: records {value, d/dx, d/dy, d/dz}.
    // The scalar members are evaluated on the host (wnhost_multiband3d_footprint), bit-identical to the kernels.
    float WMultibandNoise(const float p[3], float s, bool fade, const float *normal, int firstBand, int nbands,
                          const float *w, float variance) const;
    float WMultibandNoiseGradient(const float p[3], float s, bool fade, const float *normal, int firstBand, int nbands,
                                  const float *w, float grad[3], float variance) const;
    void WMultibandNoise(const float *xyz, const float *normals, bool oneNormal, size_t n, const float *s, bool fade,
                         int firstBand, int nbands, const float *w, float variance, float *out) const;
    void WMultibandNoiseGradient(const float *xyz, const float *normals, bool oneNormal, size_t n, const float *s, bool fade,
                                 int firstBand, int nbands, const float *w, float variance, float *out4) const;
    // WMultibandNoise on the 2-D tile (include/wnoise_multiband2d.h; absent from the reference): bands are evaluate2D at
    // 2 * p * 2^(firstBand+b), band b runs while (s + firstBand) + b < 0, the sum is divided by sqrt(sum w^2 * variance)
    // (0.19686: the reference's 2-D constant).  The gradient is taken with respect to p.  The one-sample members are
    // evaluated on the host (wnhost_multiband2d_footprint), bit-identical to the kernels; the batched forms run on the
    // device: one s for the call (wn_multiband2d_points / _grad_points), or one per point with the hard cut or the fade
    // (wn_multiband2d_footprint_points / _grad_points).  out3: records {value, d/dx, d/dy}.
    float WMultibandNoise2D(const float p[2], float s, int firstBand, int nbands, const float *w, float variance = 0.19686f,
                            bool fade = false) const;
    float WMultibandNoise2DGradient(const float p[2], float s, int firstBand, int nbands, const float *w, float grad[2],
                                    float variance = 0.19686f, bool fade = false) const;
    void WMultibandNoise2D(const float *xy, size_t n, float s, int firstBand, int nbands, const float *w, float variance,
                           float *out) const;
    void WMultibandNoise2DGradient(const float *xy, size_t n, float s, int firstBand, int nbands, const float *w,
                                   float variance, float *out3) const;
    void WMultibandNoise2D(const float *xy, size_t n, const float *s, bool fade, int firstBand, int nbands, const float *w,
                           float variance, float *out) const;
    void WMultibandNoise2DGradient(const float *xy, size_t n, const float *s, bool fade, int firstBand, int nbands,
                                   const float *w, float variance, float *out3) const;
    // Divergence-free curl noise on the 2-D tile and particles moved through it (include/wnoise_curl2d.h; absent from the
    // reference): v = (d psi/dy, -d psi/dx) of the stream function psi = WMultibandNoise2D at ONE footprint s with the hard
    // cut -- the d/dy channel of WMultibandNoise2DGradient, and its d/dx channel with the sign flipped.  The one-sample
    // members are evaluated / traced on the host (wnhost_multiband2d_curl, wnhost_multiband2d_curl_advect), bit-identical to
    // the kernels; the batched forms run on the device (wn_multiband2d_curl_points: n records {vx, vy} to out2;
    // wn_multiband2d_curl_advect_points).  `a` carries method, steps, h, gain, drift and traj_every: the position after
    // a.steps time steps through gain * v + drift goes to p_out / xy_out (which may be the input), and with a.traj_every =
    // e >= 1 the positions after steps 0, e, 2e, ... to traj, a.steps / e + 1 snapshots of n points each ([snapshot][n][2]).
    void WMultibandNoise2DCurl(const float p[2], float s, int firstBand, int nbands, const float *w, float v[2],
                               float variance = 0.19686f) const;
    void WMultibandNoise2DCurl(const float *xy, size_t n, float s, int firstBand, int nbands, const float *w, float variance,
                               float *out2) const;
    void WMultibandNoise2DAdvectCurl(const float p[2], const wn_advect2d &a, float s, int firstBand, int nbands,
                                     const float *w, float p_out[2], float *traj = nullptr, float variance = 0.19686f) const;
    void WMultibandNoise2DAdvectCurl(const float *xy, size_t n, const wn_advect2d &a, float s, int firstBand, int nbands,
                                     const float *w, float variance, float *xy_out, float *traj = nullptr) const;
    // The two members above with solid boundaries and a background stream (absent from the reference;
    // include/wnoise_bounded2d.h, whose wn_obstacle2d the list `obs` of nobs <= WN_MAX_OBSTACLES discs, hollow discs and
    // half-planes holds): the stream function, plus ux * py - uy * px when flow = {ux, uy} is not nullptr, fades to zero
    // towards every obstacle; v is zero inside one and, without a stream, has the unbounded bits far from all of them.  The
    // one-point members run on the host (wnhost_multiband2d_curl_bounded, wnhost_multiband2d_curl_bounded_advect),
    // bit-identical to wn_multiband2d_curl_bounded_points / _advect_points, which the batched forms call.  A list or a stream
    // the C ABI refuses makes every member throw.
    void WMultibandNoise2DCurlBounded(const float p[2], const wn_obstacle2d *obs, int nobs, const float *flow, float s,
                                      int firstBand, int nbands, const float *w, float v[2], float variance = 0.19686f) const;
    void WMultibandNoise2DCurlBounded(const float *xy, size_t n, const wn_obstacle2d *obs, int nobs, const float *flow, float s,
                                      int firstBand, int nbands, const float *w, float variance, float *out2) const;
    void WMultibandNoise2DAdvectCurlBounded(const float p[2], const wn_advect2d &a, const wn_obstacle2d *obs, int nobs,
                                            const float *flow, float s, int firstBand, int nbands, const float *w,
                                            float p_out[2], float *traj = nullptr, float variance = 0.19686f) const;
    void WMultibandNoise2DAdvectCurlBounded(const float *xy, size_t n, const wn_advect2d &a, const wn_obstacle2d *obs, int nobs,
                                            const float *flow, float s, int firstBand, int nbands, const float *w,
                                            float variance, float *xy_out, float *traj = nullptr) const;
    // Divergence-free curl noise (absent from the reference; include/wnoise.h): the curl of the vector potential whose
    // components are evaluate3D (WMultibandNoiseCurl: WMultibandNoise, normal == NULL) of this tile shifted by the whole-cell
    // offsets offsets9 = (x, y, z) of psi0, psi1, psi2; nullptr: defaultCurlOffsets().  evaluate3DCurl(p, ., v) is
    // evaluated on the host (scalar_eval.h), bit-identical to wn_eval3d_curl_points; the scalar WMultibandNoiseCurl is a
    // batch of one on the device.  The batched forms write n records {vx, vy, vz} to out3.
    void evaluate3DCurl(const float p[3], const int *offsets9, float v[3]) const;
    void evaluate3DCurl(const float *xyz, size_t n, const int *offsets9, float *out3) const;
    void WMultibandNoiseCurl(const float p[3], const int *offsets9, float s, int firstBand, int nbands, const float *w,
                             float v[3], float variance = 0.18402f) const;
    void WMultibandNoiseCurl(const float *xyz, size_t n, const int *offsets9, float s, int firstBand, int nbands,
                             const float *w, float variance, float *out3) const;
    // Particles moved through that curl field (absent from the reference; include/wnoise_advect.h, whose wn_advect `a`
    // carries method, steps, h, gain, drift and traj_every): the position after a.steps time steps through
    // gain * curl + drift goes to p_out / xyz_out (which may be the input), and with a.traj_every = e >= 1 the positions after
    // steps 0, e, 2e, ... to traj, a.steps / e + 1 snapshots of n points each ([snapshot][n][3]).  advectCurl(p, ., p_out)
    // is traced on the host (scalar_eval.h), bit-identical to wn_eval3d_curl_advect_points, which the batched form calls;
    // WMultibandNoiseAdvectCurl is batched (wn_multiband3d_curl_advect_points), its scalar form a batch of one.
    void advectCurl(const float p[3], const wn_advect &a, const int *offsets9, float p_out[3], float *traj = nullptr) const;
    void advectCurl(const float *xyz, size_t n, const wn_advect &a, const int *offsets9, float *xyz_out,
                    float *traj = nullptr) const;
    void WMultibandNoiseAdvectCurl(const float p[3], const wn_advect &a, const int *offsets9, float s, int firstBand,
                                   int nbands, const float *w, float p_out[3], float *traj = nullptr,
                                   float variance = 0.18402f) const;
    void WMultibandNoiseAdvectCurl(const float *xyz, size_t n, const wn_advect &a, const int *offsets9, float s,
                                   int firstBand, int nbands, const float *w, float variance, float *xyz_out,
                                   float *traj = nullptr) const;
    // The four members above with solid boundaries (absent from the reference; include/wnoise_bounded.h, whose wn_obstacle
    // the list `obs` of nobs <= WN_MAX_OBSTACLES entries holds): v = A curl Psi + grad A x Psi, zero inside an obstacle and
    // the unbounded bits far from all of them.  The one-point evaluate3DCurlBounded and advectCurlBounded run on the host
    // (scalar_eval.h), bit-identical to wn_eval3d_curl_bounded_points / _advect_points, which the batched forms call; the
    // multiband one-point forms are batches of one.  A list the C ABI refuses makes every member throw.
    void evaluate3DCurlBounded(const float p[3], const int *offsets9, const wn_obstacle *obs, int nobs, float v[3]) const;
    void evaluate3DCurlBounded(const float *xyz, size_t n, const int *offsets9, const wn_obstacle *obs, int nobs,
                               float *out3) const;
    void WMultibandNoiseCurlBounded(const float p[3], const int *offsets9, const wn_obstacle *obs, int nobs, float s,
                                    int firstBand, int nbands, const float *w, float v[3], float variance = 0.18402f) const;
    void WMultibandNoiseCurlBounded(const float *xyz, size_t n, const int *offsets9, const wn_obstacle *obs, int nobs, float s,
                                    int firstBand, int nbands, const float *w, float variance, float *out3) const;
    void advectCurlBounded(const float p[3], const wn_advect &a, const int *offsets9, const wn_obstacle *obs, int nobs,
                           float p_out[3], float *traj = nullptr) const;
    void advectCurlBounded(const float *xyz, size_t n, const wn_advect &a, const int *offsets9, const wn_obstacle *obs,
                           int nobs, float *xyz_out, float *traj = nullptr) const;
    void WMultibandNoiseAdvectCurlBounded(const float p[3], const wn_advect &a, const int *offsets9, const wn_obstacle *obs,
                                          int nobs, float s, int firstBand, int nbands, const float *w, float p_out[3],
                                          float *traj = nullptr, float variance = 0.18402f) const;
    void WMultibandNoiseAdvectCurlBounded(const float *xyz, size_t n, const wn_advect &a, const int *offsets9,
                                          const wn_obstacle *obs, int nobs, float s, int firstBand, int nbands,
                                          const float *w, float variance, float *xyz_out, float *traj = nullptr) const;
    // (0,0,0), (n/3,)*3, (2n/3,)*3 with integer division: a default only, not a measured decorrelation.
    void defaultCurlOffsets(int offsets9[9]) const;
    // The device-resident tile (an empty tile before generate*); for the C-ABI grid entry points.
    const wn_tile *tile(int dims) const;

  private:
    int tileSizeN;
    std::vector<float> noiseCoefficients;
    unsigned int randomSeed;
    std::mt19937 rng;
    std::normal_distribution<float> gaussianDist;
    mutable wn_tile *tile_;
    int tileDims = 0; // dimension of the generated tile (0: none yet)
    void generate(int dims);
};

#endif
