// wn_tile2d_lds.hpp -- a whole 2-D tile staged in LDS, for the kernels that read every tap of every band there
// (wn_wavelet_multiband2d.hip, wn_wavelet_curl2d.hip).
#pragma once

#if defined(__HIPCC__)
namespace wn {

// The whole tile from global memory to LDS in the padded layout (row stride n+2 with two wrap-around columns: the layout
// wn::eval2d_exact<., PADDED> reads), one row per wave and step; then the workgroup's barrier.  WORKGROUP: the lanes of the
// workgroup, whole waves.
template <int WORKGROUP>
__device__ __forceinline__ void stage_tile(float *lds, const float *coef, int n)
{
    const int stride = n + 2, lane = threadIdx.x & 63;
    for (int y = threadIdx.x >> 6; y < n; y += WORKGROUP / 64)
        for (int x = lane; x < stride; x += 64) lds[y * stride + x] = coef[y * n + (x >= n ? x - n : x)];
    __syncthreads();
}

} // namespace wn
#endif
