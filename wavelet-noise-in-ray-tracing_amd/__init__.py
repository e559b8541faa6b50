"""wavelet-noise-in-ray-tracing_amd: MI355X-native evaluation of the wavelet / Perlin noise hot
path of Jason9339/Wavelet-Noise-in-ray-tracing.

Layout
  csrc/   hand-written HIP kernels + the C ABI of include/wnoise.h  -> libwnoise_hip.so
  host/   C++ host classes with the reference's names (WaveletNoise, perlin, PerlinNoise,
          noise_texture, wavelet_texture) forwarding to the C ABI
  tools/  grid generator (experient/main.cpp's role) over the batched ABI
  noise.py  Python mirror of the same interface (tests / bench harness; torch supplies device
          memory, streams and torch.distributed, nothing else)

The directory name is not a Python identifier: import it with
    importlib.import_module("wavelet-noise-in-ray-tracing_amd")
"""
from . import _capi
from ._capi import WnError, wn_grid, WN_GRID_DEFAULT, WN_GRID_EXACT, WN_Z_CONST, WN_Z_LATTICE
from ._capi import WN_PERLIN_CURL_NOISE, WN_PERLIN_CURL_TURB, WN_PERLIN_CURL_FRACTAL

_capi.load()  # fail loudly when the HIP library is missing

from .noise import (  # noqa: E402
    WaveletNoise, perlin, PerlinNoise, noise_texture, wavelet_texture, wavelet_multiband_texture,
    noise_multiband_texture, GridSpec,
    generate2DOctaveBandNoise, generate2DMultibandNoise, generate2DMultibandNoiseGradient, generate2DMultibandNoiseCurl,
    generate2DMultibandNoiseCurlBounded,
    generate3DSlicedOctaveBandNoise,
    generate3DProjectedOctaveBandNoise, generatePerlinNoise2D, generatePerlinNoise3DSliced,
    wavelet_volume, wavelet_volume_launcher, multiband_volume, perlin_volume, turb_volume, device_info, HipTimer,
    wavelet_gradient_volume, multiband_gradient_volume, wavelet2d_gradient_image, projected_gradient_volume,
    perlin_gradient_volume, turb_gradient_volume, curl_volume, multiband_curl_volume, perlin_curl_volume,
    wavelet_bricks, multiband_bricks,
    wavelet_gradient_bricks, multiband_gradient_bricks, curl_bricks, multiband_curl_bricks,
    curl_bounded_bricks, multiband_curl_bounded_bricks,
    perlin_bricks, turb_bricks, fractal_bricks, perlin_gradient_bricks, turb_gradient_bricks, fractal_gradient_bricks,
    perlin_curl_bricks, perlin_curl_bounded_bricks,
)
from .shard import slab_bounds, gather_volume, NativeComm  # noqa: E402
from . import formats  # noqa: E402

__all__ = [
    "WnError", "wn_grid", "WN_GRID_DEFAULT", "WN_GRID_EXACT", "WN_Z_CONST", "WN_Z_LATTICE",
    "WN_PERLIN_CURL_NOISE", "WN_PERLIN_CURL_TURB", "WN_PERLIN_CURL_FRACTAL",
    "WaveletNoise", "perlin", "PerlinNoise", "noise_texture", "wavelet_texture", "wavelet_multiband_texture",
    "noise_multiband_texture", "GridSpec",
    "generate2DOctaveBandNoise", "generate2DMultibandNoise", "generate2DMultibandNoiseGradient",
    "generate2DMultibandNoiseCurl",
    "generate2DMultibandNoiseCurlBounded",
    "generate3DSlicedOctaveBandNoise",
    "generate3DProjectedOctaveBandNoise", "generatePerlinNoise2D", "generatePerlinNoise3DSliced",
    "wavelet_volume", "wavelet_volume_launcher", "multiband_volume", "perlin_volume", "turb_volume", "device_info",
    "HipTimer", "wavelet_gradient_volume", "multiband_gradient_volume", "wavelet2d_gradient_image",
    "projected_gradient_volume", "perlin_gradient_volume", "turb_gradient_volume", "curl_volume",
    "multiband_curl_volume", "perlin_curl_volume", "wavelet_bricks", "multiband_bricks",
    "wavelet_gradient_bricks", "multiband_gradient_bricks", "curl_bricks", "multiband_curl_bricks",
    "curl_bounded_bricks", "multiband_curl_bounded_bricks", "perlin_bricks", "turb_bricks", "fractal_bricks",
    "perlin_gradient_bricks", "turb_gradient_bricks", "fractal_gradient_bricks", "perlin_curl_bricks", "perlin_curl_bounded_bricks",
    "slab_bounds",
    "gather_volume", "NativeComm", "formats",
]
