"""ctypes binding of libwnoise_hip.so (include/wnoise.h, include/wnoise_perlin_curl.h, include/wnoise_footprint.h,
include/wnoise_perlin_footprint.h, include/wnoise_multiband2d.h, include/wnoise_advect.h, include/wnoise_bounded.h,
include/wnoise_perlin_advect.h, include/wnoise_curl2d.h, include/wnoise_bounded2d.h, include/wnoise_bricks.h,
include/wnoise_brick_fields.h, include/wnoise_bounded_bricks.h, include/wnoise_perlin_bounded.h,
include/wnoise_perlin_bounded_bricks.h).

The library is the product: if it is missing or fails to load this module raises, it never
substitutes a CPU implementation.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libwnoise_hip.so")

WN_OK, WN_ERR_INVALID, WN_ERR_NO_DEVICE, WN_ERR_HIP, WN_ERR_ALLOC = range(5)
WN_Z_LATTICE, WN_Z_CONST = 0, 1
WN_GRID_DEFAULT, WN_GRID_EXACT = 0, 1


class WnError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"wnoise error {code}: {msg}")
        self.code = code


class wn_grid(C.Structure):
    _fields_ = [("den", C.c_int32), ("nx", C.c_int32), ("ny", C.c_int32), ("z0", C.c_int32),
                ("z1", C.c_int32), ("base_range", C.c_float), ("octave_scale", C.c_float),
                ("post_scale", C.c_float), ("z_mode", C.c_int32), ("z_const", C.c_float),
                ("out_scale", C.c_float), ("flags", C.c_int32)]


# name -> (restype, argtypes); every symbol include/wnoise.h declares.
_vp, _sz, _i, _u32, _f, _d = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.c_float, C.c_double
_pp = C.POINTER(C.c_void_p)
_gp = C.POINTER(wn_grid)
_i32p = C.POINTER(C.c_int32)
SIGNATURES = {
    "wn_last_error": (C.c_char_p, []),
    "wn_version": (C.c_char_p, []),
    "wn_device_count": (_i, [C.POINTER(C.c_int)]),
    "wn_device_set": (_i, [_i]),
    "wn_device_get": (_i, [C.POINTER(C.c_int)]),
    "wn_device_info": (_i, [C.c_char_p, _sz, C.POINTER(C.c_int), C.POINTER(_sz)]),
    "wn_dev_alloc": (_i, [_pp, _sz]),
    "wn_dev_free": (_i, [_vp]),
    "wn_host_alloc_mapped": (_i, [_pp, _pp, _sz]),
    "wn_host_free_mapped": (_i, [_vp]),
    "wn_copy_h2d": (_i, [_vp, _vp, _sz, _vp]),
    "wn_copy_d2h": (_i, [_vp, _vp, _sz, _vp]),
    "wn_stream_sync": (_i, [_vp]),
    "wn_timer_create": (_i, [_pp]),
    "wn_timer_start": (_i, [_vp, _vp]),
    "wn_timer_stop": (_i, [_vp, _vp]),
    "wn_timer_elapsed_ms": (_i, [_vp, C.POINTER(C.c_float)]),
    "wn_timer_destroy": (None, [_vp]),
    "wn_gaussian_fill": (_i, [_u32, _sz, _vp]),
    "wn_perlin_permutation": (_i, [_u32, _vp]),
    "wn_tile_even_size": (_i, [_i]),
    "wn_tile_create": (_i, [_i, _i, _vp, _pp]),
    "wn_tile_generate": (_i, [_i, _i, _u32, _pp]),
    "wn_tile_generate_from_field": (_i, [_i, _i, _vp, _pp]),
    "wn_tile_size": (_i, [_vp]),
    "wn_tile_dims": (_i, [_vp]),
    "wn_tile_count": (_sz, [_vp]),
    "wn_tile_device_ptr": (_vp, [_vp]),
    "wn_tile_download": (_i, [_vp, _vp]),
    "wn_tile_destroy": (None, [_vp]),
    "wn_perm_create": (_i, [_vp, _pp]),
    "wn_perm_create_seeded": (_i, [_u32, _pp]),
    "wn_perm_download": (_i, [_vp, _vp]),
    "wn_perm_destroy": (None, [_vp]),
    "wn_eval3d_grid": (_i, [_vp, _gp, _vp, _vp]),
    "wn_eval2d_grid": (_i, [_vp, _gp, _vp, _vp]),
    "wn_eval3d_projected_grid": (_i, [_vp, _gp, C.POINTER(C.c_float), _vp, _vp]),
    "wn_multiband3d_grid": (_i, [_vp, _gp, _f, _i, _i, C.POINTER(C.c_float), _f, _vp, _vp]),
    "wn_perlin_grid": (_i, [_vp, _gp, _vp, _vp]),
    "wn_perlin_turb_grid": (_i, [_vp, _gp, _i, _vp, _vp]),
    "wn_perlin_fractal_grid": (_i, [_vp, _gp, _vp, _vp]),
    "wn_eval3d_points": (_i, [_vp, _vp, _sz, _vp, _vp]),
    "wn_eval2d_points": (_i, [_vp, _vp, _sz, _vp, _vp]),
    "wn_eval3d_projected_points": (_i, [_vp, _vp, _vp, _sz, _vp, _vp]),
    "wn_multiband3d_points": (_i, [_vp, _vp, _sz, _f, _i, _i, C.POINTER(C.c_float), _f, _vp, _vp]),
    "wn_multiband3d_projected_points": (_i, [_vp, _vp, _vp, _i, _sz, _f, _i, _i, C.POINTER(C.c_float), _f, _vp, _vp]),
    "wn_perlin_points": (_i, [_vp, _vp, _sz, _vp, _vp]),
    "wn_perlin_points_vec3": (_i, [_vp, _vp, _sz, _vp, _vp]),
    "wn_perlin_turb_points": (_i, [_vp, _vp, _sz, _i, _vp, _vp]),
    "wn_perlin_fractal_points": (_i, [_vp, _vp, _sz, _vp, _vp]),
    "wn_eval3d_grad_points": (_i, [_vp, _vp, _sz, _vp, _vp]),
    "wn_multiband3d_grad_points": (_i, [_vp, _vp, _sz, _f, _i, _i, C.POINTER(C.c_float), _f, _vp, _vp]),
    "wn_eval3d_grad_grid": (_i, [_vp, _gp, _vp, _vp]),
    "wn_multiband3d_grad_grid": (_i, [_vp, _gp, _f, _i, _i, C.POINTER(C.c_float), _f, _vp, _vp]),
    "wn_eval2d_grad_points": (_i, [_vp, _vp, _sz, _vp, _vp]),
    "wn_eval2d_grad_grid": (_i, [_vp, _gp, _vp, _vp]),
    "wn_eval3d_projected_grad_points": (_i, [_vp, _vp, _vp, _sz, _vp, _vp]),
    "wn_eval3d_projected_grad_grid": (_i, [_vp, _gp, C.POINTER(C.c_float), _vp, _vp]),
    "wn_multiband3d_projected_grad_points": (_i, [_vp, _vp, _vp, _i, _sz, _f, _i, _i, C.POINTER(C.c_float), _f, _vp, _vp]),
    "wn_perlin_grad_points": (_i, [_vp, _vp, _sz, _vp, _vp]),
    "wn_perlin_grad_points_vec3": (_i, [_vp, _vp, _sz, _vp, _vp]),
    "wn_perlin_turb_grad_points": (_i, [_vp, _vp, _sz, _i, _vp, _vp]),
    "wn_perlin_fractal_grad_points": (_i, [_vp, _vp, _sz, _vp, _vp]),
    "wn_perlin_grad_grid": (_i, [_vp, _gp, _vp, _vp]),
    "wn_perlin_turb_grad_grid": (_i, [_vp, _gp, _i, _vp, _vp]),
    "wn_perlin_fractal_grad_grid": (_i, [_vp, _gp, _vp, _vp]),
    "wn_eval3d_curl_points": (_i, [_vp, _vp, _sz, _i32p, _vp, _vp]),
    "wn_multiband3d_curl_points": (_i, [_vp, _vp, _sz, _i32p, _f, _i, _i, C.POINTER(C.c_float), _f, _vp, _vp]),
    "wn_eval3d_curl_grid": (_i, [_vp, _gp, _i32p, _vp, _vp]),
    "wn_multiband3d_curl_grid": (_i, [_vp, _gp, _i32p, _f, _i, _i, C.POINTER(C.c_float), _f, _vp, _vp]),
    "wn_wavelet_texture_points": (_i, [_vp, _i, _d, _i, _vp, _vp, _sz, _vp, _vp]),
    "wn_noise_texture_points": (_i, [_vp, _d, _i, _vp, _vp, _sz, _vp, _vp]),
    "wn_scalar_eval3d": (_i, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "wn_scalar_eval2d": (_i, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "wn_scalar_eval3d_projected": (_i, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "wn_scalar_perlin": (_i, [_vp, _d, _d, _d, C.POINTER(C.c_double)]),
    "wn_scalar_perlin_vec3": (_i, [_vp, C.POINTER(C.c_float), _i, _i, C.POINTER(C.c_double)]),
    "wn_scalar_wavelet_texture": (_i, [_vp, _i, _d, _i, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "wn_scalar_noise_texture": (_i, [_vp, _d, _i, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "wn_scalar_stats": (_i, [C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]),
    "wn_scalar_shutdown": (_i, []),
}

# name -> (restype, argtypes); every symbol include/wnoise_perlin_curl.h declares (SIGNATURES mirrors include/wnoise.h alone).
WN_PERLIN_CURL_NOISE, WN_PERLIN_CURL_TURB, WN_PERLIN_CURL_FRACTAL = range(3)
PERLIN_CURL_SIGNATURES = {
    "wn_perlin_curl_points": (_i, [_vp, _vp, _sz, _i32p, _vp, _vp]),
    "wn_perlin_curl_points_vec3": (_i, [_vp, _vp, _sz, _i, _i, _i32p, _vp, _vp]),
    "wn_perlin_curl_grid": (_i, [_vp, _gp, _i, _i, _i32p, _vp, _vp]),
}

# name -> (restype, argtypes); every symbol include/wnoise_footprint.h declares.
_fp = C.POINTER(C.c_float)
FOOTPRINT_SIGNATURES = {
    "wn_multiband3d_footprint_points": (_i, [_vp, _vp, _vp, _sz, _i, _i, _fp, _f, _i, _vp, _vp]),
    "wn_multiband3d_projected_footprint_points": (_i, [_vp, _vp, _vp, _i, _vp, _sz, _i, _i, _fp, _f, _i, _vp, _vp]),
    "wn_multiband3d_footprint_grad_points": (_i, [_vp, _vp, _vp, _sz, _i, _i, _fp, _f, _i, _vp, _vp]),
    "wn_multiband3d_projected_footprint_grad_points": (_i, [_vp, _vp, _vp, _i, _vp, _sz, _i, _i, _fp, _f, _i, _vp, _vp]),
    "wn_wavelet_multiband_texture_points": (_i, [_vp, _d, _i, _i, _fp, _f, _i, _vp, _vp, _vp, _sz, _vp, _vp]),
}

# name -> (restype, argtypes); every symbol include/wnoise_perlin_footprint.h declares.
_points_fp = (_i, [_vp, _vp, _vp, _sz, _i, _f, _i, _vp, _vp])  # perm, xyz, s, n, depth / octaves, bias, fade, out, stream
PERLIN_FOOTPRINT_SIGNATURES = {
    "wn_perlin_turb_footprint_points": _points_fp,
    "wn_perlin_fractal_footprint_points": _points_fp,
    "wn_perlin_turb_footprint_grad_points": _points_fp,
    "wn_perlin_fractal_footprint_grad_points": _points_fp,
    "wn_noise_multiband_texture_points": (_i, [_vp, _d, _i, _f, _i, _vp, _vp, _vp, _sz, _vp, _vp]),
}

# name -> (restype, argtypes); every symbol include/wnoise_multiband2d.h declares.
_grid_mb2d = (_i, [_vp, _gp, _f, _i, _i, _fp, _f, _vp, _vp])            # tile, grid, s, first_band, nbands, w, var, out, stream
_points_mb2d = (_i, [_vp, _vp, _sz, _f, _i, _i, _fp, _f, _vp, _vp])     # tile, xy, n, s, first_band, nbands, w, var, out, stream
_points_fp_mb2d = (_i, [_vp, _vp, _vp, _sz, _i, _i, _fp, _f, _i, _vp, _vp])  # tile, xy, s, n, first_band, nbands, w, var, fade, out, stream
MULTIBAND2D_SIGNATURES = {
    "wn_multiband2d_grid": _grid_mb2d,
    "wn_multiband2d_grad_grid": _grid_mb2d,
    "wn_multiband2d_points": _points_mb2d,
    "wn_multiband2d_grad_points": _points_mb2d,
    "wn_multiband2d_footprint_points": _points_fp_mb2d,
    "wn_multiband2d_footprint_grad_points": _points_fp_mb2d,
}

# name -> (restype, argtypes); every symbol include/wnoise_advect.h declares, and its wn_advect.
WN_ADVECT_EULER, WN_ADVECT_MIDPOINT, WN_ADVECT_RK4 = range(3)


class wn_advect(C.Structure):
    _fields_ = [("method", C.c_int32), ("steps", C.c_int32), ("h", C.c_float), ("gain", C.c_float),
                ("drift", C.c_float * 3), ("traj_every", C.c_int32)]


_ap = C.POINTER(wn_advect)
ADVECT_SIGNATURES = {
    "wn_eval3d_curl_advect_points": (_i, [_vp, _vp, _sz, _i32p, _ap, _vp, _vp, _vp]),
    "wn_multiband3d_curl_advect_points": (_i, [_vp, _vp, _sz, _i32p, _f, _i, _i, _fp, _f, _ap, _vp, _vp, _vp]),
    "wn_advect_launch_steps": (_i, []),
}

# name -> (restype, argtypes); every symbol include/wnoise_bounded.h declares, and its wn_obstacle.
WN_OBSTACLE_SPHERE, WN_OBSTACLE_CONTAINER, WN_OBSTACLE_HALFSPACE = range(3)
WN_MAX_OBSTACLES = 16


class wn_obstacle(C.Structure):
    _fields_ = [("kind", C.c_int32), ("c", C.c_float * 3), ("r", C.c_float), ("d0", C.c_float),
                ("reserved", C.c_int32 * 2)]


_op = C.POINTER(wn_obstacle)
BOUNDED_SIGNATURES = {
    # tile, xyz, n, offsets9, [s, first_band, nbands, w, var,] obstacles, nobs, out3, stream
    "wn_eval3d_curl_bounded_points": (_i, [_vp, _vp, _sz, _i32p, _op, _i, _vp, _vp]),
    "wn_multiband3d_curl_bounded_points": (_i, [_vp, _vp, _sz, _i32p, _f, _i, _i, _fp, _f, _op, _i, _vp, _vp]),
    # tile, xyz_in, n, offsets9, [s, first_band, nbands, w, var,] obstacles, nobs, a, xyz_out, traj, stream
    "wn_eval3d_curl_bounded_advect_points": (_i, [_vp, _vp, _sz, _i32p, _op, _i, _ap, _vp, _vp, _vp]),
    "wn_multiband3d_curl_bounded_advect_points": (_i, [_vp, _vp, _sz, _i32p, _f, _i, _i, _fp, _f, _op, _i, _ap, _vp, _vp, _vp]),
}

# name -> (restype, argtypes); every symbol include/wnoise_perlin_advect.h declares.
PERLIN_ADVECT_SIGNATURES = {
    "wn_perlin_curl_advect_points": (_i, [_vp, _vp, _sz, _i, _i, _i32p, _ap, _vp, _vp, _vp]),
    "wn_perlin_advect_launch_steps": (_i, [_i, _i, _i]),
}

# name -> (restype, argtypes); every symbol include/wnoise_perlin_bricks.h declares.  (Named as SIGNATURES_PERLIN_BOUNDED is.)
SIGNATURES_PERLIN_BRICKS = {
    # perm, grid, [kind,] [depth,] [offsets9,] bricks, n, out, stream
    "wn_perlin_bricks": (_i, [_vp, _gp, _vp, _sz, _vp, _vp]),
    "wn_perlin_turb_bricks": (_i, [_vp, _gp, _i, _vp, _sz, _vp, _vp]),
    "wn_perlin_fractal_bricks": (_i, [_vp, _gp, _vp, _sz, _vp, _vp]),
    "wn_perlin_grad_bricks": (_i, [_vp, _gp, _vp, _sz, _vp, _vp]),
    "wn_perlin_turb_grad_bricks": (_i, [_vp, _gp, _i, _vp, _sz, _vp, _vp]),
    "wn_perlin_fractal_grad_bricks": (_i, [_vp, _gp, _vp, _sz, _vp, _vp]),
    "wn_perlin_curl_bricks": (_i, [_vp, _gp, _i, _i, _i32p, _vp, _sz, _vp, _vp]),
}

# name -> (restype, argtypes); every symbol include/wnoise_perlin_bounded.h declares.  (The name leads with SIGNATURES:
# tests/test_bounded_bricks_host.py pins the set of names that end with it.)
SIGNATURES_PERLIN_BOUNDED = {
    # perm, xyz, n, [kind, depth,] offsets9, [obstacles, nobs,] out3, stream
    "wn_perlin_curl_potential_points_f64": (_i, [_vp, _vp, _sz, _i32p, _vp, _vp]),
    "wn_perlin_curl_potential_points_f32": (_i, [_vp, _vp, _sz, _i, _i, _i32p, _vp, _vp]),
    "wn_perlin_curl_bounded_points_f64": (_i, [_vp, _vp, _sz, _i32p, _op, _i, _vp, _vp]),
    "wn_perlin_curl_bounded_points_f32": (_i, [_vp, _vp, _sz, _i, _i, _i32p, _op, _i, _vp, _vp]),
    # perm, xyz_in, n, kind, depth, offsets9, obstacles, nobs, a, xyz_out, traj, stream
    "wn_perlin_curl_bounded_advect_points_f64": (_i, [_vp, _vp, _sz, _i, _i, _i32p, _op, _i, _ap, _vp, _vp, _vp]),
    "wn_perlin_bounded_advect_launch_steps": (_i, [_i, _i, _i, _i]),
}

# name -> (restype, argtypes); every symbol include/wnoise_perlin_bounded_bricks.h declares.
SIGNATURES_PERLIN_BOUNDED_BRICKS = {
    # perm, grid, kind, depth, offsets9, obstacles, nobs, bricks, n, out, stream
    "wn_perlin_curl_bounded_bricks": (_i, [_vp, _gp, _i, _i, _i32p, _op, _i, _vp, _sz, _vp, _vp]),
}

# name -> (restype, argtypes); every symbol include/wnoise_curl2d.h declares, and its wn_advect2d.
class wn_advect2d(C.Structure):
    _fields_ = [("method", C.c_int32), ("steps", C.c_int32), ("h", C.c_float), ("gain", C.c_float),
                ("drift", C.c_float * 2), ("traj_every", C.c_int32)]


_a2p = C.POINTER(wn_advect2d)
CURL2D_SIGNATURES = {
    "wn_multiband2d_curl_points": _points_mb2d,
    "wn_multiband2d_curl_grid": _grid_mb2d,
    # tile, xy_in, n, s, first_band, nbands, w, var, a, xy_out, traj, stream
    "wn_multiband2d_curl_advect_points": (_i, [_vp, _vp, _sz, _f, _i, _i, _fp, _f, _a2p, _vp, _vp, _vp]),
    "wn_advect2d_launch_steps": (_i, [_i, _i]),
}

# name -> (restype, argtypes); every symbol include/wnoise_bounded2d.h declares, and its wn_obstacle2d.
class wn_obstacle2d(C.Structure):
    _fields_ = [("kind", C.c_int32), ("c", C.c_float * 2), ("r", C.c_float), ("d0", C.c_float),
                ("reserved", C.c_int32 * 3)]


_o2p = C.POINTER(wn_obstacle2d)
BOUNDED2D_SIGNATURES = {
    # tile, xy, n, s, first_band, nbands, w, var, obstacles, nobs, flow2, out2, stream
    "wn_multiband2d_curl_bounded_points": (_i, [_vp, _vp, _sz, _f, _i, _i, _fp, _f, _o2p, _i, _fp, _vp, _vp]),
    # tile, grid, s, first_band, nbands, w, var, obstacles, nobs, flow2, out, stream
    "wn_multiband2d_curl_bounded_grid": (_i, [_vp, _gp, _f, _i, _i, _fp, _f, _o2p, _i, _fp, _vp, _vp]),
    # tile, xy_in, n, s, first_band, nbands, w, var, obstacles, nobs, flow2, a, xy_out, traj, stream
    "wn_multiband2d_curl_bounded_advect_points": (_i, [_vp, _vp, _sz, _f, _i, _i, _fp, _f, _o2p, _i, _fp, _a2p, _vp, _vp, _vp]),
}

# name -> (restype, argtypes); every symbol include/wnoise_bricks.h declares.
WN_BRICK = 8
BRICKS_SIGNATURES = {
    # tile, grid, bricks, n, [s, first_band, nbands, w, var,] out, stream
    "wn_eval3d_bricks": (_i, [_vp, _gp, _vp, _sz, _vp, _vp]),
    "wn_multiband3d_bricks": (_i, [_vp, _gp, _vp, _sz, _f, _i, _i, _fp, _f, _vp, _vp]),
}

# name -> (restype, argtypes); every symbol include/wnoise_brick_fields.h declares.
BRICK_FIELDS_SIGNATURES = {
    # tile, grid, bricks, n, [offsets9,] [s, first_band, nbands, w, var,] out, stream
    "wn_eval3d_grad_bricks": (_i, [_vp, _gp, _vp, _sz, _vp, _vp]),
    "wn_multiband3d_grad_bricks": (_i, [_vp, _gp, _vp, _sz, _f, _i, _i, _fp, _f, _vp, _vp]),
    "wn_eval3d_curl_bricks": (_i, [_vp, _gp, _vp, _sz, _i32p, _vp, _vp]),
    "wn_multiband3d_curl_bricks": (_i, [_vp, _gp, _vp, _sz, _i32p, _f, _i, _i, _fp, _f, _vp, _vp]),
}

# name -> (restype, argtypes); every symbol include/wnoise_bounded_bricks.h declares.
BOUNDED_BRICKS_SIGNATURES = {
    # tile, grid, bricks, n, offsets9, [s, first_band, nbands, w, var,] obstacles, nobs, out, stream
    "wn_eval3d_curl_bounded_bricks": (_i, [_vp, _gp, _vp, _sz, _i32p, _op, _i, _vp, _vp]),
    "wn_multiband3d_curl_bounded_bricks": (_i, [_vp, _gp, _vp, _sz, _i32p, _f, _i, _i, _fp, _f, _op, _i, _vp, _vp]),
}

_lib = None


def load():
    """Load libwnoise_hip.so or raise: there is no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `make -C {HERE}` (or "
            "__graft_entry__.build()).  This package has no CPU implementation.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in (*SIGNATURES.items(), *PERLIN_CURL_SIGNATURES.items(), *FOOTPRINT_SIGNATURES.items(),
                              *PERLIN_FOOTPRINT_SIGNATURES.items(), *MULTIBAND2D_SIGNATURES.items(),
                              *ADVECT_SIGNATURES.items(), *BOUNDED_SIGNATURES.items(), *PERLIN_ADVECT_SIGNATURES.items(),
                              *CURL2D_SIGNATURES.items(), *BOUNDED2D_SIGNATURES.items(), *BRICKS_SIGNATURES.items(),
                              *BRICK_FIELDS_SIGNATURES.items(), *BOUNDED_BRICKS_SIGNATURES.items(),
                              *SIGNATURES_PERLIN_BOUNDED.items(), *SIGNATURES_PERLIN_BRICKS.items(),
                              *SIGNATURES_PERLIN_BOUNDED_BRICKS.items()):
        fn = getattr(lib, name)  # AttributeError if the ABI lost a symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc):
    if rc != WN_OK:
        raise WnError(rc, load().wn_last_error().decode("utf-8", "replace"))
