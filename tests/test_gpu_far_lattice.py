"""Dense grids and point lists far from the origin, up to the planners' gate at 1e6 cells.

Every fast dense-grid kernel sizes its LDS coefficient box on the host from wn::lattice_step (csrc/wn_internal.hpp), which
models the float32 rounding of a coordinate as slack = pmax * 4.8e-7 and refuses lattices whose coordinates could pass 1e6
cells.  The route tables of test_gpu_dispatch / test_gpu_gradient / test_gpu_curl stay within a few hundred cells of the
origin, where slack is 1e-4 and decides nothing.  The tables here move only z0 (or z_const):

 * FAR_VALUE / FAR_DERIV: per fast kernel, rows at coordinates of about 1e3, 1e4 and 1e5 cells with divisors that are not
   powers of two (the coordinates really round), one power-of-two row a whole number of tile periods out (about 1e6 planes),
   and pairs of rows one plane apart on both sides of the check that binds first for the row's step -- derived with the host
   checks restated in tests/_far_plan.py, not guessed; the CPU tests recompute them.  The gradient rows are served by the
   curl entry points too.
 * CPU precondition: the host's exact evaluators (libwnoise_host.so) against the float64 reference at every far row, within
   the near rows' tolerances -- so that a failure on the GPU is a finding about a kernel, not about the bound.
 * GPU: the trace child runs every row once under `rocprofv3 --kernel-trace`; the value tests run both tiers into
   sentinel-filled frames at leads 0 and 1 and compare with WN_GRID_EXACT, the oracle and the float64 reference;
   periodicity compares the power-of-two rows with the same planes next to the origin, bit for bit.
 * Point lists: magnitudes 2^10 .. 2^30 in both signs, the binades where p - 0.5f rounds, and lists collapsed onto one
   point or onto runs of identical points at chunked length.

Run as `python tests/test_gpu_far_lattice.py --child` it is the trace child.
"""
import csv
import ctypes as C
import glob
import importlib
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _far_plan as fp  # noqa: E402
import _ref64  # noqa: E402
import _ref64_curl  # noqa: E402
import _ref64_grad  # noqa: E402
import _ref64_footprint as F  # noqa: E402
import _ref64_perlin_curl as RC  # noqa: E402
import _ref64_perlin_grad as RG  # noqa: E402
import _ref_perlin_footprint as RPF  # noqa: E402
import test_gpu_curl as tc  # noqa: E402
import test_gpu_dispatch as td  # noqa: E402
import test_gpu_footprint as tfp  # noqa: E402
import test_gpu_gradient as tg  # noqa: E402
import test_gpu_perlin_curl as tpc  # noqa: E402
import test_gpu_perlin_footprint as tpf  # noqa: E402
import test_gpu_perlin_grad as tpg  # noqa: E402
import test_gpu_point_dispatch as tp  # noqa: E402
from _frame import Frame  # noqa: E402

PKG = os.path.join(ROOT, "wavelet-noise-in-ray-tracing_amd")
f32 = np.float32
MBP, STRIP, EXACT_LDS, DIRECT, SEP = td.MBP, td.STRIP, td.EXACT_LDS, td.DIRECT, td.SEP
GSEP, GDIRECT = tg.SEP, tg.DIRECT_PADDED
W5, W8 = td.W5, tg.W8
INV32 = f32(1.0) / np.sqrt(f32(0.18402))
TILE_N = {"t128": 128, "t32": 32, "t16": 16, "t8": 8, "t6": 6, "empty": 0}
CUS = 256   # compute units of an MI355X: the strip kernel's owner ranges (strip_try) depend on them

# ---- the far route tables ------------------------------------------------------------------------------------------------
# (name, call, kernel of the default tier, edge).  Calls are td.ROUTES' tuples, and ("vz", tile, den, nx, ny, z_const, octave):
# wavelet_volume's lattice with WN_Z_CONST.  edge = (side, chain link, check): the row is the last z0 at which that link of
# the entry point's chain (_far_plan: "mbp", "strip", "sep", "exact_lds", "brick") still takes the lattice ("in"), or the first
# at which `check` declines it ("out").  The comments give step, pmax and slack of the band that decides (the top band) as
# lattice_step computes them at that link, and the deciding expression.  Out rows name the kernel the lattice falls to.
FAR_VALUE = [
    # -- mbp1
    ("mbp1_1e3", ('v', 't128', 600, 512, 6, 4690, 4699, 4), MBP.format(1), None),
     # step 0.21333 pmax 1003.5 slack 0.00048
    ("mbp1_1e4", ('v', 't128', 600, 512, 6, 46878, 46887, 4), MBP.format(1), None),
     # step 0.21333 pmax 10003.6 slack 0.00480
    ("mbp1_1e5", ('v', 't128', 600, 512, 6, 468752, 468761, 4), MBP.format(1), None),
     # step 0.21333 pmax 100003.3 slack 0.04800
    ("mbp1_pow2", ('v', 't128', 512, 512, 6, 999939, 999948, 4), MBP.format(1), None),
     # step 0.25000 pmax 249988.0 slack 0.11999 (den a power of two: coordinates exact; z0 = 3 + 1953 * 512, whole tile periods)
    ("mbp1_K_in", ('v', 't128', 449, 512, 6, 32539, 32548, 4), MBP.format(1), ("in", "mbp", "K")),
     # step 0.28508 pmax 9279.7 slack 0.00445: 7 * step + slack = 1.9999999 (K <= 5 while < 2)
    ("mbp1_K_out", ('v', 't128', 449, 512, 6, 32540, 32549, 4), STRIP, ("out", "mbp", "K")),
     # step 0.28508 pmax 9280.0 slack 0.00445: 7 * step + slack = 2.0000001 (K <= 5 while < 2)
    ("mbp1_two_mids_in", ('v', 't128', 600, 512, 6, 3515611, 3515620, 4), MBP.format(1), ("in", "mbp", "two_mids")),
     # step 0.21333 pmax 749999.9 slack 0.36000: 3 * step + slack = 1.0000000 (<= 1)
    ("mbp1_two_mids_out", ('v', 't128', 600, 512, 6, 3515612, 3515621, 4), EXACT_LDS, ("out", "mbp", "two_mids")),
     # step 0.21333 pmax 750000.1 slack 0.36000: 3 * step + slack = 1.0000001 (<= 1)
    ("mbp1_gate_in", ('v', 't128', 750, 512, 6, 5859360, 5859369, 4), MBP.format(1), ("in", "mbp", "gate")),
     # step 0.17067 pmax 1000000.0 slack 0.48000: pmax (<= 1e6)
    ("mbp1_gate_out", ('v', 't128', 750, 512, 6, 5859361, 5859370, 4), DIRECT, ("out", "mbp", "gate")),
     # step 0.17067 pmax 1000000.1 slack 0.48000: pmax (<= 1e6)
    # -- mbp3
    ("mbp3_1e3", ('m', 't128', 600, 512, 8, 4690, 4699, -16.0, 2, 3, [1.0] * 3), MBP.format(3), None),
     # step 0.21333 pmax 1003.5 slack 0.00048
    ("mbp3_1e4", ('m', 't128', 600, 512, 8, 46878, 46887, -16.0, 2, 3, [1.0] * 3), MBP.format(3), None),
     # step 0.21333 pmax 10003.6 slack 0.00480
    ("mbp3_1e5", ('m', 't128', 600, 512, 8, 468752, 468761, -16.0, 2, 3, [1.0] * 3), MBP.format(3), None),
     # step 0.21333 pmax 100003.3 slack 0.04800
    ("mbp3_pow2", ('m', 't128', 512, 512, 8, 999427, 999436, -16.0, 2, 3, [1.0] * 3), MBP.format(3), None),
     # step 0.25000 pmax 249860.0 slack 0.11993 (den a power of two: coordinates exact; z0 = 3 + 488 * 2048, whole tile periods)
    ("mbp3_box_in", ('m', 't128', 449, 512, 8, 32536, 32545, -16.0, 2, 3, [1.0] * 3), MBP.format(3), ("in", "mbp", "box")),
     # step 0.28508 pmax 9278.9 slack 0.00445: box floats 4*4*44 + 4*4*80 + 5*5*156 = 5884 (<= 6144)
    ("mbp3_box_out", ('m', 't128', 449, 512, 8, 32537, 32546, -16.0, 2, 3, [1.0] * 3), SEP(3, 2), ("out", "mbp", "box")),
     # step 0.28508 pmax 9279.1 slack 0.00445: box floats 4*4*44 + 5*5*80 + 5*5*156 = 6604 (<= 6144)
    ("mbp3_two_mids_in", ('m', 't128', 600, 512, 8, 3515611, 3515620, -16.0, 2, 3, [1.0] * 3), MBP.format(3), ("in", "mbp", "two_mids")),
     # step 0.21333 pmax 749999.9 slack 0.36000: 3 * step + slack = 1.0000000 (<= 1)
    ("mbp3_two_mids_out", ('m', 't128', 600, 512, 8, 3515612, 3515621, -16.0, 2, 3, [1.0] * 3), DIRECT, ("out", "mbp", "two_mids")),
     # step 0.21333 pmax 750000.1 slack 0.36000: 3 * step + slack = 1.0000001 (<= 1)
    # -- mbp5
    ("mbp5_1e3", ('m', 't128', 600, 512, 8, 4690, 4699, -16.0, 0, 5, W5), MBP.format(5), None),
     # step 0.21333 pmax 1003.5 slack 0.00048
    ("mbp5_1e4", ('m', 't128', 600, 512, 8, 46878, 46887, -16.0, 0, 5, W5), MBP.format(5), None),
     # step 0.21333 pmax 10003.6 slack 0.00480
    ("mbp5_1e5", ('m', 't128', 600, 512, 8, 468752, 468761, -16.0, 0, 5, W5), MBP.format(5), None),
     # step 0.21333 pmax 100003.3 slack 0.04800
    ("mbp5_pow2", ('m', 't128', 512, 512, 8, 999427, 999436, -16.0, 0, 5, W5), MBP.format(5), None),
     # step 0.25000 pmax 249860.0 slack 0.11993 (den a power of two: coordinates exact; z0 = 3 + 122 * 8192, whole tile periods)
    ("mbp5_box_in", ('m', 't128', 492, 512, 8, 455716, 455725, -16.0, 0, 5, W5), MBP.format(5), ("in", "mbp", "box")),
     # step 0.26016 pmax 118563.6 slack 0.05691: box floats 4*4*16 + 4*4*24 + 4*4*44 + 4*4*76 + 5*5*140 = 6060 (<= 6144)
    ("mbp5_box_out", ('m', 't128', 492, 512, 8, 455717, 455726, -16.0, 0, 5, W5), SEP(5, 2), ("out", "mbp", "box")),
     # step 0.26016 pmax 118563.9 slack 0.05691: box floats 4*4*16 + 4*4*24 + 4*4*44 + 4*4*76 + 5*5*144 = 6160 (<= 6144)
    ("mbp5_gate_in", ('m', 't128', 750, 512, 8, 5859360, 5859369, -16.0, 0, 5, W5), MBP.format(5), ("in", "mbp", "gate")),
     # step 0.17067 pmax 1000000.0 slack 0.48000: pmax (<= 1e6)
    ("mbp5_gate_out", ('m', 't128', 750, 512, 8, 5859361, 5859370, -16.0, 0, 5, W5), DIRECT, ("out", "mbp", "gate")),
     # step 0.17067 pmax 1000000.1 slack 0.48000: pmax (<= 1e6)
    # -- strip
    ("strip_1e3", ('v', 't128', 449, 256, 5, 3510, 3519, 4), STRIP, None),
     # step 0.28508 pmax 1004.2 slack 0.00048
    ("strip_1e4", ('v', 't128', 449, 256, 5, 35081, 35090, 4), STRIP, None),
     # step 0.28508 pmax 10004.4 slack 0.00480
    ("strip_1e5", ('v', 't128', 449, 256, 5, 350784, 350793, 4), STRIP, None),
     # step 0.28508 pmax 100004.3 slack 0.04800
    ("strip_pow2", ('v', 't128', 512, 256, 5, 999939, 999948, 4), STRIP, None),
     # step 0.25000 pmax 249988.0 slack 0.11999 (den a power of two: coordinates exact; z0 = 3 + 1953 * 512, whole tile periods)
    ("strip_two_mids_in", ('v', 't128', 385, 256, 5, 16264, 16273, 4), STRIP, ("in", "strip", "two_mids")),
     # step 0.33247 pmax 5411.2 slack 0.00260: 3 * step + slack = 1.0000000 (<= 1)
    ("strip_two_mids_out", ('v', 't128', 385, 256, 5, 16265, 16274, 4), EXACT_LDS, ("out", "strip", "two_mids")),
     # step 0.33247 pmax 5411.6 slack 0.00260: 3 * step + slack = 1.0000002 (<= 1)
    ("strip_two_mids_018_in", ('v', 't128', 711, 768, 5, 5322251, 5322260, 4), STRIP, ("in", "strip", "two_mids")),
     # step 0.18003 pmax 958157.5 slack 0.45992: 3 * step + slack = 1.0000000 (<= 1)
    ("strip_two_mids_018_out", ('v', 't128', 711, 768, 5, 5322252, 5322261, 4), EXACT_LDS, ("out", "strip", "two_mids")),
     # step 0.18003 pmax 958157.7 slack 0.45992: 3 * step + slack = 1.0000001 (<= 1)
    # -- sep11
    ("sep11_1e3", ('v', 't128', 712, 768, 5, 5565, 5574, 4), SEP(1, 1), None),
     # step 0.17978 pmax 1003.1 slack 0.00048
    ("sep11_1e4", ('v', 't128', 712, 768, 5, 55628, 55637, 4), SEP(1, 1), None),
     # step 0.17978 pmax 10003.2 slack 0.00480
    ("sep11_1e5", ('v', 't128', 712, 768, 5, 556253, 556262, 4), SEP(1, 1), None),
     # step 0.17978 pmax 100003.2 slack 0.04800
    ("sep11_pow2", ('v', 't128', 1024, 768, 5, 999427, 999436, 4), SEP(1, 1), None),
     # step 0.12500 pmax 124930.5 slack 0.05997 (den a power of two: coordinates exact; z0 = 3 + 976 * 1024, whole tile periods)
    ("sep11_two_mids_in", ('v', 't128', 712, 768, 5, 5338527, 5338536, 4), SEP(1, 1), ("in", "sep", "two_mids")),
     # step 0.17978 pmax 959737.8 slack 0.46067: 3 * step + slack = 1.0000000 (<= 1)
    ("sep11_two_mids_out", ('v', 't128', 712, 768, 5, 5338528, 5338537, 4), EXACT_LDS, ("out", "sep", "two_mids")),
     # step 0.17978 pmax 959738.0 slack 0.46067: 3 * step + slack = 1.0000001 (<= 1)
    ("sep11_gate_in", ('v', 't128', 1000, 768, 5, 7812483, 7812492, 4), SEP(1, 1), ("in", "sep", "gate")),
     # step 0.12800 pmax 1000000.0 slack 0.48000: pmax (<= 1e6)
    ("sep11_gate_out", ('v', 't128', 1000, 768, 5, 7812484, 7812493, 4), DIRECT, ("out", "sep", "gate")),
     # step 0.12800 pmax 1000000.1 slack 0.48000: pmax (<= 1e6)
    # -- sep11, 16 planes per brick (one band, 256-wide bricks, nz >= 16): BZ = 16 while extent(16) = floor(15 * step + slack) + 4
    #    stays within the 6 box rows, else 8 -- the same kernel name either way (SEP_BZ below names the brick shape)
    ("sep11_bz16_1e3", ('v', 't128', 712, 768, 5, 5565, 5585, 4), SEP(1, 1), None),
     # step 0.17978 pmax 1005.0 slack 0.00048: 15 * step + slack = 2.6971116 (< 3: 16 planes)
    ("sep11_bz16_1e4", ('v', 't128', 712, 768, 5, 55628, 55648, 4), SEP(1, 1), None),
     # step 0.17978 pmax 10005.1 slack 0.00480: 15 * step + slack = 2.7014317
    ("sep11_bz16_1e5", ('v', 't128', 712, 768, 5, 556253, 556273, 4), SEP(1, 1), None),
     # step 0.17978 pmax 100005.1 slack 0.04800: 15 * step + slack = 2.7446317
    ("sep11_bz16_in", ('v', 't128', 712, 768, 5, 3515599, 3515619, 4), SEP(1, 1), None),
     # step 0.17978 pmax 632022.4 slack 0.30337: 15 * step + slack = 2.99999996 (< 3: 16 planes)
    ("sep11_bz16_out", ('v', 't128', 712, 768, 5, 3515600, 3515620, 4), SEP(1, 1), None),
     # step 0.17978 pmax 632022.6 slack 0.30337: 15 * step + slack = 3.00000004 (extent(16) = 7 rows: 8 planes per brick)
    # -- sep12
    ("sep12_1e3", ('v', 't128', 491, 998, 5, 3838, 3847, 4), SEP(1, 2), None),
     # step 0.26069 pmax 1003.9 slack 0.00048
    ("sep12_1e4", ('v', 't128', 491, 998, 5, 38362, 38371, 4), SEP(1, 2), None),
     # step 0.26069 pmax 10004.0 slack 0.00480
    ("sep12_1e5", ('v', 't128', 491, 998, 5, 383596, 383605, 4), SEP(1, 2), None),
     # step 0.26069 pmax 100003.9 slack 0.04800
    ("sep12_pow2", ('v', 't128', 512, 998, 5, 999939, 999948, 4), SEP(1, 2), None),
     # step 0.25000 pmax 249988.0 slack 0.11999 (den a power of two: coordinates exact; z0 = 3 + 1953 * 512, whole tile periods)
    ("sep12_two_mids_in", ('v', 't128', 491, 998, 5, 1741523, 1741532, 4), SEP(1, 2), ("in", "sep", "two_mids")),
     # step 0.26069 pmax 454005.3 slack 0.21792: 3 * step + slack = 0.9999999 (<= 1)
    ("sep12_two_mids_out", ('v', 't128', 491, 998, 5, 1741524, 1741533, 4), EXACT_LDS, ("out", "sep", "two_mids")),
     # step 0.26069 pmax 454005.5 slack 0.21792: 3 * step + slack = 1.0000000 (<= 1)
    ("sep12_gate_in", ('v', 't128', 1000, 998, 5, 7812483, 7812492, 4), SEP(1, 2), ("in", "sep", "gate")),
     # step 0.12800 pmax 1000000.0 slack 0.48000: pmax (<= 1e6)
    ("sep12_gate_out", ('v', 't128', 1000, 998, 5, 7812484, 7812493, 4), DIRECT, ("out", "sep", "gate")),
     # step 0.12800 pmax 1000000.1 slack 0.48000: pmax (<= 1e6)
    # -- sep5
    ("sep5_1e3", ('m', 't128', 491, 512, 8, 3838, 3847, -16.0, 0, 5, W5), SEP(5, 2), None),
     # step 0.26069 pmax 1003.9 slack 0.00048
    ("sep5_1e4", ('m', 't128', 491, 512, 8, 38362, 38371, -16.0, 0, 5, W5), SEP(5, 2), None),
     # step 0.26069 pmax 10004.0 slack 0.00480
    ("sep5_1e5", ('m', 't128', 491, 512, 8, 383596, 383605, -16.0, 0, 5, W5), SEP(5, 2), None),
     # step 0.26069 pmax 100003.9 slack 0.04800
    ("sep5_pow2", ('m', 't128', 512, 516, 8, 999427, 999436, -16.0, 0, 5, W5), SEP(5, 1), None),
     # step 0.25000 pmax 249860.0 slack 0.11993 (den a power of two: coordinates exact; z0 = 3 + 122 * 8192, whole tile periods)
    ("sep5_two_mids_in", ('m', 't128', 491, 512, 8, 1741523, 1741532, -16.0, 0, 5, W5), SEP(5, 2), ("in", "sep", "two_mids")),
     # step 0.26069 pmax 454005.3 slack 0.21792: 3 * step + slack = 0.9999999 (<= 1)
    ("sep5_two_mids_out", ('m', 't128', 491, 512, 8, 1741524, 1741533, -16.0, 0, 5, W5), DIRECT, ("out", "sep", "two_mids")),
     # step 0.26069 pmax 454005.5 slack 0.21792: 3 * step + slack = 1.0000000 (<= 1)
    ("sep5_gate_in", ('m', 't128', 750, 516, 8, 5859360, 5859369, -16.0, 0, 5, W5), SEP(5, 1), ("in", "sep", "gate")),
     # step 0.17067 pmax 1000000.0 slack 0.48000: pmax (<= 1e6)
    ("sep5_gate_out", ('m', 't128', 750, 516, 8, 5859361, 5859370, -16.0, 0, 5, W5), DIRECT, ("out", "sep", "gate")),
     # step 0.17067 pmax 1000000.1 slack 0.48000: pmax (<= 1e6)
    # -- sep8
    ("sep8_1e3", ('m', 't128', 4001, 1000, 8, 3910, 3919, -16.0, 0, 8, [1.0] * 8), SEP(8, 2), None),
     # step 0.25594 pmax 1004.0 slack 0.00048
    ("sep8_1e4", ('m', 't128', 4001, 1000, 8, 39075, 39084, -16.0, 0, 8, [1.0] * 8), SEP(8, 2), None),
     # step 0.25594 pmax 10004.0 slack 0.00480
    ("sep8_1e5", ('m', 't128', 4001, 1000, 8, 390725, 390734, -16.0, 0, 8, [1.0] * 8), SEP(8, 2), None),
     # step 0.25594 pmax 100003.9 slack 0.04800
    ("sep8_pow2", ('m', 't128', 4096, 1000, 8, 983043, 983052, -16.0, 0, 8, [1.0] * 8), SEP(8, 2), None),
     # step 0.25000 pmax 245764.0 slack 0.11797 (den a power of two: coordinates exact; z0 = 3 + 15 * 65536, whole tile periods)
    ("sep8_two_mids_in", ('m', 't128', 4001, 768, 8, 1890042, 1890051, -16.0, 0, 8, [1.0] * 8), SEP(8, 1), ("in", "sep", "two_mids")),
     # step 0.25594 pmax 483733.1 slack 0.23219: 3 * step + slack = 0.9999999 (<= 1)
    ("sep8_two_mids_out", ('m', 't128', 4001, 768, 8, 1890043, 1890052, -16.0, 0, 8, [1.0] * 8), DIRECT, ("out", "sep", "two_mids")),
     # step 0.25594 pmax 483733.4 slack 0.23219: 3 * step + slack = 1.0000001 (<= 1)
    ("sep8_gate_in", ('m', 't128', 8001, 1000, 8, 7813459, 7813468, -16.0, 0, 8, [1.0] * 8), SEP(8, 2), ("in", "sep", "gate")),
     # step 0.12798 pmax 999999.9 slack 0.48000: pmax (<= 1e6)
    ("sep8_gate_out", ('m', 't128', 8001, 1000, 8, 7813460, 7813469, -16.0, 0, 8, [1.0] * 8), DIRECT, ("out", "sep", "gate")),
     # step 0.12798 pmax 1000000.0 slack 0.48000: pmax (<= 1e6)
    # -- exact_lds
    ("exact_lds_1e3", ('v', 't128', 384, 256, 5, 3003, 3012, 4), EXACT_LDS, None),
     # step 0.33333 pmax 1005.0 slack 1.00048
    ("exact_lds_1e4", ('v', 't128', 384, 256, 5, 30003, 30012, 4), EXACT_LDS, None),
     # step 0.33333 pmax 10005.0 slack 1.00480
    ("exact_lds_1e5", ('v', 't128', 384, 256, 5, 300003, 300012, 4), EXACT_LDS, None),
     # step 0.33333 pmax 100005.0 slack 1.04800
    ("exact_lds_pow2", ('v', 't128', 512, 256, 5, 999939, 999948, 5), EXACT_LDS, None),
     # step 0.50000 pmax 499975.0 slack 1.23999 (den a power of two: coordinates exact; z0 = 3 + 3906 * 256, whole tile periods)
    ("exact_lds_box_in", ('v', 't128', 445, 256, 5, 1098622, 1098631, 5), EXACT_LDS, ("in", "exact_lds", "box")),
     # step 0.57528 pmax 632022.4 slack 1.30337: slack includes the kernel's margin of 1 cell; box 151 * 9 * 9 = 12231 floats (<= 12288)
    ("exact_lds_box_out", ('v', 't128', 445, 256, 5, 1098623, 1098632, 5), DIRECT, ("out", "exact_lds", "box")),
     # step 0.57528 pmax 632023.0 slack 1.30337: slack includes the kernel's margin of 1 cell; box 152 * 9 * 9 = 12312 floats (<= 12288)
    ("exact_lds_gate_in", ('v', 't128', 384, 256, 5, 2999988, 2999997, 4), EXACT_LDS, ("in", "exact_lds", "gate")),
     # step 0.33333 pmax 1000000.0 slack 1.48000: pmax (<= 1e6)
    ("exact_lds_gate_out", ('v', 't128', 384, 256, 5, 2999989, 2999998, 4), DIRECT, ("out", "exact_lds", "gate")),
     # step 0.33333 pmax 1000000.3 slack 1.48000: pmax (<= 1e6)
    # -- WN_Z_CONST: pmax includes |z_const|; the plane pipeline and the strip kernel index planes and decline
    ("sep12_zconst", ("vz", "t128", 513, 300, 7, 300000.375, 4), SEP(1, 2), None),
     # step 0.24951 pmax 300076.2 slack 0.14404: 3 * step + slack = 0.8925780 (<= 1)
]

# The strip kernel's chunk_max = min(128, floor((32 - slack) / step) + 1) bounds the planes of an item.  It changes a launch
# only where an owner range is longer than it: at least 98 planes in one range, which takes at least 2 * CUS row groups
# (256 x 2045 samples per plane).  Step .28508: 32 / step = 112.25, so chunk_max falls from 113 to 112 where slack passes
# .25 * step = .07127; a range of 113 planes is then walked as two items of 57 instead of one of 113.
STRIP_CHUNK = [
    ("strip_chunk_in", ("v", "t128", 449, 256, 2045, 520716, 520829, 4), STRIP, 113),
     # step 0.28508 pmax 148477.9 slack 0.07126937: (32 - slack) / step = 112.0000004
    ("strip_chunk_out", ("v", "t128", 449, 256, 2045, 520717, 520830, 4), STRIP, 57),
     # step 0.28508 pmax 148478.1 slack 0.07126951: (32 - slack) / step = 111.9999999
]

# Gradient rows (tg.ROUTES' tuples); test_gpu_curl's run_call serves the same tuples with the curl kernels.  The fallback of
# both families is the direct kernel.
FAR_DERIV = [
    # -- brick1
    ("brick1_1e3", ('g', 't128', 600, 256, 5, 4690, 4699, 4), GSEP.format(1), None),
     # step 0.21333 pmax 1003.5 slack 0.00048
    ("brick1_1e4", ('g', 't128', 600, 256, 5, 46878, 46887, 4), GSEP.format(1), None),
     # step 0.21333 pmax 10003.6 slack 0.00480
    ("brick1_1e5", ('g', 't128', 600, 256, 5, 468752, 468761, 4), GSEP.format(1), None),
     # step 0.21333 pmax 100003.3 slack 0.04800
    ("brick1_pow2", ('g', 't128', 512, 256, 5, 999939, 999948, 4), GSEP.format(1), None),
     # step 0.25000 pmax 249988.0 slack 0.11999 (den a power of two: coordinates exact; z0 = 3 + 1953 * 512, whole tile periods)
    ("brick1_two_mids_in", ('g', 't128', 385, 256, 5, 16264, 16273, 4), GSEP.format(1), ("in", "brick", "two_mids")),
     # step 0.33247 pmax 5411.2 slack 0.00260: 3 * step + slack = 1.0000000 (<= 1)
    ("brick1_two_mids_out", ('g', 't128', 385, 256, 5, 16265, 16274, 4), GDIRECT, ("out", "brick", "two_mids")),
     # step 0.33247 pmax 5411.6 slack 0.00260: 3 * step + slack = 1.0000002 (<= 1)
    ("brick1_gate_in", ('g', 't128', 1000, 256, 5, 7812483, 7812492, 4), GSEP.format(1), ("in", "brick", "gate")),
     # step 0.12800 pmax 1000000.0 slack 0.48000: pmax (<= 1e6)
    ("brick1_gate_out", ('g', 't128', 1000, 256, 5, 7812484, 7812493, 4), GDIRECT, ("out", "brick", "gate")),
     # step 0.12800 pmax 1000000.1 slack 0.48000: pmax (<= 1e6)
    # -- brick5
    ("brick5_1e3", ('m', 't128', 600, 256, 5, 4690, 4699, -16.0, 0, 5, W8[:5]), GSEP.format(5), None),
     # step 0.21333 pmax 1003.5 slack 0.00048
    ("brick5_1e4", ('m', 't128', 600, 256, 5, 46878, 46887, -16.0, 0, 5, W8[:5]), GSEP.format(5), None),
     # step 0.21333 pmax 10003.6 slack 0.00480
    ("brick5_1e5", ('m', 't128', 600, 256, 5, 468752, 468761, -16.0, 0, 5, W8[:5]), GSEP.format(5), None),
     # step 0.21333 pmax 100003.3 slack 0.04800
    ("brick5_pow2", ('m', 't128', 512, 256, 5, 999427, 999436, -16.0, 0, 5, W8[:5]), GSEP.format(5), None),
     # step 0.25000 pmax 249860.0 slack 0.11993 (den a power of two: coordinates exact; z0 = 3 + 122 * 8192, whole tile periods)
    ("brick5_two_mids_in", ('m', 't128', 385, 256, 5, 16264, 16273, -16.0, 0, 5, W8[:5]), GSEP.format(5), ("in", "brick", "two_mids")),
     # step 0.33247 pmax 5411.2 slack 0.00260: 3 * step + slack = 1.0000000 (<= 1)
    ("brick5_two_mids_out", ('m', 't128', 385, 256, 5, 16265, 16274, -16.0, 0, 5, W8[:5]), GDIRECT, ("out", "brick", "two_mids")),
     # step 0.33247 pmax 5411.6 slack 0.00260: 3 * step + slack = 1.0000002 (<= 1)
    ("brick5_gate_in", ('m', 't128', 1000, 256, 5, 7812483, 7812492, -16.0, 0, 5, W8[:5]), GSEP.format(5), ("in", "brick", "gate")),
     # step 0.12800 pmax 1000000.0 slack 0.48000: pmax (<= 1e6)
    ("brick5_gate_out", ('m', 't128', 1000, 256, 5, 7812484, 7812493, -16.0, 0, 5, W8[:5]), GDIRECT, ("out", "brick", "gate")),
     # step 0.12800 pmax 1000000.1 slack 0.48000: pmax (<= 1e6)
    # -- WN_Z_CONST ("gs": octave scale 16, post 2)
    ("brick1_zconst", ("gs", "t128", 513, 300, 7, 0, 1, 4.0, -300000.375), GSEP.format(1), None),
     # step 0.24951 pmax 300076.2 slack 0.14404: 3 * step + slack = 0.8925780 (<= 1)
]
FAR_CURL = [(n, c, k.replace("grad3d_", "curl3d_"), e) for n, c, k, e in FAR_DERIV]

SEP_BZ = {"sep11_bz16_1e3": 16, "sep11_bz16_1e4": 16, "sep11_bz16_1e5": 16, "sep11_bz16_in": 16, "sep11_bz16_out": 8}
VALUE_FAMILIES = {"mbp1": MBP.format(1), "mbp3": MBP.format(3), "mbp5": MBP.format(5), "strip": STRIP, "sep11": SEP(1, 1),
                  "sep12": SEP(1, 2), "sep5": SEP(5, 2), "sep8": SEP(8, 2), "exact_lds": EXACT_LDS}
DERIV_FAMILIES = {"brick1": GSEP.format(1), "brick5": GSEP.format(5)}


# ---- calls -> the restated host checks -------------------------------------------------------------------------------------
def value_grid(call):
    """(fp.Grid, multiband (s, first, nbands) or None) of a value call."""
    kind = call[0]
    if kind == "v":
        den, nx, ny, z0, z1, octave = call[2:]
        return fp.Grid(den, nx, ny, z0, z1 - z0, 4.0, 2.0 ** octave, 2.0), None
    if kind == "vz":
        den, nx, ny, zc, octave = call[2:]
        return fp.Grid(den, nx, ny, 0, 1, 4.0, 2.0 ** octave, 2.0, z_const=zc), None
    if kind == "vc":
        size, octave = call[2:]
        return fp.Grid(size, size, size, 0, 1, 4.0, 2.0 ** octave, 2.0, z_const=2.0), None
    if kind == "m":
        den, nx, ny, z0, z1, s, first, nb, _w = call[2:]
        return fp.Grid(den, nx, ny, z0, z1 - z0), (s, first, nb)
    assert kind == "mc", kind
    den, nx, ny, zc, s, first, nb, _w = call[2:]
    return fp.Grid(den, nx, ny, 0, 1, z_const=zc), (s, first, nb)


def value_route(call, exact=False, aligned=True):
    g, bands = value_grid(call)
    n = TILE_N[call[1]]
    return fp.eval3d_route(g, n, exact, aligned) if bands is None else fp.multiband3d_route(g, n, exact, *bands, aligned=aligned)


def deriv_grid(call):
    kind = call[0]
    if kind == "g":
        den, nx, ny, z0, z1, octave = call[2:]
        return fp.Grid(den, nx, ny, z0, z1 - z0, 4.0, 2.0 ** octave, 2.0), None
    if kind == "gs":
        den, nx, ny, z0, z1, rng_, zc = call[2:]
        return fp.Grid(den, nx, ny, z0, z1 - z0, rng_, 16.0, 2.0, z_const=zc), None
    if kind == "m":
        den, nx, ny, z0, z1, s, first, nb, _w = call[2:]
        return fp.Grid(den, nx, ny, z0, z1 - z0), (s, first, nb)
    assert kind == "mc", kind
    den, nx, ny, zc, s, first, nb, _w = call[2:]
    return fp.Grid(den, nx, ny, 0, 1, z_const=zc), (s, first, nb)


def deriv_route(call, family, exact=False):
    g, bands = deriv_grid(call)
    return fp.deriv_route(g, TILE_N[call[1]], exact, family, bands)


def moved(call, z0):
    """The call with its slab moved to start at plane z0 (kinds with a z-slab)."""
    assert call[0] in ("v", "m", "g"), call[0]
    return call[:5] + (z0, z0 + call[6] - call[5]) + call[7:]


def top_step(call, value=True):
    """LatticeStep of the call's top band as the fast kernels' planners see it (gate lifted)."""
    g, bands = value_grid(call) if value else deriv_grid(call)
    if bands is None:
        os_ = g.octave_scale
    else:
        os_ = g.octave_scale * 2.0 ** (bands[1] + fp.active_bands(*bands) - 1)
        g = fp.Grid(g.den, g.nx, g.ny, g.z0, g.nz, g.base_range, g.octave_scale, 2.0, z_const=g.z_const if g.z_const_mode else None)
    gate, fp.GATE = fp.GATE, float("inf")
    try:
        return fp.lattice_step(g, os_, True, False, 0.0)
    finally:
        fp.GATE = gate


# ---- CPU: the tables are derived -------------------------------------------------------------------------------------------
def test_restated_planners_reproduce_the_near_tables():
    """tests/_far_plan.py names the kernel of every row of the three near tables (whose trace tests pin them)."""
    for name, call, exact, kernel in td.ROUTES:
        assert value_route(call, exact)[0] == kernel, (name, value_route(call, exact))
    for family, mod in (("grad", tg), ("curl", tc)):
        for name, call, kernel in mod.GRID_ROUTES:
            assert deriv_route(call, family)[0] == kernel, (family, name, deriv_route(call, family))


def _check_table(rows, route, value):
    by_name = {n: (c, k, e) for n, c, k, e in rows}
    assert len(by_name) == len(rows)
    for name, call, kernel, edge in rows:
        got, why = route(call)
        assert got == kernel, (name, kernel, got, why)
        ls = top_step(call, value)
        if edge is None:
            for tag, lo, hi in (("_1e3", 1e3, 1.1e3), ("_1e4", 1e4, 1.01e4), ("_1e5", 1e5, 1.001e5)):
                if name.endswith(tag):
                    assert lo <= ls.pmax <= hi, (name, ls.pmax)
            continue
        side, link, check = edge
        assert name.endswith("_" + side), name
        if side == "in":
            assert why[link] is None, (name, why)
            partner = by_name[name[:-3] + "_out"]
            assert partner[2] == ("out", link, check)
            assert partner[0] == moved(call, call[5] + 1), (name, "the out row is the next plane index")
        else:
            assert why[link] == check, (name, why)
            assert name[:-4] + "_in" in by_name
            # the checks before this one in the planner still hold: this is the one that binds
            if check == "two_mids":
                assert 3.0 * ls.step + ls.slack > 1.0 and ls.pmax <= fp.GATE
            elif check == "gate":
                assert ls.pmax > fp.GATE and (link == "exact_lds" or 3.0 * ls.step + ls.slack <= 1.0)
            elif check == "K":
                assert 7.0 * ls.step + ls.slack >= 2.0 and 3.0 * ls.step + ls.slack <= 1.0


def _band_grids(call, value):
    """(fp.Grid, oscale) of every band of a call as the fast kernels' planners pass them to lattice_step."""
    g, bands = value_grid(call) if value else deriv_grid(call)
    if bands is None:
        return [(g, g.octave_scale)]
    gb = fp.Grid(g.den, g.nx, g.ny, g.z0, g.nz, g.base_range, g.octave_scale, 2.0, z_const=g.z_const if g.z_const_mode else None)
    return [(gb, g.octave_scale * 2.0 ** (bands[1] + b)) for b in range(fp.active_bands(*bands))]


def test_lattice_step_is_what_the_tables_were_derived_from(tmp_path):
    """wn::lattice_step itself (csrc/wn_internal.hpp, compiled into tests/host_src/lattice_step_check.cpp: host code only)
    on every band of every far row, as each planner calls it (with and without |z_const|, the exact kernel's margin of
    one cell): step, pmax, slack, two_mids() and extent() are, to the last bit, what tests/_far_plan.py computes -- so a
    changed slack or gate in the header fails here, before any GPU run."""
    exe = tmp_path / "lattice_step_check"
    src = os.path.join(HERE, "host_src", "lattice_step_check.cpp")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-w", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                            "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "csrc"), src, "-o", str(exe)],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    cases = []
    for rows, value in ((FAR_VALUE + STRIP_CHUNK, True), (FAR_DERIV, False)):
        for name, call, _, _ in rows:
            for g, os_ in _band_grids(call, value):
                for with_z, margin in ((False, 0.0), (True, 0.0), (True, 1.0)):
                    cases.append((name, g, os_, with_z, margin))
    text = "".join(f"{g.den} {g.nx} {g.ny} {g.z0} {g.nz} {g.base_range!r} {os_!r} {g.post_scale!r} {int(g.z_const_mode)} "
                   f"{g.z_const!r} {int(with_z)} 1 {margin!r}\n" for _, g, os_, with_z, margin in cases)
    run = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.splitlines()
    assert len(lines) == len(cases) > 500
    refused = 0
    for (name, g, os_, with_z, margin), line in zip(cases, lines):
        ls = fp.lattice_step(g, os_, with_z, True, margin)
        if ls is None:
            assert line == "0", (name, line)
            refused += 1
            continue
        f = line.split()
        assert f[0] == "1", (name, line)
        assert (float(f[1]), float(f[2]), float(f[3])) == (ls.step, ls.pmax, ls.slack), (name, line, ls.step, ls.pmax, ls.slack)
        assert int(f[4]) == int(ls.two_mids()), (name, line)
        assert [int(v) for v in f[5:9]] == [ls.extent(k) for k in (8, 16, 256, 512)], (name, line)
    assert refused >= 10        # the gate rows


def test_far_value_table_is_derived():
    _check_table(FAR_VALUE, value_route, True)
    # every row's WN_GRID_EXACT tier: the LDS-staged exact kernel for one band while its box fits, else the direct kernel
    for name, call, kernel, edge in FAR_VALUE:
        exact = value_route(call, True)[0]
        assert exact in (EXACT_LDS, DIRECT)
        if kernel in (EXACT_LDS, DIRECT):
            assert exact == kernel, name


def test_far_derivative_tables_are_derived():
    _check_table(FAR_DERIV, lambda c: deriv_route(c, "grad"), False)
    _check_table(FAR_CURL, lambda c: deriv_route(c, "curl"), False)


def test_far_tables_cover_every_fast_kernel():
    """Per kernel: rows at 1e3, 1e4, 1e5 cells, the power-of-two row and at least one in / out pair; one WN_Z_CONST row per
    brick family; value kernels <5,*> and <8,*> in both brick widths."""
    for fams, rows in ((VALUE_FAMILIES, FAR_VALUE), (DERIV_FAMILIES, FAR_DERIV)):
        names = {n: (k, e) for n, _, k, e in rows}
        for fam, kernel in fams.items():
            for tag in ("1e3", "1e4", "1e5", "pow2"):
                assert names[f"{fam}_{tag}"][0].split(",")[0] == kernel.split(",")[0], (fam, tag)
            pairs = [n for n, (k, e) in names.items() if n.startswith(fam + "_") and e and e[0] == "in"]
            assert pairs and all(names[n][0].split(",")[0] == kernel.split(",")[0] for n in pairs), fam
    kernels = {k for _, _, k, _ in FAR_VALUE}
    assert {SEP(5, 1), SEP(5, 2), SEP(8, 1), SEP(8, 2), SEP(3, 2)} <= kernels
    for rows in (FAR_VALUE, FAR_DERIV):
        zc = [c for _, c, _, _ in rows if c[0] in ("vz", "gs")]
        assert len(zc) == 1 and 2.5e5 <= abs(zc[0][5] if zc[0][0] == "vz" else zc[0][8]) <= 3.5e5
    # divisors: every in / out pair and every magnitude row really rounds (den is no power of two)
    for _, call, _, edge in FAR_VALUE + FAR_DERIV:
        if edge is not None:
            assert call[2] & (call[2] - 1), call


def test_brick_kernel_planes_per_brick():
    """The rows of SEP_BZ reach the 16-plane brick up to the plane index where slack takes extent(16) to 7 rows, the next
    one the 8-plane brick; every other sep11 row has nz 9 (8 planes); without slack the out row would keep 16 planes."""
    by_name = {n: c for n, c, _, _ in FAR_VALUE}
    assert by_name["sep11_bz16_out"] == moved(by_name["sep11_bz16_in"], by_name["sep11_bz16_in"][5] + 1)
    for name, call, kernel, _ in FAR_VALUE:
        if kernel != SEP(1, 1):
            continue
        g, _ = value_grid(call)
        assert fp.sep_brick_planes(g, 128, [g.octave_scale]) == SEP_BZ.get(name, 8), name
        assert (g.nz >= 16) == (name in SEP_BZ) and g.nx == 768
    saved = fp.SLACK_PER_CELL
    try:
        fp.SLACK_PER_CELL = 0.0
        g, _ = value_grid(by_name["sep11_bz16_out"])
        assert fp.sep_brick_planes(g, 128, [g.octave_scale]) == 16
    finally:
        fp.SLACK_PER_CELL = saved


@pytest.mark.parametrize("den,planes,rows,what", [(449, 8, 5, "the plane pipeline's K"), (712, 16, 6, "the 16-plane brick's box rows"),
                                                  (385, 8, 6, "the brick kernels' box rows at step .3325"),
                                                  (449, 113, 37, "the strip kernel's planes of an item")])
def test_float32_plane_coordinates_never_use_the_slack(den, planes, rows, what):
    """Why no VALUE test can notice a smaller slack on these lattices: slack is a worst-case bound (4 ulp of pmax), and along
    z -- the only axis that can be moved far -- the float32 coordinates ((i / den) * 4) * 16 * 2 round once (the three
    products are by powers of two), so `planes` consecutive planes never touch more coefficient rows than the exact step
    gives: mid(last) - mid(first) + 3 <= rows at EVERY plane index up to the gate.  A fast kernel that a wrong slack lets
    take a lattice one plane index past an edge (or anywhere up to the gate) still finds its taps inside the box it was
    given: the far rows see such a change as a change of kernel (the trace, the bit comparison of rows that fall to an exact
    kernel, the restated planners, lattice_step_check), never as a value outside its bound."""
    step = 128.0 / den
    z = np.arange(0, int(fp.GATE / step) + planes)
    c = _ref64.lattice_coords(z, den, 4.0, 16.0, 2.0)
    mid = np.ceil(c - f32(0.5)).astype(np.int64)
    span = mid[planes - 1:] - mid[:len(mid) - planes + 1]
    assert int(span.max()) + 3 <= rows, (what, int(span.max()) + 3)
    assert int(math.floor((planes - 1) * step)) + 1 + 3 <= rows       # the capacity without slack (extent(); strip: kPlanes)


def test_strip_kernel_slack_edges():
    """strip_try uses slack in three places.  two_mids: the strip_two_mids rows.  The column test 255 * step + slack + 7 <= 96
    cannot bind inside two_mids and the gate: step <= 1/3 and slack <= 0.48 give at most 85 + 0.48 + 7.  chunk_max: the
    STRIP_CHUNK rows, one plane index apart, are walked in items of 113 and of 57 planes."""
    assert 255.0 / 3.0 + fp.GATE * fp.SLACK_PER_CELL + 7.0 < 96.0
    (n_in, c_in, k_in, len_in), (n_out, c_out, k_out, len_out) = STRIP_CHUNK
    assert c_out == moved(c_in, c_in[5] + 1)
    for call, kernel, want in ((c_in, k_in, len_in), (c_out, k_out, len_out)):
        assert value_route(call)[0] == kernel == STRIP
        g, _ = value_grid(call)
        assert fp.strip_items(g, CUS) == (113, want)
    # the near strip rows and the far ones never reach chunk_max: their ranges are shorter than 98 planes
    for _, call, kernel, _ in FAR_VALUE:
        if kernel == STRIP:
            g, _ = value_grid(call)
            assert fp.strip_items(g, CUS)[0] < 98


def _moved_rows():
    rows = []
    for table, route in ((FAR_VALUE + [r[:3] + (None,) for r in STRIP_CHUNK], value_route),
                         (FAR_DERIV, lambda c: deriv_route(c, "grad")), (FAR_CURL, lambda c: deriv_route(c, "curl"))):
        for name, call, kernel, _ in table:
            if route(call)[0] != kernel:
                rows.append(name)
    chunk = [fp.strip_items(value_grid(c)[0], CUS)[1] for _, c, _, _ in STRIP_CHUNK]
    return rows, chunk


def test_the_tables_notice_a_changed_slack_or_gate():
    """With slack set to 0 every "out" row of a slack edge stays with its fast kernel, and with the gate at 1e7 every "out"
    row of a gate edge does: the trace test fails on exactly those rows.  Without slack the strip kernel also takes the
    exact_lds rows at step 1/3 (3 * step is then exactly 1), as it would the near row step_1_3_at."""
    saved = fp.SLACK_PER_CELL, fp.GATE
    try:
        fp.SLACK_PER_CELL = 0.0
        rows, chunk = _moved_rows()
        want = {n for t in (FAR_VALUE, FAR_DERIV) for n, _, _, e in t if e and e[0] == "out" and e[2] != "gate"}
        want |= {n for n, c, k, _ in FAR_VALUE if k == EXACT_LDS and c[2] == 384}
        assert set(rows) == want, set(rows) ^ want
        assert chunk == [113, 113]
        fp.SLACK_PER_CELL, fp.GATE = saved[0], 1.0e7
        rows, _ = _moved_rows()
        want = {n for t in (FAR_VALUE, FAR_DERIV) for n, _, _, e in t if e and e == ("out", e[1], "gate")}
        assert set(rows) == want, set(rows) ^ want
    finally:
        fp.SLACK_PER_CELL, fp.GATE = saved


# ---- references ------------------------------------------------------------------------------------------------------------
def value_coords(call):
    """float32 coordinates (px, py, pz) of a value call in lattice_coord's order."""
    kind = call[0]
    if kind in ("v", "vz"):
        den, nx, ny = call[2:5]
        os_ = f32(2.0 ** call[-1])
        px, py = (_ref64.lattice_coords(np.arange(n), den, 4.0, os_, 2.0) for n in (nx, ny))
        pz = f32([call[5]]) if kind == "vz" else _ref64.lattice_coords(np.arange(call[5], call[6]), den, 4.0, os_, 2.0)
        return px, py, pz
    assert kind == "m", kind
    den, nx, ny, z0, z1 = call[2:7]
    return [_ref64.lattice_coords(np.arange(a, b), den) for a, b in ((0, nx), (0, ny), (z0, z1))]


def lattice_points(px, py, pz):
    """(N, 3) float32, x fastest, then y, then z: the order of the output."""
    return np.ascontiguousarray(np.stack(np.broadcast_arrays(px[None, None, :], py[None, :, None], pz[:, None, None]), -1)
                                .reshape(-1, 3), f32)


def value_shape(call):
    return (1, call[4], call[3]) if call[0] == "vz" else (call[6] - call[5], call[4], call[3])


def ref64_value(coef, call):
    if call[0] == "vz":
        return _ref64.evaluate_lattice(coef, *value_coords(call)) / np.sqrt(np.float64(f32(0.18402)))
    return td._ref64_volume(coef, call)


def oracle_value_planes(ora, coef, call, zs):
    if call[0] == "vz":
        pts = lattice_points(*value_coords(call))
        return [(ora.evaluate3d(coef, pts) * INV32).astype(f32).reshape(call[4], call[3])]
    return td._oracle_planes(ora, coef, call, zs)


def deriv_shape(call):
    return (1 if call[0] == "gs" and call[8] is not None else call[6] - call[5]), call[4], call[3]


class Host:
    """libwnoise_host.so's scalar evaluators over point lists (the exact kernels' bits), called with raw addresses."""

    def __init__(self):
        path = os.path.join(PKG, "libwnoise_host.so")
        if not os.path.exists(path):
            import __graft_entry__
            __graft_entry__.build()
        lib = C.CDLL(path)
        V, I = C.c_void_p, C.c_int
        self.e3, self.g3, self.c3 = lib.wnhost_eval3d, lib.wnhost_eval3d_grad, lib.wnhost_eval3d_curl
        self.e3.restype, self.e3.argtypes = C.c_float, [V, I, V]
        self.g3.restype, self.g3.argtypes = C.c_float, [V, I, V, V]
        self.c3.restype, self.c3.argtypes = None, [V, I, V, V, V]
        self.tex = lib.wnhost_wavelet_texture_value
        self.tex.restype, self.tex.argtypes = C.c_float, [V, I, I, C.c_double, I, V]
        self.lib = lib

    def texture(self, coef, pts):
        """wavelet_texture(scale 1, octave 4, 3-D) at every point."""
        coef, n = self._tile(coef)
        pts = np.ascontiguousarray(pts, f32)
        fn, cp, base = self.tex, coef.ctypes.data, pts.ctypes.data
        return np.array([fn(cp, n, 1, 1.0, 4, base + 12 * i) for i in range(len(pts))], f32)

    @staticmethod
    def _tile(coef):
        coef = np.ascontiguousarray(coef, f32)
        n = int(round(coef.size ** (1.0 / 3.0)))
        assert n ** 3 == coef.size
        return coef, n

    def eval3d(self, coef, pts):
        coef, n = self._tile(coef)
        pts = np.ascontiguousarray(pts, f32)
        fn, cp, base = self.e3, coef.ctypes.data, pts.ctypes.data
        return np.array([fn(cp, n, base + 12 * i) for i in range(len(pts))], f32)

    def grad(self, coef, pts):
        coef, n = self._tile(coef)
        pts = np.ascontiguousarray(pts, f32)
        out = np.empty((len(pts), 4), f32)
        fn, cp, base, ob = self.g3, coef.ctypes.data, pts.ctypes.data, out.ctypes.data
        out[:, 0] = [fn(cp, n, base + 12 * i, ob + 16 * i + 4) for i in range(len(pts))]
        return out

    def curl(self, coef, pts, offsets):
        coef, n = self._tile(coef)
        pts = np.ascontiguousarray(pts, f32)
        off = np.ascontiguousarray(np.asarray(offsets, np.int32).reshape(9))
        out = np.empty((len(pts), 3), f32)
        fn, cp, base, ob, op = self.c3, coef.ctypes.data, pts.ctypes.data, out.ctypes.data, off.ctypes.data
        for i in range(len(pts)):
            fn(cp, n, base + 12 * i, op, ob + 12 * i)
        return out


@pytest.fixture(scope="module")
def host():
    return Host()


def band_points(pts, first, b):
    """WMultibandNoise's coordinate of band b: (2 * p) * 2^(first + b), both products exact."""
    return (f32(2) * pts) * f32(2.0 ** (first + b))


def host_value(host, coef, call):
    """The call by the host's exact evaluator: one band in the exact kernel's own arithmetic (float32 result times the
    float32 scale), several bands composed in float64 from the float32 band values."""
    pts = lattice_points(*value_coords(call))
    if call[0] in ("v", "vz"):
        return (host.eval3d(coef, pts) * INV32).astype(np.float64).reshape(value_shape(call))
    s, first, nb, w = call[-4:]
    out = np.zeros(len(pts))
    for b in range(fp.active_bands(s, first, nb)):
        out += float(f32(w[b])) * host.eval3d(coef, band_points(pts, first, b)).astype(np.float64)
    return (out / _ref64_grad.out_div(w, nb, 0.18402)).reshape(value_shape(call))


def host_deriv(host, coef, call, family):
    """[4 or 3, nz, ny, nx] float64 by the host's evaluators (gradient records; curl with the offsets tc.MIXED)."""
    pts = lattice_points(*tg.call_coords(call))
    ev = host.grad if family == "grad" else (lambda c, p: host.curl(c, p, tc.MIXED))
    if call[0] in ("g", "gs"):
        out = (ev(coef, pts) * f32(tg.INV)).astype(np.float64)
    else:
        s, first, nb, w = call[-4:]
        out = np.zeros((len(pts), 4 if family == "grad" else 3))
        for b in range(fp.active_bands(s, first, nb)):
            e = ev(coef, band_points(pts, first, b)).astype(np.float64) * float(f32(w[b]))
            if family == "grad":
                e[:, 1:] *= 2.0 * 2.0 ** (first + b)
            else:
                e *= 2.0 * 2.0 ** (first + b)
            out += e
        out /= _ref64_grad.out_div(w, nb, 0.18402)
    return np.ascontiguousarray(out.T).reshape((out.shape[1],) + deriv_shape(call))


# Bounds against the float64 reference: the near rows' tolerances, unchanged.  VALUE_BOUND / DERIV_BOUND would name the rows
# whose bound comes from the host evaluator's measured error instead (twice that error); the CPU precondition below finds
# none: exact evaluation alone stays inside the near bounds at every far row.
VALUE_BOUND = {}
DERIV_BOUND = {}


def value_bound(name):
    return VALUE_BOUND.get(name, td.REF64_TOL)


def deriv_bound(name, call, family):
    return DERIV_BOUND.get((family, name), tg.call_tol(call) if family == "grad" else tc.call_tol(call))


# ---- CPU precondition: exact evaluation alone stays inside the bounds ---------------------------------------------------------
@pytest.fixture(scope="module")
def cpu_coefs(ora, gold):
    return {"t128": ora.tile3d(128, 12345), "t32": ora.tile3d(32, td.SEED32), "t8": gold["tile3d_8_7"],
            "t16": gold["tile3d_16_12345"], "t6": gold["tile3d_5odd_11"]}


@pytest.mark.parametrize("name,call", [pytest.param(n, c, id=n) for n, c, _, _ in FAR_VALUE])
def test_host_evaluator_within_the_value_bound(host, cpu_coefs, name, call):
    coef = cpu_coefs[call[1]]
    err = float(np.abs(host_value(host, coef, call) - ref64_value(coef, call)).max())
    print(f"{name}: |host - ref64| {err:.3e} (bound {value_bound(name):.1e})")
    assert err <= td.REF64_TOL or name in VALUE_BOUND, (name, err)
    if name in VALUE_BOUND:
        assert VALUE_BOUND[name] >= 2.0 * err > 2.0 * td.REF64_TOL, (name, err)


@pytest.mark.parametrize("family", ["grad", "curl"])
@pytest.mark.parametrize("name,call", [pytest.param(n, c, id=n) for n, c, _, _ in FAR_DERIV])
def test_host_evaluator_within_the_derivative_bound(host, cpu_coefs, family, name, call):
    coef = cpu_coefs[call[1]]
    ref = tg.ref64_call(coef, call) if family == "grad" else tc.ref64_call(coef, call)
    got = host_deriv(host, coef, call, family)
    assert got.shape == ref.shape
    err = np.abs(got - ref).reshape(ref.shape[0], -1).max(1)
    near = tg.call_tol(call) if family == "grad" else tc.call_tol(call)
    print(f"{family} {name}: |host - ref64| per channel {err} (bound {deriv_bound(name, call, family):.3e})")
    assert (err <= near).all() or (family, name) in DERIV_BOUND, (family, name, err, near)
    if (family, name) in DERIV_BOUND:
        assert DERIV_BOUND[(family, name)] >= 2.0 * err.max() > 2.0 * near


# ---- GPU -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wn():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU (the product has no CPU path)"
    return importlib.import_module("wavelet-noise-in-ray-tracing_amd")


@pytest.fixture(scope="module")
def tiles(wn):
    return td.load_tiles(wn)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(got, want, what):
    bad = np.flatnonzero(bits(got).ravel() != bits(want).ravel())
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} elements differ, first at {int(bad[0])}"


def run_value_call(wn, objs, call, exact, out=None):
    """td.run_call, and the "vz" kind: wn_eval3d_grid on wavelet_volume's lattice with WN_Z_CONST."""
    if call[0] != "vz":
        return td.run_call(wn, objs, call, exact, out=out)
    import torch
    nm = importlib.import_module("wavelet-noise-in-ray-tracing_amd.noise")
    den, nx, ny, zc, octave = call[2:]
    g = wn.GridSpec(den, nx, ny, octave_scale=float(2.0 ** octave), post_scale=2.0, out_scale=float(INV32),
                    z_mode=nm.WN_Z_CONST, z_const=zc, flags=nm.WN_GRID_EXACT if exact else nm.WN_GRID_DEFAULT)
    out = g.empty(out)
    gc = g.c()
    nm.check(nm._lib.wn_eval3d_grid(objs[call[1]]._handle(3), C.byref(gc), nm._ptr(out), nm._stream()))
    torch.cuda.current_stream().synchronize()
    return out[: ny * nx].view(1, ny, nx)


def framed_value(wn, objs, call, exact, lead, what):
    nz, ny, nx = value_shape(call)
    f = Frame(nz * ny * nx, lead, back_extra=16 * ny * nx)
    run_value_call(wn, objs, call, exact, out=f.tensor)
    return f.result(what=what).reshape(nz, ny, nx)


def framed_deriv(wn, family, objs, call, exact, lead, what):
    mod, ch = (tg, 4) if family == "grad" else (tc, 3)
    nz, ny, nx = deriv_shape(call)
    f = Frame(ch * nz * ny * nx, lead, back_extra=16 * ny * nx)
    mod.run_call(wn, objs, call, exact=exact, out=f.tensor)
    return f.result(what=what).reshape(ch, nz, ny, nx)


def _child():
    import torch
    assert torch.cuda.is_available()
    wn = importlib.import_module("wavelet-noise-in-ray-tracing_amd")
    objs, _ = td.load_tiles(wn)
    torch.cuda.synchronize()
    for _name, call, _kernel, _e in FAR_VALUE + STRIP_CHUNK:
        run_value_call(wn, objs, call, False)
        torch.cuda.synchronize()
    for mod, rows in ((tg, FAR_DERIV), (tc, FAR_CURL)):
        for _name, call, _kernel, _e in rows:
            mod.run_call(wn, objs, call)
            torch.cuda.synchronize()
    print(f"far lattice child: {len(FAR_VALUE) + len(STRIP_CHUNK) + len(FAR_DERIV) + len(FAR_CURL)} calls")


def kernel_label(name):
    for mod in (td, tg, tc):
        lab = mod.kernel_label(name)
        if lab is not None and not lab.split("<")[0].endswith("points_kernel"):
            return lab
    return None


@pytest.mark.gpu
def test_far_routes_reach_the_kernels_they_name(tmp_path):
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    assert os.path.exists(prof), "rocprofv3 is needed to observe which kernel ran"
    out_dir = tmp_path / "trace"
    cmd = ["timeout", "-k", "10", "300", prof, "--kernel-trace", "--output-format", "csv", "-d", str(out_dir),
           "--", sys.executable, os.path.abspath(__file__), "--child"]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
    assert res.returncode == 0, f"exit {res.returncode}\n{res.stdout[-3000:]}\n{res.stderr[-3000:]}"
    files = glob.glob(str(out_dir / "**" / "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, (files, res.stdout[-2000:])
    with open(files[0], newline="") as f:
        rows = list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    got = [lab for lab in (kernel_label(r["Kernel_Name"]) for r in rows) if lab is not None]
    want = [(n, k) for n, _, k, _ in FAR_VALUE + STRIP_CHUNK] + [("grad " + n, k) for n, _, k, _ in FAR_DERIV] + \
           [("curl " + n, k) for n, _, k, _ in FAR_CURL]
    assert len(got) == len(want), (len(got), len(want), got)
    wrong = [(name, k, g) for (name, k), g in zip(want, got) if k != g]
    assert not wrong, "lattices served by another kernel than the table names (case, expected, ran): " + repr(wrong)


@pytest.mark.gpu
@pytest.mark.parametrize("name,call,kernel", [pytest.param(n, c, k, id=n) for n, c, k, _ in FAR_VALUE])
def test_far_value_rows(wn, ora, tiles, name, call, kernel):
    """Both tiers into sentinel-filled frames at leads 0 and 1 (a misaligned output sends the plane pipeline's and the strip
    kernel's lattices to the brick kernel: the same bounds hold).  Default tier within td.TOL of WN_GRID_EXACT; both within
    the row's bound of the float64 reference at the float32 coordinates; WN_GRID_EXACT bit for bit with the oracle on the
    first and last planes, and at lead 1 with lead 0; an exact kernel's default tier has WN_GRID_EXACT's bits."""
    objs, coefs = tiles
    coef = coefs[call[1]]
    ref = ref64_value(coef, call)
    exact = {k: framed_value(wn, objs, call, True, k, f"{name} exact") for k in (0, 1)}
    fast = {k: framed_value(wn, objs, call, False, k, name) for k in (0, 1)}
    assert ref.shape == exact[0].shape == fast[0].shape
    same_bits(exact[1], exact[0], f"{name}: WN_GRID_EXACT at lead 1 against lead 0")
    e64 = exact[0].astype(np.float64)
    e_er = float(np.abs(e64 - ref).max())
    figures = [f"|exact-ref64| {e_er:.3g}"]
    for k in (0, 1):
        assert np.isfinite(fast[k]).all()
        e_fe, e_fr = float(np.abs(fast[k] - e64).max()), float(np.abs(fast[k] - ref).max())
        figures.append(f"lead {k}: |fast-exact| {e_fe:.3g} |fast-ref64| {e_fr:.3g}")
    print(f"{name} ({kernel}): " + "; ".join(figures))
    assert e_er <= value_bound(name), (name, e_er)
    for k in (0, 1):
        assert float(np.abs(fast[k] - e64).max()) <= td.TOL, (name, kernel, k)
        assert float(np.abs(fast[k] - ref).max()) <= value_bound(name), (name, kernel, k)
    if kernel in (EXACT_LDS, DIRECT):
        for k in (0, 1):
            same_bits(fast[k], exact[0], f"{name}: an exact kernel's default tier at lead {k} against WN_GRID_EXACT")
    zs = sorted({0, ref.shape[0] - 1})
    for z, want in zip(zs, oracle_value_planes(ora, coef, call, zs)):
        same_bits(exact[0][z], want, f"{name}: WN_GRID_EXACT against the oracle on plane {z}")


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["grad", "curl"])
@pytest.mark.parametrize("name,call,kernel", [pytest.param(n, c, k, id=n) for n, c, k, _ in FAR_DERIV])
def test_far_derivative_rows(wn, tiles, host, family, name, call, kernel):
    """Both tiers, frames at leads 0 and 1 (brick_plan takes no account of the pointer: the bits of lead 0); every channel of
    both tiers within the row's bound of the float64 reference and of each other; WN_GRID_EXACT has the bits of the point
    entry point at the lattice's float32 coordinates and, for one band, of the host evaluator (record times the float32
    out_scale)."""
    import torch
    objs, coefs = tiles
    coef = coefs[call[1]]
    mod = tg if family == "grad" else tc
    kernel = kernel.replace("grad3d_", family + "3d_")
    ref = mod.ref64_call(coef, call)
    tol = deriv_bound(name, call, family)
    got = {}
    for exact in (False, True):
        tier = "exact" if exact else "default"
        r = {k: framed_deriv(wn, family, objs, call, exact, k, f"{family} {name} {tier}") for k in (0, 1)}
        same_bits(r[1], r[0], f"{family} {name} {tier}: lead 1 against lead 0")
        got[exact] = r[0].astype(np.float64)
        assert got[exact].shape == ref.shape
    e_fe = np.abs(got[False] - got[True]).reshape(ref.shape[0], -1).max(1)
    e_fr = np.abs(got[False] - ref).reshape(ref.shape[0], -1).max(1)
    e_er = np.abs(got[True] - ref).reshape(ref.shape[0], -1).max(1)
    print(f"{family} {name} ({kernel}): |fast-exact| {e_fe.max():.3g} |fast-ref64| {e_fr.max():.3g} |exact-ref64| {e_er.max():.3g} "
          f"tol {tol:.3g}")
    assert (e_er <= tol).all(), (family, name, e_er, tol)
    assert (e_fe <= tol).all() and (e_fr <= tol).all(), (family, name, kernel, e_fe, e_fr, tol)
    td_ = torch.from_numpy(lattice_points(*tg.call_coords(call))).cuda()
    tile = objs[call[1]]
    if call[0] in ("g", "gs"):
        pk = tile.evaluate3DGradient(td_) if family == "grad" else tile.evaluate3DCurl(td_, tc.MIXED)
        pk = pk.cpu().numpy() * f32(tg.INV)
    else:
        s, first, nb, w = call[-4:]
        pk = tile.WMultibandNoiseGradient(td_, s, first, nb, w) if family == "grad" else \
            tile.WMultibandNoiseCurl(td_, s, first, nb, w, offsets=tc.MIXED)
        pk = pk.cpu().numpy()
    same_bits(got[True].astype(f32).reshape(ref.shape[0], -1).T, pk, f"{family} {name}: WN_GRID_EXACT against the point kernel")
    if call[0] in ("g", "gs"):
        pts = lattice_points(*tg.call_coords(call))
        rec = host.grad(coef, pts) if family == "grad" else host.curl(coef, pts, tc.MIXED)
        same_bits(got[True].astype(f32).reshape(ref.shape[0], -1).T, rec * f32(tg.INV),
                  f"{family} {name}: WN_GRID_EXACT against the host evaluator")


PERIODIC = [(n, c, k, "value") for n, c, k, _ in FAR_VALUE if n.endswith("_pow2")] + \
           [(n, c, k, f) for f, rows in (("grad", FAR_DERIV), ("curl", FAR_CURL)) for n, c, k, _ in rows if n.endswith("_pow2")]


def test_periodic_rows_are_whole_tile_periods_out():
    """z0 = 3 + k * P with P = 128 / (the lowest band's step) planes and k * P about 1e6 planes; den a power of two; the
    same kernel serves the planes next to the origin."""
    assert len(PERIODIC) == len(VALUE_FAMILIES) + 2 * len(DERIV_FAMILIES)
    for name, call, kernel, family in PERIODIC:
        assert call[1] == "t128" and call[2] & (call[2] - 1) == 0, name
        g, bands = value_grid(call) if family == "value" else deriv_grid(call)
        low = (8.0 * 2.0 ** call[-1] if bands is None else 8.0 * 2.0 ** bands[1]) / g.den
        period = 128.0 / low
        assert period == int(period) and (call[5] - 3) % int(period) == 0 and 0.98e6 <= call[5] - 3 <= 1.0e6, (name, period)
        near = moved(call, 3)
        route = value_route(near) if family == "value" else deriv_route(near, family)
        assert route[0] == kernel, (name, route)


@pytest.mark.gpu
@pytest.mark.parametrize("name,call,kernel,family", [pytest.param(*r, id=f"{r[3]}_{r[0]}") for r in PERIODIC])
def test_far_planes_repeat_the_near_ones(wn, tiles, name, call, kernel, family):
    """Planes z and z + k * P (about 1e6 planes out, whole periods of the 128 tile in every band; power-of-two den: the
    coordinates are exact) have the same bits, in both tiers, whichever kernel serves them."""
    objs, _ = tiles
    for exact in (False, True):
        if family == "value":
            far, near = (run_value_call(wn, objs, c, exact).cpu().numpy() for c in (call, moved(call, 3)))
        else:
            mod = tg if family == "grad" else tc
            far, near = (mod.run_call(wn, objs, c, exact=exact).cpu().numpy() for c in (call, moved(call, 3)))
        same_bits(far, near, f"{family} {name} ({kernel}, {'exact' if exact else 'default'} tier): planes from {call[5]} against 3")


@pytest.mark.gpu
def test_strip_chunk_max_edge(wn, ora, tiles):
    """The two STRIP_CHUNK lattices (113 planes of 256 x 2045 samples; by strip_try's arithmetic, restated in
    _far_plan.strip_items, walked as one item and as two -- derived, not observed: the item length is a kernel argument
    that neither the trace nor the output shows, so only the values tell whether either split is right): the default tier
    within td.TOL of WN_GRID_EXACT on the whole lattice (compared on the device), every element written and nothing beyond
    (sentinel prefill, checked on the device), first and last planes against the float64 reference and the oracle."""
    import torch
    from _frame import SENTINEL_BITS
    objs, coefs = tiles
    assert wn.device_info()["compute_units"] == CUS, "STRIP_CHUNK is derived for 256 compute units"
    sentinel = int(np.uint32(SENTINEL_BITS).view(np.int32))
    for name, call, kernel, chunk_len in STRIP_CHUNK:
        nz, ny, nx = value_shape(call)
        count, guard = nz * ny * nx, 4096
        res = {}
        for exact in (False, True):
            buf = torch.empty(count + 2 * guard, dtype=torch.float32, device="cuda")
            buf.view(torch.int32).fill_(sentinel)
            assert (buf.data_ptr() + 4 * guard) % 16 == 0
            run_value_call(wn, objs, call, exact, out=buf[guard:guard + count])
            torch.cuda.synchronize()
            words = buf.view(torch.int32)
            assert bool((words[:guard] == sentinel).all()) and bool((words[guard + count:] == sentinel).all()), name
            assert not bool((words[guard:guard + count] == sentinel).any()), name
            res[exact] = buf[guard:guard + count].view(nz, ny, nx)
        e_fe = float((res[False] - res[True]).abs().max())
        print(f"{name} (items of {chunk_len} planes): |fast-exact| {e_fe:.3g}")
        assert e_fe <= td.TOL, (name, e_fe)
        zs = (0, nz - 1)
        for z, want in zip(zs, oracle_value_planes(ora, coefs[call[1]], call, zs)):
            ref = ref64_value(coefs[call[1]], moved(call, call[5] + z)[:6] + (call[5] + z + 1,) + call[7:])[0]
            same_bits(res[True][z].cpu().numpy(), want, f"{name}: WN_GRID_EXACT against the oracle on plane {z}")
            e_fr = float(np.abs(res[False][z].cpu().numpy().astype(np.float64) - ref).max())
            assert e_fr <= td.REF64_TOL, (name, z, e_fr)
        del res, buf
        torch.cuda.empty_cache()


# ======== point lists far out and collapsed =====================================================================================
# wnoise.h defines results for |coordinate| < 2^31; every coordinate here (the finest band's or octave's included) stays at or
# below 2^30.  (a) magnitudes spread exponentially over 2^10 .. 2^cap in both signs; (b) the binade edges +-2^23 and +-2^24,
# where p - 0.5f rounds and t is 0 or 0.5; (c) lists of N_LONG points collapsed onto one point, or onto runs of identical
# points (a far plane seen through neighbouring pixels: x advances by less than one float32 ulp per sample).
N_LONG = 16 * 4096 + 4096 + 1000      # one chunk and a ragged tail beyond kSortMinPoints
N_SLAB = tp.SLAB_MIN + 4096 + 1000    # ... beyond kSlabMinPoints: plane_sorted_points_kernel<Ops, true> + row_slab_points_kernel
MB = (-16.0, -2, 5, W5)               # WMultibandNoise: finest coordinate 2 * p * 2^(first + nb - 1) = 8 p
MB_CAP = 27                           # 8 * 2^27 = 2^30
TEX_CAP = 25                          # the texture coordinate is 32 p
TURB_DEPTH, TURB_CAP = 7, 24          # octaves p * 2^0 .. p * 2^6
FRACTAL_CAP = 25                      # fractal_noise: six octaves p * 2^0 .. p * 2^5
FOOT = (0, 5)                         # footprint lists: first band, bands; finest coordinate 2 * p * 2^4
FOOT_CAP = 25


def magnitude_points(n, cap, seed, finest=1.0):
    """(n, 3) float32 with |coordinate| = 2^e, e uniform over [10, cap], both signs; the first rows hold +-2^cap and +-2^10
    themselves.  `finest`: the factor of the finest band or octave of the call the list is for."""
    rng = np.random.default_rng(seed)
    p = (rng.choice([-1.0, 1.0], (n, 3)) * 2.0 ** rng.uniform(10.0, cap, (n, 3))).astype(f32)
    p = np.clip(p, -f32(2.0 ** cap), f32(2.0 ** cap))
    p[0], p[1], p[2], p[3] = 2.0 ** cap, -2.0 ** cap, 2.0 ** 10, -2.0 ** 10
    p[4] = (2.0 ** cap, -2.0 ** 10, 2.0 ** ((cap + 10) // 2))
    assert np.isfinite(p).all() and float(np.abs(p).max()) * finest <= 2.0 ** 30
    assert float(np.abs(p).min()) >= 2.0 ** 10 and (p > 0).any() and (p < 0).any()
    return np.ascontiguousarray(p)


def binade_values():
    vals = []
    for k in (23, 24):
        for sgn in (-1.0, 1.0):
            v = f32(sgn * 2.0 ** k)
            below = above = v
            vals.append(v)
            for _ in range(3):
                below, above = np.nextafter(below, f32(0.0)), np.nextafter(above, f32(sgn * np.inf))
                vals += [below, above]
    return np.array(vals, f32)


def binade_points(scale=1.0, seed=3):
    """Every binade value on each axis in turn beside two far coordinates, and on all three axes at once; times `scale` (a
    power of two: a band's coordinate 2 * p * 2^(first + b) then lands on the binade edge)."""
    v = binade_values()
    rng = np.random.default_rng(seed)
    rows = []
    for axis in range(3):
        p = (rng.choice([-1.0, 1.0], (len(v), 3)) * 2.0 ** rng.uniform(10.0, 22.0, (len(v), 3))).astype(f32)
        p[:, axis] = v
        rows.append(p)
    rows.append(np.stack([v, np.roll(v, 5), np.roll(v, 11)], 1))
    p = np.concatenate(rows) * f32(scale)
    assert float(np.abs(p).max()) <= 2.0 ** 25 * scale
    return np.ascontiguousarray(p, f32)


def test_binade_points_sit_where_the_subtraction_rounds():
    v = binade_values()
    assert len(v) == 28 and len(np.unique(v)) == 28
    pm = v - f32(0.5)
    t = np.ceil(pm) - pm
    assert set(np.unique(t)) == {0.0, 0.5}                       # no other fraction survives at these magnitudes
    big = np.abs(v) >= 2.0 ** 24
    assert ((v.astype(np.float64) - 0.5)[big] != pm[big]).all()  # p - 0.5f rounded
    assert (t[big] == 0.0).all()


def collapsed(kind, n):
    """`alt`: the stream below with z alternating between two far planes -- the only collapsed list whose chunks
    plane_sorted_points_kernel<Ops, true> defers to the row-slab kernel (test_which_collapsed_chunks_reach_the_slab_kernel).
    `one`: a single far point repeated.  `stream`: x advances by 0.002 per sample at 2^26 (ulp 8: runs of 4000 identical
    samples), z by 0.0001 at -2^25 (ulp 4), y is the row 77 (mod 128) far out: a coherent far-plane stream."""
    if kind == "one":
        return np.ascontiguousarray(np.broadcast_to(f32([2.0 ** 26 + 40.0, -3.0e6 + 0.25, 1.5e7 + 3.0]), (n, 3)))
    i = np.arange(n, dtype=np.float64)
    p = np.stack([2.0 ** 26 + 0.002 * i, np.full(n, 128.0 * 9000 + 77.0), -2.0 ** 25 + 0.0001 * i], 1).astype(f32)
    if kind == "alt":    # ... seen through two surfaces in turn: z jumps by 40 cells between neighbours (ulp 4 at 2^25)
        p[:, 2] = f32(-2.0 ** 25) + f32(40.0) * (np.arange(n) % 2).astype(f32)
    return np.ascontiguousarray(p)


def runs_of(pts):
    """(starts, lengths) of the runs of identical consecutive points."""
    change = np.flatnonzero((pts[1:] != pts[:-1]).any(1)) + 1
    starts = np.concatenate([[0], change])
    return starts, np.diff(np.concatenate([starts, [len(pts)]]))


def test_which_collapsed_chunks_reach_the_slab_kernel():
    """tp.defer_model on the collapsed lists: `one` and `stream` are coherent chunks, which the first kernel of the row-slab
    pair evaluates itself (those rows exercise the pair's route and the first kernel, not row_slab_points_kernel's
    arithmetic); every full chunk of `alt` is deferred, for evaluate3D and for the texture."""
    n = 8 * tp.CHUNK + 1000
    for kind, want in (("one", 0), ("stream", 0), ("alt", 8)):
        cells = collapsed(kind, n)
        assert int(tp.defer_model(tp.mid_of(cells), n).sum()) == want, kind
        assert int(tp.defer_model(tp.texture_mids(tp.to_texture(cells)), n).sum()) == want, kind
    alt = collapsed("alt", n)
    assert len(runs_of(alt[0::2])[0]) <= 20 and len(runs_of(alt[1::2])[0]) <= 20      # each half stays collapsed
    assert (alt[0:n - 1:2, 2] != alt[1::2, 2]).all()


def test_collapsed_lists_are_collapsed():
    assert N_LONG == tp.SORT_MIN + tp.CHUNK + 1000
    starts, lengths = runs_of(collapsed("one", N_LONG))
    assert len(starts) == 1
    starts, lengths = runs_of(collapsed("stream", N_LONG))
    assert 15 <= len(starts) <= 40 and lengths.max() >= 2000
    assert float(np.abs(collapsed("stream", 10)).max()) * 8 <= 2.0 ** 30      # WMultibandNoise's finest band


# (name, entry, tile, list, n, extra, kernels of the call): tp.POINT_ROUTES' row format; tp.run_row runs a row, tp.row_reference
# is the oracle's answer.  `list` names the generator.  Lists of N_LONG points take the plane-ordered kernels, their slices
# and the short lists the plain ones, N_SLAB the pair with the row-slab kernel (unmasked, tile 128).
FAR_POINT_ROUTES = [
    ("e3_magnitude", "e3", "t128", ("magnitude", 30, 1.0), 3000, None, (tp.EV3(True),)),
    ("e3_binade", "e3", "t128", ("binade", 1.0), 112, None, (tp.EV3(True),)),
    ("e3_t6_magnitude", "e3", "t6", ("magnitude", 30, 1.0), 3000, None, (tp.EV3(True),)),
    ("mb_magnitude", "mb", "t128", ("magnitude", MB_CAP, 8.0), 3000, MB, (tp.MB3(True),)),
    ("mb_binade_top", "mb", "t128", ("binade", 1.0 / 8.0), 112, MB, (tp.MB3(True),)),
    ("mb_binade_low", "mb", "t128", ("binade", 2.0), 112, MB, (tp.MB3(True),)),
    ("proj_magnitude", "proj", "t128", ("magnitude", 30, 1.0), 2000, None, (tp.PROJ_PTS,)),
    ("proj_binade", "proj", "t128", ("binade", 1.0), 112, None, (tp.PROJ_PTS,)),
    ("mbproj_magnitude", "mbproj", "t128", ("magnitude", 28, 4.0), 2000, (-16.0, -1, 3, [1.0, 0.5, 2.0]), (tp.MB_PROJ,)),
    ("tex_magnitude", "tex", "t128", ("magnitude", TEX_CAP, 32.0), 3000, (True, False), (tp.TEXK(False, True),)),
    ("tex_binade", "tex", "t128", ("binade", 1.0 / 32.0), 112, (True, True), (tp.TEXK(True, True),)),
    ("e3_one", "e3", "t128", ("one",), N_LONG, None, (tp.SORTED(tp.EV_OPS(True, False)),)),
    ("e3_stream", "e3", "t128", ("stream",), N_LONG, None, (tp.SORTED(tp.EV_OPS(True, False)),)),
    ("mb_one", "mb", "t128", ("one",), N_LONG, MB, (tp.SORTED(tp.EV_OPS(True, True)),)),
    ("mb_stream", "mb", "t128", ("stream",), N_LONG, MB, (tp.SORTED(tp.EV_OPS(True, True)),)),
    ("tex_one", "tex", "t128", ("one",), N_LONG, (True, False), (tp.SORTED(tp.TEX_OPS(False, True)),)),
    ("tex_stream", "tex", "t128", ("stream",), N_LONG, (True, False), (tp.SORTED(tp.TEX_OPS(False, True)),)),
    ("tex_stream_masked", "tex", "t128", ("stream",), N_LONG, (True, True), (tp.SORTED(tp.TEX_OPS(True, True)),)),
    ("e3_alt_slab", "e3", "t128", ("alt",), N_SLAB, None, tp.PAIR(tp.EV_OPS(True, False))),
    ("tex_alt_slab", "tex", "t128", ("alt",), N_SLAB, (True, False), tp.PAIR(tp.TEX_OPS(False, True))),
    ("e3_stream_slab", "e3", "t128", ("stream",), N_SLAB, None, tp.PAIR(tp.EV_OPS(True, False))),
    ("tex_stream_slab", "tex", "t128", ("stream",), N_SLAB, (True, False), tp.PAIR(tp.TEX_OPS(False, True))),
]


def far_row_inputs(row):
    """The row's points as the entry point takes them, and the active mask of the masked texture rows."""
    name, entry, tile, spec, n, extra = row[:6]
    if spec[0] == "magnitude":
        cells = magnitude_points(n, spec[1], len(name), spec[2])
    elif spec[0] == "binade":
        cells = binade_points(spec[1])
        assert len(cells) == n
    else:
        cells = collapsed(spec[0], n)
    if entry == "tex":
        pts = tp.to_texture(cells) if spec[0] in ("one", "stream", "alt") else cells   # (the other lists are made for 32 p)
        assert float(np.abs(pts).max()) * 32.0 <= 2.0 ** 30
    else:
        pts = cells
    active = None
    if entry == "tex" and extra[1]:
        active = (np.random.default_rng(n).uniform(size=n) < 0.6).astype(np.uint8)
        if n > 5 * tp.CHUNK:
            active[: 3 * tp.CHUNK] = 1
            active[3 * tp.CHUNK: 5 * tp.CHUNK] = 0
    return np.ascontiguousarray(pts, f32), active


def test_far_point_rows_stay_inside_the_domain():
    for row in FAR_POINT_ROUTES:
        if row[4] > N_LONG:
            continue
        pts, _ = far_row_inputs(row)
        entry, extra = row[1], row[5]
        finest = {"e3": 1.0, "proj": 1.0, "tex": 32.0}.get(entry) or 2.0 * 2.0 ** (extra[1] + extra[2] - 1)
        assert float(np.abs(pts).max()) * finest <= 2.0 ** 30, row[0]
        assert np.isfinite(pts).all()


def _points_child():
    import torch
    assert torch.cuda.is_available()
    ctx = tp.Ctx(importlib.import_module("wavelet-noise-in-ray-tracing_amd"))
    torch.cuda.synchronize()
    for row in FAR_POINT_ROUTES:
        pts, active = far_row_inputs(row)
        tp.run_row(ctx, row, pts, active)
        torch.cuda.synchronize()
    print(f"far point child: {len(FAR_POINT_ROUTES)} calls")


@pytest.fixture(scope="module")
def ctx(wn):
    return tp.Ctx(wn)


@pytest.mark.gpu
def test_far_point_routes_reach_the_kernels_they_name(tmp_path):
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    assert os.path.exists(prof), "rocprofv3 is needed to observe which kernel ran"
    out_dir = tmp_path / "trace"
    cmd = ["timeout", "-k", "10", "300", prof, "--kernel-trace", "--output-format", "csv", "-d", str(out_dir),
           "--", sys.executable, os.path.abspath(__file__), "--child-points"]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
    assert res.returncode == 0, f"exit {res.returncode}\n{res.stdout[-3000:]}\n{res.stderr[-3000:]}"
    files = glob.glob(str(out_dir / "**" / "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, (files, res.stdout[-2000:])
    with open(files[0], newline="") as f:
        rows = list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    got = [lab for lab in (tp.kernel_label(r["Kernel_Name"]) for r in rows) if lab is not None]
    wrong, pos = [], 0
    for r in FAR_POINT_ROUTES:
        ran = tuple(got[pos:pos + len(r[6])])
        if ran != tuple(r[6]):
            wrong.append((r[0], r[6], ran))
        pos += len(r[6])
    assert pos == len(got) and not wrong, \
        f"{len(got)} kernels traced, {pos} expected; calls served otherwise (case, expected, ran): {wrong!r}"


def multiband_points_ref64(coef, pts, s, first, nb, w, var_per_band):
    """_ref64.multiband_points' sum (band b: w_b * evaluate3D((2 p) * 2^(first + b)) over the bands `s` lets run, divided by
    sqrt(sum w^2 * var_per_band)), vectorised over the list."""
    out = np.zeros(len(pts))
    for b in range(fp.active_bands(s, first, nb)):
        out += float(f32(w[b])) * _ref64.evaluate3d_points(coef, band_points(pts, first, b))
    return out / _ref64_grad.out_div(w, nb, var_per_band)


def _expand(pts, fn):
    """fn on the first point of every run of identical points, repeated over the run (a list that alternates between two
    such streams: each half on its own)."""
    starts, lengths = runs_of(pts)
    if len(starts) > 100000 and len(starts) > len(pts) // 2:
        even, odd = _expand(pts[0::2], fn), _expand(pts[1::2], fn)
        out = np.empty((len(pts),) + even.shape[1:], even.dtype)
        out[0::2], out[1::2] = even, odd
        return out
    return np.repeat(fn(np.ascontiguousarray(pts[starts])), lengths, axis=0)


@pytest.mark.gpu
@pytest.mark.parametrize("row", FAR_POINT_ROUTES, ids=[r[0] for r in FAR_POINT_ROUTES])
def test_far_point_route_values(ctx, host, row):
    """Every element against the oracle, bit for bit (masked rows: inactive elements keep the sentinel); evaluate3D rows also
    against the host evaluator's bits and the float64 reference (td.REF64_TOL), WMultibandNoise rows against the float64
    reference, the projected rows within _ref64's per-point bound; lists of N_LONG points and more against their slices of
    SORT_MIN / 2 + 5 points (the plain kernels), bit for bit."""
    import torch
    name, entry, tile, spec, n, extra = row[:6]
    pts, active = far_row_inputs(row)
    got = tp.run_row(ctx, row, pts, active)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    if entry in ("proj", "mbproj"):       # tp's normals are drawn per list length: no run-length shortcut
        want = tp.row_reference(ctx, row, pts, active)
    else:
        want = _expand(pts, lambda p: tp.row_reference(ctx, row[:4] + (len(p),) + row[5:], p, None))
    if active is not None:
        want = np.where(active != 0, want, np.uint32(tp.SENTINEL_BITS).view(f32))
    count, first = tp._first_differences(got, want)
    assert count == 0, f"{name}: {count} elements differ from the oracle, first (index, got, want): {first}"
    coef = ctx.coef[tile]
    on = slice(None) if active is None else active != 0
    if entry == "e3":
        same_bits(got, _expand(pts, lambda p: host.eval3d(coef, p)), f"{name}: against the host evaluator")
        err = float(np.abs(got - _expand(pts, lambda p: _ref64.evaluate3d_points(coef, p))).max())
        assert err <= td.REF64_TOL, (name, err)
    elif entry == "mb":
        ref = _expand(pts, lambda p: multiband_points_ref64(coef, p, *extra, 0.18402))
        err = float(np.abs(got - ref).max())
        assert err <= td.REF64_TOL, (name, err)
    elif entry == "tex":
        # the host evaluator's bits, and the float64 reference: grey = 0.5 * (1 + clamp(noise / 4)), noise = evaluate3D(32 p)
        # / sqrt(0.18402f).  evaluate3D is held to td.REF64_TOL, so the grey level to that times INV / 8, plus half a
        # float32 ulp of a value in [0, 1] for the cast.
        want_host = _expand(pts, lambda p: host.texture(coef, p))
        same_bits(got[on], want_host[on], f"{name}: against the host evaluator")
        cells = (pts * f32(tp.TEX_CELLS)).astype(f32)
        noise = _expand(cells, lambda p: _ref64.evaluate3d_points(coef, p)) / np.sqrt(np.float64(f32(0.18402)))
        grey = 0.5 * (1.0 + np.clip(noise / 4.0, -1.0, 1.0))
        err = float(np.abs(got[on] - grey[on]).max())
        assert err <= td.REF64_TOL * float(INV32) / 8.0 + 2.0 ** -25, (name, err)
    elif entry == "proj":
        ref = _ref64.projected_points(coef, pts, tp._normals(n))
        assert (np.abs(got - ref) <= _ref64.projected_bound(pts)).all(), name
    elif entry == "mbproj":
        ref, bound = _ref64.multiband_projected_points(coef, pts, tp._normals(n), *extra, 0.296)
        assert (np.abs(got - ref) <= bound).all(), name
    if n >= N_LONG and entry not in ("proj", "mbproj"):
        step = tp.SORT_MIN // 2 + 5
        if n > N_LONG:                     # the row-slab lists: their first N_LONG points, and the last ragged stretch
            spans = [(a, min(a + step, N_LONG)) for a in range(0, N_LONG, step)] + [(n - step - 7, n)]
        else:
            spans = [(a, min(a + step, n)) for a in range(0, n, step)]
        for a, b in spans:
            short = tp.run_row(ctx, row[:4] + (b - a,) + row[5:], pts[a:b], None if active is None else active[a:b])
            torch.cuda.synchronize()
            same_bits(short.cpu().numpy(), got[a:b], f"{name}: the slice [{a}, {b}) against the long list")


POINT_SETS = ("magnitude", "binade")


def point_set(kind, cap, finest, seed, n=2000):
    """The list of set `kind` for a call whose finest coordinate is `finest` * p (a power of two)."""
    return magnitude_points(n, cap, seed, finest) if kind == "magnitude" else binade_points(1.0 / finest)


@pytest.mark.gpu
@pytest.mark.parametrize("pset", POINT_SETS)
@pytest.mark.parametrize("tile", ["t128", "t6"])
def test_far_points_gradient_and_curl(ctx, host, tile, pset):
    """evaluate3DGradient / evaluate3DCurl: the host evaluators' bits, the value channel the bits of evaluate3D, and the
    float64 references within the owning modules' tolerances."""
    import torch
    coef, obj = ctx.coef[tile], ctx.obj[tile]
    pts = point_set(pset, 30, 1.0, 11)
    td_ = torch.from_numpy(pts).cuda()
    grad = obj.evaluate3DGradient(td_).cpu().numpy()
    same_bits(grad, host.grad(coef, pts), f"{tile} {pset}: evaluate3DGradient against the host evaluator")
    same_bits(grad[:, 0], obj.evaluate3D(td_).cpu().numpy(), f"{tile} {pset}: the value channel against evaluate3D")
    err = np.abs(grad.astype(np.float64) - _ref64_grad.evaluate3d_grad_points(coef, pts)).max(0)
    assert (err <= _ref64_grad.tolerance()).all(), (tile, pset, err)
    curl = obj.evaluate3DCurl(td_, tc.MIXED).cpu().numpy()
    same_bits(curl, host.curl(coef, pts, tc.MIXED), f"{tile} {pset}: evaluate3DCurl against the host evaluator")
    err = np.abs(curl.astype(np.float64) - _ref64_curl.evaluate3d_curl_points(coef, pts, tc.MIXED)).max(0)
    assert (err <= _ref64_curl.tolerance()).all(), (tile, pset, err)


@pytest.mark.gpu
@pytest.mark.parametrize("pset", POINT_SETS + ("binade_low",))
def test_far_points_multiband_gradient_and_curl(ctx, pset):
    """WMultibandNoiseGradient / WMultibandNoiseCurl with the bands MB (finest coordinate 8 p <= 2^30; binade: the top band on
    the binade edges, binade_low: the lowest): the value channel has WMultibandNoise's bits, the curl is the subtraction of
    gradient channels on the rolled tiles, and both lie within the owning modules' tolerances of the float64 references."""
    import torch
    coef, obj = ctx.coef["t128"], ctx.obj["t128"]
    pts = binade_points(2.0) if pset == "binade_low" else point_set(pset, MB_CAP, 8.0, 12)
    assert float(np.abs(pts).max()) * 8.0 <= 2.0 ** 30
    td_ = torch.from_numpy(pts).cuda()
    band = MB + (0.18402,)
    grad = obj.WMultibandNoiseGradient(td_, *MB).cpu().numpy()
    same_bits(grad[:, 0], obj.WMultibandNoise(td_, *MB).cpu().numpy(), f"{pset}: the value channel against WMultibandNoise")
    err = np.abs(grad.astype(np.float64) - _ref64_grad.multiband_grad_points(coef, pts, *band)).max(0)
    assert (err <= _ref64_grad.tolerance(1.0, band)).all(), (pset, err)
    curl = obj.WMultibandNoiseCurl(td_, *MB, offsets=tc.MIXED).cpu().numpy()
    rolled = [ctx.wn.WaveletNoise.from_coefficients(t, 3) for t in _ref64_curl.rolled_tiles(coef, tc.MIXED)]
    same_bits(curl, tc.curl_f32(*[t.WMultibandNoiseGradient(td_, *MB).cpu().numpy() for t in rolled]),
              f"{pset}: WMultibandNoiseCurl against the gradients of the rolled tiles")
    err = np.abs(curl.astype(np.float64) - _ref64_curl.multiband_curl_points(coef, pts, tc.MIXED, *band)).max(0)
    assert (err <= _ref64_curl.tolerance(1.0, band)).all(), (pset, err)


@pytest.fixture(scope="module")
def perlin_host():
    lib = C.CDLL(os.path.join(PKG, "libwnoise_host.so"))
    IP, DP, FP, D = C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_float), C.c_double
    for name, res, args in (("wnhost_perlin_grad", D, [IP, D, D, D, DP]), ("wnhost_perlin_turb_grad", D, [IP, FP, C.c_int, DP]),
                            ("wnhost_perlin_fractal_grad", D, [IP, FP, DP]), ("wnhost_perlin_curl", None, [IP, D, D, D, IP, DP]),
                            ("wnhost_perlin_turb_curl", None, [IP, FP, C.c_int, IP, DP]),
                            ("wnhost_perlin_fractal_curl", None, [IP, FP, IP, DP])):
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    return lib


PERLIN_KINDS = [("noise64", 0, 30, 1.0), ("noise32", 0, 30, 1.0), ("turb", TURB_DEPTH, TURB_CAP, 64.0),
                ("fractal", 0, FRACTAL_CAP, 32.0)]


@pytest.mark.gpu
@pytest.mark.parametrize("pset", POINT_SETS)
@pytest.mark.parametrize("kind,depth,cap,finest", PERLIN_KINDS, ids=[k[0] for k in PERLIN_KINDS])
def test_far_points_perlin(ctx, perlin_host, ora, kind, depth, cap, finest, pset):
    """noise (double and float lists), turb and fractal_noise, their gradients and curls: the value against the oracle and
    the gradient's value channel bit for bit, gradient and curl records against the host evaluators bit for bit and within
    the owning modules' bounds of their references."""
    import torch
    p = ctx.perlin
    pts = point_set(pset, cap, finest, 13 + depth).astype(np.float64 if kind == "noise64" else f32)
    if kind == "noise64":
        pts = np.ascontiguousarray(pts * 0.9999999)           # doubles that are no floats
        assert float(np.abs(pts).max()) <= 2.0 ** 30
    td_ = torch.from_numpy(pts).cuda()
    rkind = "noise" if kind.startswith("noise") else kind
    if rkind == "noise":
        val, grad, want = p.noise(td_), p.noise_gradient(td_), ora.perlin_noise(ctx.perm, pts.astype(np.float64))
    elif kind == "turb":
        val, grad, want = p.turb(td_, depth), p.turb_gradient(td_, depth), ora.perlin_turb(ctx.perm, pts, depth)
    else:
        val, grad, want = p.fractal_noise(td_), p.fractal_noise_gradient(td_), ora.perlin_fractal(ctx.perm, pts)
    val, grad = val.cpu().numpy(), grad.cpu().numpy()
    curl = tpc.gpu_curl(p, kind, td_, depth).cpu().numpy()
    assert (tpg.bits64(val) == tpg.bits64(np.asarray(want, np.float64))).all(), (kind, pset)
    assert (tpg.bits64(grad[:, 0]) == tpg.bits64(val)).all(), (kind, pset)
    assert (tpg.bits64(grad) == tpg.bits64(tpg.host_records(perlin_host, p.p, kind, pts, depth))).all(), (kind, pset)
    assert (tpg.bits64(curl) == tpg.bits64(tpc.host_records(perlin_host, p.p, kind, pts, depth))).all(), (kind, pset)
    ref, s = RG.eval_records(p.p, rkind, pts, depth)
    keep = (np.abs(s) >= 1e-10) | (s == 0.0) if kind == "turb" else np.ones(len(pts), bool)
    err = np.abs(grad - ref)[keep].max(0)
    assert (err <= RG.bound(rkind, depth)).all(), (kind, pset, err)
    err = np.abs(curl - RC.velocity(p.p, rkind, pts, depth, tpc.OFF).astype(np.float64)).max(0)
    assert (err <= RC.bound(rkind, depth)).all(), (kind, pset, err)


@pytest.mark.gpu
@pytest.mark.parametrize("pset", POINT_SETS)
def test_far_points_wavelet_footprints(ctx, pset):
    """The per-sample footprint entry points (value, projected, gradient, projected gradient, texture; bands FOOT, finest
    coordinate 32 p <= 2^30): the host evaluators' bits, the gradient records within _ref64_footprint's tolerance."""
    nm, coef, obj = ctx.nm, ctx.coef["t128"], ctx.obj["t128"]
    fhost = F.bind_host(C.CDLL(os.path.join(PKG, "libwnoise_host.so")))
    first, nb = FOOT
    pts = point_set(pset, FOOT_CAP, 32.0, 14, n=1500)
    n = len(pts)
    w, s, nrs = F.weights(nb, first), F.footprints(first, nb, n, 15), F.normals(n, 16)
    for fade in (0, 1):
        got = {k: tfp.run(nm, k, obj, pts, nrs, s, first, nb, w, fade) for k in tfp.KINDS}
        want = tfp.host_records(fhost, coef, pts, nrs, s, first, nb, w, fade)
        for k in tfp.KINDS:
            same_bits(got[k], want[k], f"footprint {k} {pset} fade {fade}: against the host evaluator")
        ref, _ = F.multiband_footprint_points(coef, pts, None, s, first, nb, w, tfp.VAR, fade)
        err = np.abs(got["grad"].astype(np.float64) - ref)
        assert (err <= F.tolerance(s, first, nb, w, tfp.VAR)[:, None]).all(), (pset, fade, err.max(0))


@pytest.mark.gpu
@pytest.mark.parametrize("pset", POINT_SETS)
def test_far_points_perlin_footprints(ctx, pset):
    """turb / fractal_noise footprint lists (7 octaves: finest coordinate 64 p <= 2^30), their gradients and the texture: the
    host evaluators' bits."""
    nm, p = ctx.nm, ctx.perlin
    table = np.ascontiguousarray(p.p, np.int32)
    fhost = RPF.bind_host(C.CDLL(os.path.join(PKG, "libwnoise_host.so")))
    pts = point_set(pset, TURB_CAP, 64.0, 17, n=1500)
    s = RPF.footprints(7, 0.0, len(pts), 18)
    for fade in (0, 1):
        got = {k: tpf.run(nm, k, p, pts, s, 7, 0.0, fade) for k in tpf.KINDS}
        want = tpf.host_records(fhost, table, pts, s, 7, 0.0, fade)
        for k in tpf.KINDS:
            assert (tpf.bits(got[k]) == tpf.bits(want[k].astype(tpf.np_dtype(k)))).all(), (k, pset, fade)


@pytest.mark.gpu
@pytest.mark.parametrize("stream", ["one", "stream"])
@pytest.mark.parametrize("kind", tfp.KINDS)
def test_collapsed_footprint_lists_have_the_bits_of_their_slices(ctx, kind, stream):
    """Collapsed lists of N_LONG points through the footprint entry points (their chunked kernels from SORT_MIN points;
    the texture also masked) against slices of SORT_MIN / 2 + 5 points, bit for bit."""
    nm, obj = ctx.nm, ctx.obj["t128"]
    first, nb = FOOT
    w = F.weights(nb, first)
    pts = (collapsed(stream, N_LONG) / f32(4.0)).astype(f32)      # 32 * 2^24 = 2^29
    assert float(np.abs(pts).max()) * 32.0 <= 2.0 ** 30
    s, nrs = F.footprints(first, nb, N_LONG, 19), F.normals(N_LONG, 20)
    masks = [None] + ([(np.random.default_rng(21).random(N_LONG) < 0.4).astype(np.uint8)] if kind == "tex" else [])
    step = tfp.SORT_MIN // 2 + 5
    for active in masks:
        long_ = tfp.run(nm, kind, obj, pts, nrs, s, first, nb, w, 1, active=active, fill=-7.0)
        short = np.concatenate([tfp.run(nm, kind, obj, pts[a:a + step], nrs[a:a + step], s[a:a + step], first, nb, w, 1,
                                        active=None if active is None else active[a:a + step], fill=-7.0)
                                for a in range(0, N_LONG, step)])
        same_bits(long_, short, f"footprint {kind} {stream}: the long list against its slices")
        if active is not None:
            assert (long_[active == 0] == -7.0).all() and (long_[active != 0] != -7.0).all()


@pytest.mark.parametrize("pset", POINT_SETS + ("one", "stream"))
@pytest.mark.parametrize("tile", ["t128", "t6"])
def test_host_evaluators_within_bounds_on_the_far_point_sets(host, cpu_coefs, tile, pset):
    """CPU precondition of the point tests: evaluate3D, its gradient and curl, and every band of MB, by the host's exact
    evaluators against the float64 references within the owning modules' tolerances."""
    coef = cpu_coefs[tile]
    if pset in POINT_SETS:
        pts, mb_pts = point_set(pset, 30, 1.0, 11), point_set(pset, MB_CAP, 8.0, 12)
    else:
        pts = collapsed(pset, N_LONG)
        pts = mb_pts = np.ascontiguousarray(pts[runs_of(pts)[0]])
    err = float(np.abs(host.eval3d(coef, pts) - _ref64.evaluate3d_points(coef, pts)).max())
    assert err <= td.REF64_TOL, (tile, pset, err)
    err = np.abs(host.grad(coef, pts) - _ref64_grad.evaluate3d_grad_points(coef, pts)).max(0)
    assert (err <= _ref64_grad.tolerance()).all(), (tile, pset, err)
    err = np.abs(host.curl(coef, pts, tc.MIXED) - _ref64_curl.evaluate3d_curl_points(coef, pts, tc.MIXED)).max(0)
    assert (err <= _ref64_curl.tolerance()).all(), (tile, pset, err)
    for b in range(MB[2]):
        q = band_points(mb_pts, MB[1], b)
        assert float(np.abs(q).max()) <= 2.0 ** 30
        err = float(np.abs(host.eval3d(coef, q) - _ref64.evaluate3d_points(coef, q)).max())
        assert err <= td.REF64_TOL, (tile, pset, b, err)


if __name__ == "__main__" and "--child" in sys.argv:
    _child()
if __name__ == "__main__" and "--child-points" in sys.argv:
    _points_child()
