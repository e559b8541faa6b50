"""The kernels of csrc/wn_perlin_bounded_bricks.hip (include/wnoise_perlin_bounded_bricks.h):
perlin_curl_bounded_bricks_kernel<KIND>, KIND = 0 noise, 1 turb, 2 fractal_noise, and nothing else.  This compiles the file with
the Makefile's own command line for the device only and reads the kernel descriptors: no kernel has a private segment and no
body spills to scratch; the static LDS of every instantiation is the permutation table plus one axis slice per wave, from the
constants the source states (kPermBytes + kWaves * kSliceBytes), with no dynamic LDS at the launch.  Each instantiation's
VGPRs and the waves per SIMD they allow are printed; no occupancy is asserted."""
import os
import re

import pytest

from _device_asm import PKG, assert_no_scratch, descriptor, device_assembly, kernels, waves_per_simd

KINDS = {0: "noise", 1: "turb", 2: "fractal_noise"}


def mangled(kind):
    name, arg = "perlin_curl_bounded_bricks_kernel", "PerlinBoundedBricksArgs"
    return f"_ZN12_GLOBAL__N_1{len(name)}{name}ILi{kind}EEEvNS_{len(arg)}{arg}E"


KERNELS = {k: mangled(k) for k in KINDS}


@pytest.fixture(scope="module")
def text(tmp_path_factory):
    return device_assembly("wn_perlin_bounded_bricks", tmp_path_factory.mktemp("asm"))


def constants():
    src = open(os.path.join(PKG, "csrc", "wn_perlin_bounded_bricks.hip")).read()
    c = {name: int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1)) for name in ("kWaves", "kPermBytes", "kSliceBytes")}
    assert "__launch_bounds__(64 * kWaves)" in src
    assert "static_assert(sizeof(BrickAxisSlice) == kSliceBytes" in src
    assert src.count("__shared__") == 2 and "s_perm[kPermBytes]" in src and "BrickAxisSlice s_axis[kWaves]" in src
    # the launch passes no dynamic LDS and 64 * kWaves lanes
    (launch,) = re.findall(r"hipLaunchKernel\(fn,[^;]*;", src)
    assert re.search(r"dim3\(256\), params, 0, wn::as_stream\(stream\)\);$", launch) and c["kWaves"] * 64 == 256, launch
    return c


def test_the_kernel_set_is_the_expected_instantiations(text):
    assert len(set(KERNELS.values())) == 3
    assert kernels(text) == set(KERNELS.values()), sorted(kernels(text) ^ set(KERNELS.values()))


def test_no_private_segment_and_the_lds_is_the_table_and_the_slices(text):
    c = constants()
    assert c == {"kWaves": 4, "kPermBytes": 512, "kSliceBytes": 24 * 3 * 8 + 24}
    lds = c["kPermBytes"] + c["kWaves"] * c["kSliceBytes"]
    print()
    for k, sym in KERNELS.items():
        d = descriptor(text, sym)
        print(f"perlin_curl_bounded_bricks_kernel<{KINDS[k]}>: vgprs {d['next_free_vgpr']}, waves per SIMD "
              f"{waves_per_simd(d['next_free_vgpr'])}, sgprs {d['next_free_sgpr']}, static LDS {d['group_segment_fixed_size']} B")
        assert_no_scratch(text, sym)
        assert d["group_segment_fixed_size"] == lds, (sym, d["group_segment_fixed_size"], lds)
