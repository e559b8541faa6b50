"""The kernels of csrc/wn_wavelet_bounded_bricks.hip (include/wnoise_bounded_bricks.h): bounded_bricks_exact_kernel<PADDED, MB>
and curl_bounded_bricks_sep_kernel<NB>, NB = 1..8, and nothing else.  This compiles the file with the Makefile's own command
line for the device only and reads the kernel descriptors: no kernel has a private segment and no body spills; the exact
kernels use no LDS, and a separable kernel's static LDS is its coefficient boxes -- two bricks of 3 NB boxes of kBoxCap floats,
as curl_bricks_sep_kernel's -- plus the kFlagBytes of per-wave flags the source names, with no dynamic LDS at the launch.
Each instantiation's VGPRs and the waves per SIMD they allow are printed; no occupancy is asserted."""
import os
import re

import pytest

from _device_asm import PKG, assert_no_scratch, descriptor, device_assembly, kernels, waves_per_simd


def mangled(name, targs, arg):
    return f"_ZN12_GLOBAL__N_1{len(name)}{name}I{targs}EEvNS_{len(arg)}{arg}E"


EXACT = [mangled("bounded_bricks_exact_kernel", f"Lb{p}ELb{m}E", "BoundedExactArgs") for p in (0, 1) for m in (0, 1)]
SEP = {nb: mangled("curl_bounded_bricks_sep_kernel", f"Li{nb}E", "BoundedSepArgs") for nb in range(1, 9)}
KERNELS = EXACT + list(SEP.values())


@pytest.fixture(scope="module")
def text(tmp_path_factory):
    return device_assembly("wn_wavelet_bounded_bricks", tmp_path_factory.mktemp("asm"))


def product(expr):
    out = 1
    for f in expr.split("*"):
        out *= int(f)
    return out


def source_constants():
    """kBoxCap and kFlagBytes as the source states them; the launches as it writes them."""
    src = open(os.path.join(PKG, "csrc", "wn_wavelet_bounded_bricks.hip")).read()
    (cap,) = re.findall(r"constexpr int kBoxCap = ([\d\s\*]+);", src)
    # the unbounded curl bricks' box: the same cells under the same 8 samples
    assert re.findall(r"constexpr int kBoxCap = ([\d\s\*]+);", open(os.path.join(PKG, "csrc", "wn_wavelet_brick_fields.hip")).read()) == [cap]
    (flags,) = re.findall(r"constexpr int kFlagBytes = ([\d\s\*]+);", src)
    assert "__shared__ int open_wave[kFlagBytes / 4];" in src
    # the separable launch passes no dynamic LDS, and both launches have 256 lanes
    launches = re.findall(r"hipLaunchKernelGGL\(curl_bounded_bricks_sep_kernel<[^;]*;", src)
    assert len(launches) == 1 and re.search(r"blocks, block,\s*0, stream, a\);$", launches[0]), launches
    assert "stride_blocks((n + 1) / 2 * 256, kBoundedSepBlockCap)), block(256);" in src
    assert "stride_blocks(d.count * kSamples, kBoundedExactBlockCap)), block(256);" in src
    return product(cap), product(flags)


def test_the_kernel_set_is_the_expected_instantiations(text):
    assert len(KERNELS) == 12 and len(set(KERNELS)) == 12
    assert kernels(text) == set(KERNELS), sorted(kernels(text) ^ set(KERNELS))


def test_no_private_segment_and_the_lds_is_the_boxes_and_the_flags(text):
    cap, flags = source_constants()
    assert cap == 7 * 6 * 6 == 252 and flags == 16        # one int for each of the workgroup's four waves
    print()
    for sym in EXACT:
        d = descriptor(text, sym)
        print(f"{sym}: vgprs {d['next_free_vgpr']}, waves per SIMD {waves_per_simd(d['next_free_vgpr'])}, "
              f"sgprs {d['next_free_sgpr']}, static LDS {d['group_segment_fixed_size']}")
        assert_no_scratch(text, sym)
        assert d["group_segment_fixed_size"] == 0, f"{sym} uses LDS"
    for nb, sym in SEP.items():
        d = descriptor(text, sym)
        print(f"curl_bounded_bricks_sep_kernel<{nb}>: vgprs {d['next_free_vgpr']}, waves per SIMD {waves_per_simd(d['next_free_vgpr'])}, "
              f"sgprs {d['next_free_sgpr']}, static LDS {d['group_segment_fixed_size']} B")
        assert_no_scratch(text, sym)
        assert d["group_segment_fixed_size"] == 2 * nb * 3 * cap * 4 + flags, (sym, d["group_segment_fixed_size"])
    assert 2 * 8 * 3 * cap * 4 + flags == 48400 < 64 * 1024        # the largest: under the static limit
