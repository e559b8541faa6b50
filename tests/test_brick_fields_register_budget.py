"""The kernels of csrc/wn_wavelet_brick_fields.hip (include/wnoise_brick_fields.h): brick_fields_exact_kernel<PADDED, MB,
CURL>, grad_bricks_sep_kernel<NB> and curl_bricks_sep_kernel<NB>, NB = 1..8, and nothing else.  This compiles the file with
the Makefile's own command line for the device only and reads the kernel descriptors: no kernel has a private segment and
no body spills; the exact kernels use no LDS, and a separable kernel's static LDS is its coefficient boxes alone -- two
bricks of NB boxes of kBoxCap floats for the gradient, of 3 NB boxes (one per potential) for the curl -- with no dynamic LDS
at the launch.  Each instantiation's VGPRs and the waves per SIMD they allow are printed; no occupancy is asserted."""
import os
import re

import pytest

from _device_asm import PKG, assert_no_scratch, descriptor, device_assembly, kernels, waves_per_simd


def mangled(name, targs, arg, shared=False):
    """A kernel of the file's unnamed namespace; its argument struct is the file's own, or wn::'s (shared)."""
    return f"_ZN12_GLOBAL__N_1{len(name)}{name}I{targs}EEv" + (f"N2wn{len(arg)}{arg}E" if shared else f"NS_{len(arg)}{arg}E")


EXACT = [mangled("brick_fields_exact_kernel", f"Lb{p}ELb{m}ELb{c}E", "FieldsExactArgs") for p in (0, 1) for m in (0, 1) for c in (0, 1)]
GRAD = {nb: mangled("grad_bricks_sep_kernel", f"Li{nb}E", "BrickSepArgs", True) for nb in range(1, 9)}
CURL = {nb: mangled("curl_bricks_sep_kernel", f"Li{nb}E", "BrickSepArgs", True) for nb in range(1, 9)}
KERNELS = EXACT + list(GRAD.values()) + list(CURL.values())


@pytest.fixture(scope="module")
def text(tmp_path_factory):
    return device_assembly("wn_wavelet_brick_fields", tmp_path_factory.mktemp("asm"))


def box_cap():
    src = open(os.path.join(PKG, "csrc", "wn_wavelet_brick_fields.hip")).read()
    (expr,) = re.findall(r"constexpr int kBoxCap = ([\d\s\*]+);", src)
    cap = 1
    for f in expr.split("*"):
        cap *= int(f)
    # the value bricks' box: the same cells under the same 8 samples
    assert re.findall(r"constexpr int kBoxCap = ([\d\s\*]+);", open(os.path.join(PKG, "csrc", "wn_wavelet_bricks.hip")).read()) == [expr]
    # the separable launches pass no dynamic LDS
    launches = re.findall(r"hipLaunchKernelGGL\((?:grad|curl)_bricks_sep_kernel<[^;]*;", src)
    assert len(launches) == 2 and all(re.search(r"blocks, block,\s*0, stream, a\);$", ln) for ln in launches), launches
    assert "kSepBlockCap)), block(256);" in src
    return cap


def test_the_kernel_set_is_the_expected_instantiations(text):
    assert len(KERNELS) == 24 and len(set(KERNELS)) == 24
    assert kernels(text) == set(KERNELS), sorted(kernels(text) ^ set(KERNELS))


def test_no_private_segment_and_the_lds_is_the_boxes(text):
    cap = box_cap()
    assert cap == 7 * 6 * 6 == 252
    print()
    for sym in EXACT:
        d = descriptor(text, sym)
        print(f"{sym}: vgprs {d['next_free_vgpr']}, waves per SIMD {waves_per_simd(d['next_free_vgpr'])}, "
              f"sgprs {d['next_free_sgpr']}, static LDS {d['group_segment_fixed_size']}")
        assert_no_scratch(text, sym)
        assert d["group_segment_fixed_size"] == 0, f"{sym} uses LDS"
    for name, table, boxes in (("grad_bricks_sep_kernel", GRAD, 1), ("curl_bricks_sep_kernel", CURL, 3)):
        for nb, sym in table.items():
            d = descriptor(text, sym)
            print(f"{name}<{nb}>: vgprs {d['next_free_vgpr']}, waves per SIMD {waves_per_simd(d['next_free_vgpr'])}, "
                  f"sgprs {d['next_free_sgpr']}, static LDS {d['group_segment_fixed_size']} B")
            assert_no_scratch(text, sym)
            assert d["group_segment_fixed_size"] == 2 * nb * boxes * cap * 4, (sym, d["group_segment_fixed_size"])
    assert 2 * 8 * 3 * cap * 4 == 48384 < 64 * 1024           # the largest: under the static limit
