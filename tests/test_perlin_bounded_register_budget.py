"""The kernels of csrc/wn_perlin_bounded.hip (include/wnoise_perlin_bounded.h): perlin_potential_points_kernel,
perlin_curl_bounded_points_kernel<KIND> and perlin_curl_bounded_advect_kernel<KIND, METHOD>, and nothing else.  This compiles
the file with the Makefile's own command line for the device only and reads the kernel descriptors: every kernel's LDS is the
512-byte permutation table, and none has a private segment.  Each instantiation's VGPRs and the waves per SIMD they allow are
printed beside those of perlin_curl_advect_kernel (csrc/wn_perlin_advect.hip); no occupancy is asserted."""
import pytest

from _device_asm import descriptor, device_assembly, kernels, waves_per_simd


def mangled(name, targs, arg):
    return f"_ZN12_GLOBAL__N_1{len(name)}{name}{'I' + targs + 'E' if targs else ''}{'Ev' if targs else 'E'}NS_{len(arg)}{arg}E"


KIND_NAMES = {0: "noise", 1: "turb", 2: "fractal"}
METHOD_NAMES = {0: "euler", 1: "midpoint", 2: "rk4"}
POTENTIAL = mangled("perlin_potential_points_kernel", "", "PotentialPointsArgs")
POINTS = {k: mangled("perlin_curl_bounded_points_kernel", f"Li{k}E", "BoundedPointsArgs") for k in range(3)}
ADVECT = {(k, m): mangled("perlin_curl_bounded_advect_kernel", f"Li{k}ELi{m}E", "BoundedAdvectArgs") for k in range(3) for m in range(3)}
UNBOUNDED = {(k, m): mangled("perlin_curl_advect_kernel", f"Li{k}ELi{m}E", "PerlinAdvectArgs") for k in range(3) for m in range(3)}
KERNELS = [POTENTIAL] + list(POINTS.values()) + list(ADVECT.values())


@pytest.fixture(scope="module")
def text(tmp_path_factory):
    return device_assembly("wn_perlin_bounded", tmp_path_factory.mktemp("asm"))


@pytest.fixture(scope="module")
def unbounded_text(tmp_path_factory):
    return device_assembly("wn_perlin_advect", tmp_path_factory.mktemp("asm_unbounded"))


def test_the_kernel_set_is_the_expected_instantiations(text):
    assert len(KERNELS) == 13 and len(set(KERNELS)) == 13
    assert kernels(text) == set(KERNELS), sorted(kernels(text) ^ set(KERNELS))


def test_no_private_segment_and_the_lds_is_the_table(text, unbounded_text):
    def line(label, d):
        return (f"{label}: vgprs {d['next_free_vgpr']}, waves per SIMD {waves_per_simd(d['next_free_vgpr'])}, "
                f"sgprs {d['next_free_sgpr']}, static LDS {d['group_segment_fixed_size']} B")
    print()
    for sym, label in [(POTENTIAL, "perlin_potential_points_kernel")] + \
                      [(POINTS[k], f"perlin_curl_bounded_points_kernel<{KIND_NAMES[k]}>") for k in range(3)]:
        d = descriptor(text, sym)
        print(line(label, d))
        assert d["private_segment_fixed_size"] == 0, f"{label} has a private segment"
        assert d["group_segment_fixed_size"] == 512, label
    for (k, m), sym in ADVECT.items():
        d, u = descriptor(text, sym), descriptor(unbounded_text, UNBOUNDED[(k, m)])
        print(line(f"perlin_curl_bounded_advect_kernel<{KIND_NAMES[k]}, {METHOD_NAMES[m]}>", d))
        print(line(f"        perlin_curl_advect_kernel<{KIND_NAMES[k]}, {METHOD_NAMES[m]}>", u))
        assert d["private_segment_fixed_size"] == 0, f"{sym} has a private segment"
        assert d["group_segment_fixed_size"] == 512, sym
