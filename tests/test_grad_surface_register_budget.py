"""Every kernel of csrc/wn_wavelet_grad_surface.hip (the 2-D point and grid kernels, the projected point and grid kernels
and the multiband projected point kernel) compiles without scratch: the projected cell loop is VALU-bound, and a spill
would add vector-memory traffic to every cell.  This compiles the file with the Makefile's own command line for the
device only and reads the kernel descriptors."""
import os
import re
import shlex
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "wavelet-noise-in-ray-tracing_amd")
SRC = "csrc/wn_wavelet_grad_surface.hip"

KERNELS = ["_ZN12_GLOBAL__N_120grad2d_points_kernelENS_14SurfPointsArgsE",
           "_ZN12_GLOBAL__N_128grad_projected_points_kernelENS_14SurfPointsArgsE",
           "_ZN12_GLOBAL__N_138grad_multiband_projected_points_kernelENS_14SurfPointsArgsE",
           "_ZN12_GLOBAL__N_118grad2d_grid_kernelENS_12SurfGridArgsE",
           "_ZN12_GLOBAL__N_126grad_projected_grid_kernelENS_12SurfGridArgsE"]


def _makefile_compile_command():
    out = subprocess.run(["make", "--no-print-directory", "-n", "-B", "-C", PKG, "build/wn_wavelet_grad_surface.o"],
                         capture_output=True, text=True, check=True).stdout
    lines = [ln for ln in out.splitlines() if SRC in ln and " -c " in ln]
    assert len(lines) == 1, out
    return shlex.split(lines[0])


def test_surface_gradient_kernels_use_no_scratch(tmp_path):
    cmd = _makefile_compile_command()
    i = cmd.index("-o")
    del cmd[i:i + 2]
    cmd.remove("-c")
    asm = tmp_path / "wn_wavelet_grad_surface.s"
    cmd += ["--cuda-device-only", "-S", "-o", str(asm)]
    res = subprocess.run(cmd, cwd=PKG, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr
    text = asm.read_text()
    found = set(re.findall(r"^\s*\.amdhsa_kernel (\S+)", text, re.M))
    assert found == set(KERNELS), sorted(found ^ set(KERNELS))
    for sym in KERNELS:
        body = re.search(rf"^{sym}:[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M)
        assert body, f"{sym} not found in the device assembly"
        assert "scratch_" not in body.group(1), f"{sym} spills to scratch"
        kd = re.search(rf"^\s*\.amdhsa_kernel {sym}\n(.*?)^\s*\.end_amdhsa_kernel", text, re.S | re.M)
        assert kd and re.search(r"\.amdhsa_private_segment_fixed_size 0\n", kd.group(1)), f"{sym} has a private segment"
