"""The plane pipeline's store waves wait with `s_waitcnt vmcnt(8)` for the next brick's box rows
(csrc/wn_wavelet_multiband.hip): a count of their own vector-memory instructions, correct only while the compiler adds
none to that path.  Register spills would (scratch loads and stores are vector-memory instructions), and the wait would
then let collapse waves read box rows that have not landed.  This compiles the kernel with the Makefile's own command
line for the device only, and asserts that no instantiation grid3d_mbp_kernel<1..5> uses scratch."""
import os
import re
import shlex
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "wavelet-noise-in-ray-tracing_amd")
SRC = "csrc/wn_wavelet_multiband.hip"


def _makefile_compile_command():
    out = subprocess.run(["make", "--no-print-directory", "-n", "-B", "-C", PKG, "build/wn_wavelet_multiband.o"],
                         capture_output=True, text=True, check=True).stdout
    lines = [ln for ln in out.splitlines() if SRC in ln and " -c " in ln]
    assert len(lines) == 1, out
    return shlex.split(lines[0])


def test_plane_pipeline_kernels_use_no_scratch(tmp_path):
    cmd = _makefile_compile_command()
    i = cmd.index("-o")
    del cmd[i:i + 2]
    cmd.remove("-c")
    asm = tmp_path / "wn_wavelet_multiband.s"
    cmd += ["--cuda-device-only", "-S", "-o", str(asm)]
    res = subprocess.run(cmd, cwd=PKG, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr
    text = asm.read_text()
    for nb in range(1, 6):
        sym = f"_ZN12_GLOBAL__N_117grid3d_mbp_kernelILi{nb}EEEvNS_6MbArgsE"
        # the function body: from its label to its .Lfunc_end label
        body = re.search(rf"^{sym}:[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M)
        assert body, f"grid3d_mbp_kernel<{nb}> not found in the device assembly"
        assert "scratch_" not in body.group(1), f"grid3d_mbp_kernel<{nb}> spills to scratch"
        kd = re.search(rf"^\s*\.amdhsa_kernel {sym}\n(.*?)^\s*\.end_amdhsa_kernel", text, re.S | re.M)
        assert kd, nb
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\n", kd.group(1)), f"grid3d_mbp_kernel<{nb}> has a private segment"
        meta = re.search(rf"\.name:\s+{sym}\n(?:\s+\.[a-z_]+:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", text)
        assert meta and meta.group(1) == "0", f"grid3d_mbp_kernel<{nb}>: private segment {meta and meta.group(1)}"
