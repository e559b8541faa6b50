"""What the register-budget tests share: the device assembly of one csrc/*.hip file, compiled with the Makefile's own
command line for the device only, and the resources its kernel descriptors declare."""
import os
import re
import shlex
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "wavelet-noise-in-ray-tracing_amd")


def device_assembly(stem, tmp_path):
    """The device assembly of csrc/<stem>.hip, compiled as the Makefile compiles it."""
    src = f"csrc/{stem}.hip"
    out = subprocess.run(["make", "--no-print-directory", "-n", "-B", "-C", PKG, f"build/{stem}.o"],
                         capture_output=True, text=True, check=True).stdout
    lines = [ln for ln in out.splitlines() if src in ln and " -c " in ln]
    assert len(lines) == 1, out
    cmd = shlex.split(lines[0])
    i = cmd.index("-o")
    del cmd[i:i + 2]
    cmd.remove("-c")
    asm = tmp_path / f"{stem}.s"
    cmd += ["--cuda-device-only", "-S", "-o", str(asm)]
    res = subprocess.run(cmd, cwd=PKG, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr
    return asm.read_text()


def kernels(text):
    """The symbols that have a kernel descriptor."""
    return set(re.findall(r"^\s*\.amdhsa_kernel (\S+)", text, re.M))


def descriptor(text, sym):
    """The integer fields of sym's kernel descriptor: next_free_vgpr, group_segment_fixed_size (static LDS), ..."""
    kd = re.search(rf"^\s*\.amdhsa_kernel {sym}\n(.*?)^\s*\.end_amdhsa_kernel", text, re.S | re.M)
    assert kd, f"{sym} has no kernel descriptor"
    return {k: int(v) for k, v in re.findall(r"\.amdhsa_(\w+) (\d+)\n", kd.group(1))}


def assert_no_scratch(text, sym):
    body = re.search(rf"^{sym}:[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M)
    assert body, f"{sym} not found in the device assembly"
    assert "scratch_" not in body.group(1), f"{sym} spills to scratch"
    assert descriptor(text, sym)["private_segment_fixed_size"] == 0, f"{sym} has a private segment"


def waves_per_simd(vgprs):
    """Waves that fit a SIMD's 512 VGPRs when each allocates next_free_vgpr rounded up to the granule of 8; at most 8."""
    return min(8, 512 // (-(-vgprs // 8) * 8))
