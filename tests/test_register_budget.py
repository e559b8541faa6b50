"""The plane pipeline's store waves wait with `s_waitcnt vmcnt(8)` for the next brick's box rows
(csrc/wn_wavelet_multiband.hip): a count of their own vector-memory instructions, correct only while the compiler adds
none to that path.  Register spills would (scratch loads and stores are vector-memory instructions), and the wait would
then let collapse waves read box rows that have not landed.  This compiles the kernel with the Makefile's own command
line for the device only, and asserts that no instantiation grid3d_mbp_kernel<1..5> uses scratch."""
import re

from _device_asm import assert_no_scratch, device_assembly


def test_plane_pipeline_kernels_use_no_scratch(tmp_path):
    text = device_assembly("wn_wavelet_multiband", tmp_path)
    for nb in range(1, 6):
        sym = f"_ZN12_GLOBAL__N_117grid3d_mbp_kernelILi{nb}EEEvNS_6MbArgsE"
        assert_no_scratch(text, sym)
        meta = re.search(rf"\.name:\s+{sym}\n(?:\s+\.[a-z_]+:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", text)
        assert meta and meta.group(1) == "0", f"grid3d_mbp_kernel<{nb}>: private segment {meta and meta.group(1)}"
