"""Resources of k_phrase, read from the gfx950 code object inside the built
libfugu.so (no GPU needed), by test_kernel_resources.py's method: both
instantiations (single- and multi-snapshot plans) use no scratch and spill no
VGPR, and their static LDS -- k_scan's top-k buffer and select histogram plus a
kChunk survivor queue, 37.3 KB -- stays within 40 KB, so four 256-thread
workgroups fit a CU's 160 KB beside their <= 128 VGPRs per lane."""
import os

import pytest

from test_kernel_resources import LIB, LLVM, kernel_meta


@pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(f"{LLVM}/llvm-readelf")),
                    reason="needs the built libfugu.so and the ROCm LLVM tools")
def test_k_phrase_resources(tmp_path):
    meta = {k: v for k, v in kernel_meta(tmp_path).items() if "k_phraseI" in k}
    assert len(meta) == 2, sorted(meta)
    for name, v in meta.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0, (name, v)
        assert v["vgpr_count"] <= 128 and v["lds"] <= 40 * 1024, (name, v)
