"""Resources of k_fphrase, read from the gfx950 code object inside
the built libfugu.so (no GPU needed), by test_group_resources.py's method and with
k_bphrase's budget: both instantiations (single- and multi-snapshot plans) are
present, use no scratch and spill no VGPR, hold at most 128 VGPRs per lane (four
waves per SIMD) and at most 40 KB of static LDS (four 256-thread workgroups in a
CU's 160 KB).
The printed figures are kept in profiles/field_phrase/resources.txt."""
import os

import pytest

from test_kernel_resources import LIB, LLVM, kernel_meta


@pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(f"{LLVM}/llvm-readelf")),
                    reason="needs the built libfugu.so and the ROCm LLVM tools")
def test_k_fphrase_resources(tmp_path):
    meta = {k: v for k, v in kernel_meta(tmp_path).items() if "k_fphraseI" in k}
    assert len(meta) == 2, sorted(meta)
    for name, v in sorted(meta.items()):
        print(name, v)
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0, (name, v)
        assert v["vgpr_count"] <= 128 and v["lds"] <= 40 * 1024, (name, v)
