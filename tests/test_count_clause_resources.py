"""Resources of the two kernels of phrase and group clauses in fg_count_batch
(k_crow, k_cjoin), read from the gfx950 code object inside the
built libfugu.so (no GPU needed), by test_count_resources.py's method: each exists
exactly once, none uses scratch or spills a VGPR (both hold kCountItems docs per
lane in registers across their probe loops), at most 128 VGPRs, and LDS of at
most 40 KB -- k_crow's survivor queue -- so four workgroups fit a CU's 160 KB."""
import os

import pytest

from test_kernel_resources import LIB, LLVM, kernel_meta

KERNELS = ("k_crow", "k_cjoin")


@pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(f"{LLVM}/llvm-readelf")),
                    reason="needs the built libfugu.so and the ROCm LLVM tools")
def test_count_clause_kernel_resources(tmp_path):
    meta = kernel_meta(tmp_path)
    for k in KERNELS:
        mine = {n: v for n, v in meta.items() if k in n}
        assert len(mine) == 1, (k, sorted(meta))
        (name, v), = mine.items()
        figures = (f"{k}: {v['vgpr_count']} VGPRs, {v['lds']} B LDS, {v['private_segment_fixed_size']} B scratch, "
                   f"{v['vgpr_spill_count']} VGPR spills")
        print(figures)
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0, figures
        assert v["vgpr_count"] <= 128 and v["lds"] <= 40 * 1024, figures
