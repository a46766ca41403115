"""Resources of fg_count_batch's kernels (k_cfilter, k_cmatch, k_ccount, k_cfacet),
read from the gfx950 code object inside the built libfugu.so (no GPU needed), by
test_kernel_resources.py's method: none uses scratch or spills a VGPR -- k_cmatch
holds kCountItems (8) docs and k_cfacet kCountFacetItems (32) docs per lane in registers
across its probe / query loops, and a spill would put scratch traffic on every
one of them."""
import os

import pytest

from test_kernel_resources import LIB, LLVM, kernel_meta

KERNELS = ("k_cfilter", "k_cmatch", "k_ccount", "k_cfacet")


@pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(f"{LLVM}/llvm-readelf")),
                    reason="needs the built libfugu.so and the ROCm LLVM tools")
def test_count_kernel_resources(tmp_path):
    meta = kernel_meta(tmp_path)
    for k in KERNELS:
        mine = {n: v for n, v in meta.items() if k in n}
        assert len(mine) == 1, (k, sorted(meta))
        (name, v), = mine.items()
        figures = f"{k}: {v['vgpr_count']} VGPRs, {v['lds']} B LDS, {v['private_segment_fixed_size']} B scratch"
        print(figures)
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0, figures
        assert v["vgpr_count"] <= 128 and v["lds"] <= 1024, figures
