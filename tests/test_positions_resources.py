"""Resources of fg_index_build_positional's kernels (k_fwd_*: DESIGN.md §13), read
from the gfx950 code object inside the built libfugu.so (no GPU needed), by
test_kernel_resources.py's method: each is ONE kernel (the two scans share their
three kernels: the item width is a run-time choice, not a template parameter),
none uses scratch or spills a VGPR, and none needs more than 128 VGPRs (4
waves/SIMD: a background build must leave wave slots to searches)."""
import os

import pytest

from test_kernel_resources import LIB, LLVM, kernel_meta

KERNELS = ("k_fwd_reduce", "k_fwd_spine", "k_fwd_prefix", "k_fwd_len", "k_fwd_fill", "k_fwd_scatter", "k_fwd_check")


@pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(f"{LLVM}/llvm-readelf")),
                    reason="needs the built libfugu.so and the ROCm LLVM tools")
def test_positions_kernel_resources(tmp_path):
    meta = kernel_meta(tmp_path)
    for k in KERNELS:
        mine = {n: v for n, v in meta.items() if k in n}
        assert len(mine) == 1, (k, sorted(meta))
        (name, v), = mine.items()
        figures = f"{k}: {v['vgpr_count']} VGPRs, {v['lds']} B LDS, {v['private_segment_fixed_size']} B scratch"
        print(figures)
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0, figures
        assert v["vgpr_count"] <= 128, figures
    # no new name holds (or is held by) another kernel's: the resource tests select by substring
    for n in meta:
        hits = [k for k in KERNELS if k in n]
        assert len(hits) <= 1, (n, hits)
