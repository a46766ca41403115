"""bench.py's counting rules (CPU).

At N > 1 the headline step is ONE fan-out batch: each of the nq queries runs on
every rank's namespace and comes back as one merged top-k list (all-gather +
k_merge_rank).  `value` therefore counts nq queries per step at every N; the
(query, namespace) pairs the ranks searched are a separate field.
"""
import ast
import os

from conftest import ROOT


def _bench():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_fanout_value_counts_merged_queries():
    b = _bench()
    for world in (1, 2, 4, 8):
        f = b.throughput_fields(1024, world, 20, 0.025)
        assert f["value"] == round(1024 * 20 / 0.025, 1)  # 1024 merged answers per step, whatever N
        assert f["namespace_queries_per_s"] == round(1024 * world * 20 / 0.025, 1)
        assert f["queries_per_step"] == 1024


def test_headline_value_comes_from_throughput_fields():
    """The headline line's `value` is throughput_fields(...)['value'] (no other
    query count is multiplied by the world size)."""
    src = open(os.path.join(ROOT, "bench.py")).read()
    tree = ast.parse(src)
    main = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "main")
    body = ast.unparse(main)
    assert "tput = throughput_fields(nq, world, args.steps, elapsed)" in body
    assert "qps = tput['value']" in body
    assert "nq * world * args.steps" not in body


def test_dump_outputs_writes_the_hits_and_masks_the_rest(tmp_path):
    """--dump-outputs: scores f32, docs / counts f64, [nq, K]; slots past a
    query's count (undefined device words) come out as score 0, doc -1, so the
    files depend on the hits alone."""
    import numpy as np
    b = _bench()
    K = 4
    n = np.array([4, 2, 0], np.int32)
    s = np.arange(12, dtype=np.float32) + 0.5
    d = np.array([7, 6, 5, 4, 0xFFFFFFF0, 2, 99, 98, 97, 96, 95, 94], np.uint32).view(np.int32)  # as torch int32
    for junk in (0, 12345):  # different leftovers past the counts: identical files
        s2, d2 = s.copy(), d.copy()
        s2[6:] += junk
        d2[6:] += junk
        out = tmp_path / f"dump{junk}"
        b.dump_outputs(str(out), s2, d2, n, K)
        sc, dc, nc = (np.load(out / f"{x}.npy") for x in ("scores", "docs", "counts"))
        assert sc.dtype == np.float32 and dc.dtype == np.float64 and nc.dtype == np.float64
        assert sc.shape == dc.shape == (3, K) and nc.tolist() == [4.0, 2.0, 0.0]
        assert sc.tolist() == [[0.5, 1.5, 2.5, 3.5], [4.5, 5.5, 0, 0], [0, 0, 0, 0]]
        assert dc.tolist() == [[7, 6, 5, 4], [float(0xFFFFFFF0), 2, -1, -1], [-1, -1, -1, -1]]


def test_plain_run_skips_what_full_runs():
    """Without --full the run is the timed steps and the result line: the CPU
    baseline, the secondary workloads, the traffic models and the batch-of-one
    latencies are switched off before anything is set up."""
    src = open(os.path.join(ROOT, "bench.py")).read()
    main = next(n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == "main")
    body = ast.unparse(main)
    assert "'--full'" in body and "'--dump-outputs'" in body
    gate = body.index("if not args.full:")
    assert gate < body.index("import torch")
    head = body[gate:body.index("import torch")]
    assert "args.no_cpu = args.no_extra = args.no_model = True" in head and "args.p50_queries = 0" in head


def test_roofline_carries_three_fractions():
    """Every kernel line's roofline quotes the model's fraction, the fraction at
    each query's final threshold (frac_pruned) and the measured DRAM fraction; a
    model more than 1.5x the measured DRAM bytes is not the line's `frac`
    (C3's exhaustive cascade read 0.89 where the kernel moved
    0.38 of HBM)."""
    b = _bench()
    model = {"alg_bytes": 7.5e9, "stream_bytes": 5e9, "probe_bytes": 2.5e9, "output_bytes": 0,
             "line_bytes": 1.7e9, "query_line_bytes": 9e9}
    pruned = {"alg_bytes": 2.0e9, "line_bytes": 1.5e9, "query_line_bytes": 2.6e9}
    orig = b.measured_traffic
    try:
        b.measured_traffic = lambda key: (3.2e9, "profiles/test.json")
        r = b.roofline("k_conj", 1.0, model, "k", "exhaustive cascade", pruned)
        assert r["frac_model"] == round(7.5e9 / 1e-3 / 1e9 / b.HBM_PEAK_GBS, 4)
        assert r["frac_pruned"] == round(2.0e9 / 1e-3 / 1e9 / b.HBM_PEAK_GBS, 4)
        assert r["frac"] == r["hbm_frac_measured"] == round(3.2e9 / 1e-3 / 1e9 / b.HBM_PEAK_GBS, 4)
        assert "measured" in r["frac_rule"]
        b.measured_traffic = lambda key: (6.0e9, "profiles/test.json")
        r = b.roofline("k_conj", 1.0, model, "k", "exhaustive cascade", pruned)
        assert r["frac"] == r["frac_model"] and r["frac_pruned"] < r["frac"]
        b.measured_traffic = lambda key: (None, "no profile")
        r = b.roofline("k_disj", 1.0, model, "k", "k_disj at each query's final k-th score")
        assert r["frac"] == r["frac_model"] == r["frac_pruned"] and r["traffic"] is None
    finally:
        b.measured_traffic = orig
