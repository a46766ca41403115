"""fg_count_batch against the bytes it must move: hit totals and facet counts on a
1M-doc synthetic namespace whose docs carry one facet of a three-level tree
(16 x 16 x 8 leaves; 10% of the docs none; 3% deleted).

  (a) the AllQuery facet tree: ONE call whose count terms are all 2320 facets,
      against the same tree taken as one call per tree node (273 calls, each
      node's children as count terms) -- the reference's collect_facets_recursive;
  (b) a 64-query OR-2 batch with 32 count terms (the 16 top-level facets and 16
      second-level ones).

Device time per kernel from HIP events around k_cfilter / k_cmatch / k_ccount /
k_cfacet of every call (fg_count_trace), wall time around the calls.  The byte
model per kernel: k_cmatch its streamed driver postings (4 B each) or, for
AllQuery, the filled bitmap words; k_ccount every bitmap word read and written
plus the alive words per query; k_cfacet its streamed facet postings once plus
every query's bitmap once.  hbm_frac = bytes / time / 8 TB/s.

  python tools/bench_count.py [--docs N] [--steps S] [--warmup W] [--out FILE]

Prints one JSON line and writes it to --out (default profiles/count/bench_count.json).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12
L1, L2, L3 = 16, 16, 8


def facet_tokens(n_docs, seed=11):
    """per doc the FacetTokenizer tokens of one leaf facet /a/b/c: root, /a, /a/b, /a/b/c
    (ids: 0, 1 + a, 17 + a*16 + b, 273 + (a*16 + b)*8 + c); 10% of the docs carry none"""
    rng = np.random.RandomState(seed)
    a, b, c = rng.randint(0, L1, n_docs), rng.randint(0, L2, n_docs), rng.randint(0, L3, n_docs)
    has = rng.random_sample(n_docs) >= 0.10
    ab = a * L2 + b
    tok = np.stack([np.zeros(n_docs, np.int64), 1 + a, 1 + L1 + ab, 1 + L1 + L1 * L2 + ab * L3 + c], 1)
    off = np.zeros(n_docs + 1, np.uint64)
    off[1:] = np.cumsum(np.where(has, 4, 0))
    return off, tok[has].reshape(-1).astype(np.uint32), 1 + L1 + L1 * L2 + L1 * L2 * L3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "count", "bench_count.json"))
    args = ap.parse_args()
    from fugu_amd import native, synth
    global KERNELS
    KERNELS = native.COUNT_KERNELS

    def trace(enable):
        ms, n = native.count_trace(enable)
        return [ms[k] for k in KERNELS], n

    N = args.docs
    corp = synth.corpus(N)
    f_off, f_tok, n_ft = facet_tokens(N)
    deleted = (np.random.RandomState(3).random_sample(N) < 0.03).astype(np.uint8)
    ctx = native.Context((0,))
    ix = native.Index.from_docs(ctx, corp.off, corp.tok, synth.VOCAB, deleted=deleted, facets=(f_off, f_tok, n_ft))
    words = (N + 31) // 32
    flen = np.bincount(f_tok, minlength=n_ft).astype(np.int64)  # one posting per (doc, token): tokens are distinct per doc

    def measure(calls):
        """calls: a list of (q_off, terms, count_terms, mode) making ONE round"""
        def round_():
            for q_off, terms, cts, mode in calls:
                native.count_batch([ix], q_off, terms, cts, mode=mode)
        for _ in range(args.warmup):
            round_()
        trace(1)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            round_()
        wall = (time.perf_counter() - t0) * 1e3 / args.steps
        ms, n = trace(0)
        assert n == args.steps * len(calls)
        return {"wall_ms": wall, "calls": len(calls), **{k: m / args.steps for k, m in zip(KERNELS, ms)}}

    def with_model(r, bytes_by_kernel):
        r["bytes"] = bytes_by_kernel
        r["hbm_frac"] = {k: (b / (r[k] * 1e-3) / HBM_BYTES_PER_S if r[k] > 0 else 0.0) for k, b in bytes_by_kernel.items()}
        r["kernels_ms"] = sum(r[k] for k in KERNELS)
        return r

    empty = (np.zeros(2, np.uint32), np.zeros(0, np.uint32))
    # (a) the whole tree in one call
    all_terms = np.arange(1, n_ft, dtype=np.uint32)
    one = with_model(measure([(empty[0], empty[1], all_terms, native.MODE_AND)]), {
        "k_cfilter": 0, "k_cmatch": 4 * words, "k_ccount": 3 * 4 * words,
        "k_cfacet": int(4 * flen[1:].sum() + 4 * words)})
    total, count = native.count_batch([ix], empty[0], empty[1], all_terms)
    # ... and per node, the reference's call pattern: root, 16 first-level and 256 second-level nodes
    nodes = [np.arange(1, 1 + L1, dtype=np.uint32)]
    nodes += [np.arange(1 + L1 + a * L2, 1 + L1 + (a + 1) * L2, dtype=np.uint32) for a in range(L1)]
    nodes += [np.arange(1 + L1 + L1 * L2 + ab * L3, 1 + L1 + L1 * L2 + (ab + 1) * L3, dtype=np.uint32)
              for ab in range(L1 * L2)]
    per_node = with_model(measure([(empty[0], empty[1], cts, native.MODE_AND) for cts in nodes]), {
        "k_cfilter": 0, "k_cmatch": 4 * words * len(nodes), "k_ccount": 3 * 4 * words * len(nodes),
        "k_cfacet": int(4 * flen[1:].sum() + 4 * words * len(nodes))})
    got = np.concatenate([native.count_batch([ix], empty[0], empty[1], cts)[1][0] for cts in nodes])
    assert np.array_equal(got, count[0]) and int(total[0]) == int((deleted == 0).sum())
    # (b) 64 OR-2 queries, 32 count terms
    q_off, terms = synth.queries(64, 2, 2, seed_q=21)
    cts32 = np.concatenate([np.arange(1, 1 + L1), np.arange(1 + L1, 1 + 2 * L1)]).astype(np.uint32)
    driver = int(sum(ix.df(int(t)) for t in terms))
    orb = with_model(measure([(q_off, terms, cts32, native.MODE_OR)]), {
        "k_cfilter": 0, "k_cmatch": 4 * driver, "k_ccount": 64 * 3 * 4 * words,
        "k_cfacet": int(4 * flen[cts32].sum() + 64 * 4 * words)})
    orb["driver_postings"] = driver
    out = {"docs": N, "facet_terms": n_ft, "facet_postings": int(flen.sum()), "steps": args.steps, "warmup": args.warmup,
           "tree_one_call": one, "tree_per_node": per_node, "or2_64q_32terms": orb,
           "tree_speedup_wall": per_node["wall_ms"] / one["wall_ms"], "version": native.version()}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
