"""k_group (group clauses, fg_group_clauses) next to the nearest flat queries the
library runs without the switch, on a 1M-doc synthetic namespace: 1024 queries,
top-100, three shapes over terms drawn from one document each (so conjunctions
have hits) --
  must_any_term  `+(a b) +c`      beside `+a +c` (k_conj)
  dnf            `(a AND b) OR c` beside `a b c` (k_disj)
  cnf            `+(a b) +(c d)`  beside `+a +c` (k_conj)
Device time from HIP events around the search kernels of every execute
(fg_plan_profile), warm-up first, the plans of a shape alternating over two
rounds: the spread between the rounds is the noise of the comparison.  There is
no target: without the switch these queries do not run on the device at all,
and the flat neighbours are different queries (fewer or more hits).

  python tools/bench_group.py [--docs N] [--queries Q] [--k K] [--steps S] [--warmup W] [--out FILE]

Prints one JSON line and writes it to --out (default profiles/group/bench_group.json).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.bench_phrase import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group", "bench_group.json"))
    args = ap.parse_args()
    from fugu_amd import native, synth
    if native.device_count() == 0:
        raise SystemExit("bench_group: no GPU visible")
    ctx = native.Context((0,))
    c = synth.corpus(args.docs, threads=16)
    ix = native.Index.from_docs(ctx, c.off, c.tok, synth.VOCAB, threads=16, keep_host=False)
    r = np.random.default_rng(13)

    def four():  # four distinct terms of one document
        while True:
            d = int(r.integers(0, args.docs))
            t = np.unique(c.tok[int(c.off[d]):int(c.off[d + 1])])
            if len(t) >= 4:
                return [int(x) for x in r.choice(t, 4, replace=False)]

    words = [four() for _ in range(args.queries)]
    S, M = native.OCCUR_SHOULD, native.OCCUR_MUST
    ANY, ALL = native.CLAUSE_ANY, native.CLAUSE_ALL

    def plan(rows):
        """rows: per query [(occur, flag or 0, [terms])]"""
        q_off = np.cumsum([0] + [sum(len(t) for _, _, t in q) for q in rows]).astype(np.uint32)
        terms = np.array([x for q in rows for _, _, t in q for x in t], np.uint32)
        occur = np.array([oc for q in rows for oc, _, t in q for _ in t], np.uint8)
        plen = np.array([(len(t) | fl if fl else 1) if j == 0 else 0 for q in rows for _, fl, t in q
                         for j in range(len(t))], np.uint32)
        if not any(fl for q in rows for _, fl, _ in q):
            return ix.plan(q_off, terms, args.k, occur=occur)
        return ix.plan(q_off, terms, args.k, occur=occur, phrase_len=plen, phrase_pos=np.zeros(len(terms), np.uint32))

    shapes = {
        "must_any_term": {"k_group": [[(M, ANY, [a, b]), (M, 0, [c_])] for a, b, c_, _ in words],
                          "k_conj_flat": [[(M, 0, [a]), (M, 0, [c_])] for a, b, c_, _ in words]},
        "dnf": {"k_group": [[(S, ALL, [a, b]), (S, 0, [c_])] for a, b, c_, _ in words],
                "k_disj_flat": [[(S, 0, [a]), (S, 0, [b]), (S, 0, [c_])] for a, b, c_, _ in words]},
        "cnf": {"k_group": [[(M, ANY, [a, b]), (M, ANY, [c_, d])] for a, b, c_, d in words],
                "k_conj_flat": [[(M, 0, [a]), (M, 0, [c_])] for a, b, c_, _ in words]},
    }
    was = native.group_clauses(1)
    out = {"bench": "group", "version": native.version(), "docs": args.docs, "queries": args.queries,
           "k": args.k, "steps": args.steps, "warmup": args.warmup}
    try:
        for shape, rows in shapes.items():
            plans = {name: plan(q) for name, q in rows.items()}
            rounds = [{name: timed(p, args.steps, args.warmup) for name, p in plans.items()} for _ in range(2)]
            res = {"rounds_ms": [{n: round(v[0], 4) for n, v in rd.items()} for rd in rounds]}
            for name, p in plans.items():
                res[name + "_ms_per_batch"] = round(min(rd[name][0] for rd in rounds), 4)
                res[name + "_work_items"] = int(p.info().total_chunks)
                res[name + "_hits_per_query_at_k"] = round(float(p.results()[2].mean()), 2)
            out[shape] = res
    finally:
        native.group_clauses(was)
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
