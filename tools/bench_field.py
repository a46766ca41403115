"""k_field (field-qualified term clauses, fg_field_clauses) next to the same queries
with the fields stripped, which the library runs without the switch, on a 1M-doc
synthetic namespace whose docs carry a `name` of their first three text tokens:
1024 queries, top-100, three shapes over terms drawn from one document each (a
from its name, b from its text, so conjunctions have hits) --
  name_term       `name:a`           beside `a`      (k_conj, single list)
  must_name_text  `+name:a +text:b`  beside `+a +b`  (k_conj)
  must_name_term  `+name:a +b`       beside `+a +b`  (k_conj)
Device time from HIP events around the search kernels of every execute
(fg_plan_profile), warm-up first, the plans of a shape alternating over two
rounds: the spread between the rounds is the noise of the comparison.  There is
no target: without the switch these queries do not run on the device at all, and
the stripped neighbours are different queries (more hits, other scores); they are
context only.

  python tools/bench_field.py [--docs N] [--queries Q] [--k K] [--steps S] [--warmup W] [--out FILE]

Prints one JSON line and writes it to --out (default profiles/field/bench_field.json).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.bench_phrase import timed  # noqa: E402

NAME_LEN = 3  # a doc's name: its first three text tokens (every doc has at least synth.LEN_MIN)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field", "bench_field.json"))
    args = ap.parse_args()
    from fugu_amd import native, synth
    if native.device_count() == 0:
        raise SystemExit("bench_field: no GPU visible")
    ctx = native.Context((0,))
    c = synth.corpus(args.docs, threads=16)
    assert synth.LEN_MIN >= NAME_LEN
    name_off = (np.arange(args.docs + 1, dtype=np.uint64) * NAME_LEN)
    name_tok = c.tok[(c.off[:-1, None] + np.arange(NAME_LEN, dtype=np.uint64)[None, :]).ravel().astype(np.int64)]
    ix = native.Index.from_docs(ctx, c.off, c.tok, synth.VOCAB, name_off, name_tok, threads=16, keep_host=False)
    r = np.random.default_rng(17)

    def pair():  # a name term and another text term of one document
        while True:
            d = int(r.integers(0, args.docs))
            row = c.tok[int(c.off[d]):int(c.off[d + 1])]
            a = int(row[int(r.integers(0, NAME_LEN))])
            rest = np.unique(row[row != a])
            if len(rest):
                return a, int(r.choice(rest))

    words = [pair() for _ in range(args.queries)]
    M = native.OCCUR_MUST
    TEXT, NAME = native.CLAUSE_TEXT, native.CLAUSE_NAME

    def plan(rows):
        """rows: per query [(occur, flag or 0, term)]"""
        q_off = np.cumsum([0] + [len(q) for q in rows]).astype(np.uint32)
        terms = np.array([t for q in rows for _, _, t in q], np.uint32)
        occur = np.array([oc for q in rows for oc, _, _ in q], np.uint8)
        if not any(fl for q in rows for _, fl, _ in q):
            return ix.plan(q_off, terms, args.k, occur=occur)
        plen = np.array([1 | fl for q in rows for _, fl, _ in q], np.uint32)
        return ix.plan(q_off, terms, args.k, occur=occur, phrase_len=plen, phrase_pos=np.zeros(len(terms), np.uint32))

    shapes = {
        "name_term": {"k_field": [[(M, NAME, a)] for a, _ in words],
                      "k_conj_stripped": [[(M, 0, a)] for a, _ in words]},
        "must_name_text": {"k_field": [[(M, NAME, a), (M, TEXT, b)] for a, b in words],
                           "k_conj_stripped": [[(M, 0, a), (M, 0, b)] for a, b in words]},
        "must_name_term": {"k_field": [[(M, NAME, a), (M, 0, b)] for a, b in words],
                           "k_conj_stripped": [[(M, 0, a), (M, 0, b)] for a, b in words]},
    }
    was = native.field_clauses(1)
    out = {"bench": "field", "version": native.version(), "docs": args.docs, "queries": args.queries,
           "k": args.k, "steps": args.steps, "warmup": args.warmup, "name_tokens_per_doc": NAME_LEN}
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
        native.field_clauses(was)
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
