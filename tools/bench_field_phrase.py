"""k_fphrase (field-qualified phrase clauses, fg_field_phrases on top of
fg_field_clauses) next to the same phrases unqualified, which the library runs
today on k_phrase / k_bphrase, on a 1M-doc synthetic namespace built with positions
whose docs carry a `name` of their first three text tokens: 1024 queries, top-100,
three shapes over spans cut from one document each (so every query has a hit) --
  name_phrase       `name:"a b"`      beside `"a b"`      (k_phrase), a b cut from a name
  text_phrase       `text:"a b"`      beside `"a b"`      (k_phrase), a b cut from a text
  must_name_phrase  `+name:"a b" +c`  beside `+"a b" +c`  (k_bphrase, fg_phrase_clauses)
Device time from HIP events around the search kernels of every execute
(fg_plan_profile), warm-up first, the plans of a shape alternating over two
rounds: the spread between the rounds is the noise of the comparison.  There is
no target: without the switch these queries do not run on the device at all, and
the unqualified neighbours are different queries (more hits, other scores); they
are context only.

  python tools/bench_field_phrase.py [--docs N] [--queries Q] [--k K] [--steps S] [--warmup W] [--out FILE]

Prints one JSON line and writes it to --out (default profiles/field_phrase/bench_field_phrase.json).
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_phrase", "bench_field_phrase.json"))
    args = ap.parse_args()
    from fugu_amd import native, synth
    if native.device_count() == 0:
        raise SystemExit("bench_field_phrase: no GPU visible")
    ctx = native.Context((0,))
    c = synth.corpus(args.docs, threads=16)
    assert synth.LEN_MIN >= NAME_LEN
    name_off = (np.arange(args.docs + 1, dtype=np.uint64) * NAME_LEN)
    name_tok = c.tok[(c.off[:-1, None] + np.arange(NAME_LEN, dtype=np.uint64)[None, :]).ravel().astype(np.int64)]
    ix = native.Index.from_docs(ctx, c.off, c.tok, synth.VOCAB, name_off, name_tok, positions=True, threads=16,
                                keep_host=False)
    r = np.random.default_rng(19)

    def spans():  # (a name's two-term span, a text's two-term span, another text term) of one document
        while True:
            d = int(r.integers(0, args.docs))
            row = c.tok[int(c.off[d]):int(c.off[d + 1])]
            s = int(r.integers(0, NAME_LEN - 1))
            nm = [int(row[s]), int(row[s + 1])]
            s = int(r.integers(0, len(row) - 1))
            tx = [int(row[s]), int(row[s + 1])]
            rest = np.unique(row[(row != nm[0]) & (row != nm[1])])
            if len(rest):
                return nm, tx, int(r.choice(rest))

    words = [spans() for _ in range(args.queries)]
    M = native.OCCUR_MUST
    TEXT, NAME = native.CLAUSE_TEXT, native.CLAUSE_NAME

    def plan(rows):
        """rows: per query [(occur, flag or 0, [term, ...])]"""
        q_off = np.cumsum([0] + [sum(len(t) for _, _, t in q) for q in rows]).astype(np.uint32)
        terms = np.array([x for q in rows for _, _, t in q for x in t], np.uint32)
        occur = np.array([oc for q in rows for oc, _, t in q for _ in t], np.uint8)
        plen = np.array([(len(t) | fl) if j == 0 else 0 for q in rows for _, fl, t in q for j in range(len(t))], np.uint32)
        ppos = np.array([j for q in rows for _, _, t in q for j in range(len(t))], np.uint32)
        return ix.plan(q_off, terms, args.k, occur=occur, phrase_len=plen, phrase_pos=ppos)

    shapes = {
        "name_phrase": {"k_fphrase": [[(M, NAME, nm)] for nm, _, _ in words],
                        "unqualified": [[(M, 0, nm)] for nm, _, _ in words]},
        "text_phrase": {"k_fphrase": [[(M, TEXT, tx)] for _, tx, _ in words],
                        "unqualified": [[(M, 0, tx)] for _, tx, _ in words]},
        "must_name_phrase": {"k_fphrase": [[(M, NAME, nm), (M, 0, [t])] for nm, _, t in words],
                             "unqualified": [[(M, 0, nm), (M, 0, [t])] for nm, _, t in words]},
    }
    was = [native.field_clauses(1), native.field_phrases(1), native.phrase_clauses(1)]
    out = {"bench": "field_phrase", "version": native.version(), "docs": args.docs, "queries": args.queries,
           "k": args.k, "steps": args.steps, "warmup": args.warmup, "name_tokens_per_doc": NAME_LEN,
           "unqualified_kernels": {"name_phrase": "k_phrase", "text_phrase": "k_phrase", "must_name_phrase": "k_bphrase"}}
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
        native.field_clauses(was[0])
        native.field_phrases(was[1])
        native.phrase_clauses(was[2])
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
