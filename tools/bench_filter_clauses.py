"""k_phrase, k_bphrase and k_group with facet filters (fg_filter_clauses, DESIGN.md
§16) on a 1M-doc synthetic namespace built with positions and facets: 1024
queries, top-100, each shape
  phrase          a two- or three-term phrase cut from a doc
  bphrase_must    `+"phrase" +term`, the term from the same doc (fg_phrase_clauses)
  group_any_term  `+(a b) +c`, the terms from one doc (fg_group_clauses)
planned three times -- unfiltered, with a one-clause filter on about half the
docs, with one on about 1% -- plus the filter's mask alone (the same filter on a
query of missing terms: k_fmask runs, no search kernel has work).  The batch
shares one filter list, so one mask is built per execute.  Device time from HIP
events around the search kernels of every execute (fg_plan_profile; k_fmask
included), warm-up first, the plans of a shape alternating over two rounds: the
spread between the rounds is the noise of the comparison.  Every plan's hits
are asserted identical to a second run's.

  python tools/bench_filter_clauses.py [--docs N] [--queries Q] [--k K] [--steps S] [--warmup W] [--out FILE]

Prints one JSON line and writes it to --out (default profiles/filter_clauses/bench_filter_clauses.json).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.bench_phrase import timed  # noqa: E402

HALF, ONE_PCT = 0, 1  # the facet terms


def hits(plan):
    plan.execute()
    s, d, n = plan.results()
    return [(s[i, :int(n[i])].tobytes(), d[i, :int(n[i])].tobytes()) for i in range(len(n))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filter_clauses", "bench_filter_clauses.json"))
    args = ap.parse_args()
    from fugu_amd import native, synth
    if native.device_count() == 0:
        raise SystemExit("bench_filter_clauses: no GPU visible")
    ctx = native.Context((0,))
    c = synth.corpus(args.docs, threads=16)
    r = np.random.default_rng(17)
    half, pct = r.random(args.docs) < 0.5, r.random(args.docs) < 0.01
    f_cnt = half.astype(np.uint64) + pct
    f_docs = np.zeros(args.docs + 1, np.uint64)
    f_docs[1:] = np.cumsum(f_cnt)
    f_tok = np.zeros(int(f_docs[-1]), np.uint32)
    f_tok[(f_docs[:-1][pct] + half[pct]).astype(np.int64)] = ONE_PCT  # (HALF = 0 comes first in a doc with both)
    ix = native.Index.from_docs(ctx, c.off, c.tok, synth.VOCAB, threads=16, keep_host=False, positions=True,
                                facets=(f_docs, f_tok, 2))
    Q = args.queries
    phrases, same_doc, triples = [], [], []
    while len(phrases) < Q:
        d = int(r.integers(0, args.docs))
        b, e = int(c.off[d]), int(c.off[d + 1])
        m = 2 + len(phrases) % 2
        t = np.unique(c.tok[b:e])
        if e - b >= m + 1 and len(t) >= 3:
            s = int(r.integers(b, e - m + 1))
            phrases.append(c.tok[s:s + m])
            same_doc.append(int(c.tok[int(r.integers(b, e))]))
            triples.append([int(x) for x in r.choice(t, 3, replace=False)])
    M = native.OCCUR_MUST
    cat = lambda rows: np.concatenate([np.asarray(x) for x in rows])  # noqa: E731
    shapes = {
        "phrase": dict(q_off=np.cumsum([0] + [len(q) for q in phrases]), terms=cat(phrases),
                       phrase_len=cat([[len(q)] + [0] * (len(q) - 1) for q in phrases]),
                       phrase_pos=cat([np.arange(len(q)) for q in phrases])),
        "bphrase_must": dict(q_off=np.cumsum([0] + [len(q) + 1 for q in phrases]),
                             terms=cat([np.append(q, t) for q, t in zip(phrases, same_doc)]),
                             phrase_len=cat([[len(q)] + [0] * (len(q) - 1) + [1] for q in phrases]),
                             phrase_pos=cat([np.append(np.arange(len(q)), 0) for q in phrases])),
        "group_any_term": dict(q_off=np.arange(Q + 1) * 3, terms=cat(triples),
                               phrase_len=cat([[2 | native.CLAUSE_ANY, 0, 1]] * Q), phrase_pos=np.zeros(3 * Q)),
    }
    gone = dict(q_off=np.arange(Q + 1) * 2, terms=np.full(2 * Q, native.FG_TERM_MISSING, np.uint32),
                phrase_len=cat([[2, 0]] * Q), phrase_pos=cat([[0, 1]] * Q))

    def plan(sh, fterm):
        kw = dict(phrase_len=sh["phrase_len"].astype(np.uint32), phrase_pos=sh["phrase_pos"].astype(np.uint32))
        if sh is not shapes["phrase"] and sh is not gone:
            kw["occur"] = np.full(len(sh["terms"]), M, np.uint8)
        if fterm is not None:
            kw["f_off"], kw["f_terms"] = np.arange(Q + 1, dtype=np.uint32), np.full(Q, fterm, np.uint32)
        return ix.plan(sh["q_off"].astype(np.uint32), sh["terms"].astype(np.uint32), args.k, **kw)

    was = (native.phrase_clauses(1), native.group_clauses(1), native.filter_clauses(1))
    out = {"bench": "filter_clauses", "version": native.version(), "docs": args.docs, "queries": Q, "k": args.k,
           "steps": args.steps, "warmup": args.warmup,
           "filter_docs": {"half": int(half.sum()), "one_percent": int(pct.sum())}}
    try:
        masks = {"k_fmask_half": plan(gone, HALF), "k_fmask_one_percent": plan(gone, ONE_PCT)}
        rounds = [{name: timed(p, args.steps, args.warmup) for name, p in masks.items()} for _ in range(2)]
        out["k_fmask_alone"] = {"rounds_ms": [{n: round(v[0], 4) for n, v in rd.items()} for rd in rounds]}
        for name in masks:
            out["k_fmask_alone"][name + "_ms_per_batch"] = round(min(rd[name][0] for rd in rounds), 4)
        for shape, sh in shapes.items():
            plans = {"unfiltered": plan(sh, None), "filter_half": plan(sh, HALF), "filter_one_percent": plan(sh, ONE_PCT)}
            for name, p in plans.items():
                assert hits(p) == hits(p), (shape, name)
            rounds = [{name: timed(p, args.steps, args.warmup) for name, p in plans.items()} for _ in range(2)]
            res = {"rounds_ms": [{n: round(v[0], 4) for n, v in rd.items()} for rd in rounds]}
            for name, p in plans.items():
                res[name + "_ms_per_batch"] = round(min(rd[name][0] for rd in rounds), 4)
                res[name + "_work_items"] = int(p.info().total_chunks)
                res[name + "_hits_per_query_at_k"] = round(float(p.results()[2].mean()), 2)
            out[shape] = res
    finally:
        for f, w in zip((native.phrase_clauses, native.group_clauses, native.filter_clauses), was):
            f(w)
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
