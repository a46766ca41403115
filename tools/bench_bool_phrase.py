"""k_bphrase (a phrase clause beside a term clause, fg_phrase_clauses) next to the
kernels that bracket it, on a 1M-doc synthetic namespace built with positions:
1024 queries, top-100, two shapes --
  should  `phrase term`, both Should: the default parse of `e-mail server`;
  must    `+phrase +term`
-- each beside (1) k_phrase on the same phrases alone and (2) the same terms as
plain term clauses (k_disj for the Should shape, k_conj for the Must one).
Device time from HIP events around the search kernels of every execute
(fg_plan_profile), warm-up first, the three plans of a shape alternating over two
rounds: the spread between the rounds is the noise of the comparison.  There is
no target: without the switch these queries do not run on the device at all.

  python tools/bench_bool_phrase.py [--docs N] [--queries Q] [--k K] [--steps S] [--warmup W] [--out FILE]

Prints one JSON line and writes it to --out (default profiles/bool_phrase/bench_bool_phrase.json).
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bool_phrase", "bench_bool_phrase.json"))
    args = ap.parse_args()
    from fugu_amd import native, synth
    if native.device_count() == 0:
        raise SystemExit("bench_bool_phrase: no GPU visible")
    ctx = native.Context((0,))
    c = synth.corpus(args.docs, threads=16)
    ix = native.Index.from_docs(ctx, c.off, c.tok, synth.VOCAB, threads=16, keep_host=False, positions=True)
    r = np.random.default_rng(11)

    def span(m):
        while True:
            d = int(r.integers(0, args.docs))
            b, e = int(c.off[d]), int(c.off[d + 1])
            if e - b >= m + 1:
                s = int(r.integers(b, e - m + 1))
                return c.tok[s:s + m], c.tok[b:e]

    phrases, same_doc, other_doc = [], [], []
    for i in range(args.queries):
        ph, doc = span(2 + i % 2)
        phrases.append(ph)
        same_doc.append(int(doc[int(r.integers(0, len(doc)))]))
        other_doc.append(int(span(2)[1][0]))
    S, M = native.OCCUR_SHOULD, native.OCCUR_MUST
    was = native.phrase_clauses(1)
    out = {"bench": "bool_phrase", "version": native.version(), "docs": args.docs, "queries": args.queries,
           "k": args.k, "steps": args.steps, "warmup": args.warmup}
    try:
        p_off = np.cumsum([0] + [len(q) for q in phrases]).astype(np.uint32)
        p_terms = np.concatenate(phrases).astype(np.uint32)
        p_len = np.concatenate([[len(q)] + [0] * (len(q) - 1) for q in phrases]).astype(np.uint32)
        p_pos = np.concatenate([np.arange(len(q)) for q in phrases]).astype(np.uint32)
        for shape, oc, extra in (("should", S, other_doc), ("must", M, same_doc)):
            q_off = np.cumsum([0] + [len(q) + 1 for q in phrases]).astype(np.uint32)
            terms = np.concatenate([np.append(q, t) for q, t in zip(phrases, extra)]).astype(np.uint32)
            plen = np.concatenate([[len(q)] + [0] * (len(q) - 1) + [1] for q in phrases]).astype(np.uint32)
            ppos = np.concatenate([np.append(np.arange(len(q)), 0) for q in phrases]).astype(np.uint32)
            occur = np.full(len(terms), oc, np.uint8)
            plans = {
                "k_bphrase": ix.plan(q_off, terms, args.k, occur=occur, phrase_len=plen, phrase_pos=ppos),
                "k_phrase_alone": ix.plan(p_off, p_terms, args.k, phrase_len=p_len, phrase_pos=p_pos),
                ("k_disj_terms" if oc == S else "k_conj_terms"): ix.plan(q_off, terms, args.k, occur=occur),
            }
            rounds = [{name: timed(p, args.steps, args.warmup) for name, p in plans.items()} for _ in range(2)]
            res = {"rounds_ms": [{n: round(v[0], 4) for n, v in rd.items()} for rd in rounds]}
            for name, p in plans.items():
                res[name + "_ms_per_batch"] = round(min(rd[name][0] for rd in rounds), 4)
                res[name + "_work_items"] = int(p.info().total_chunks)
                res[name + "_hits_per_query_at_k"] = round(float(p.results()[2].mean()), 2)
            out[shape] = res
    finally:
        native.phrase_clauses(was)
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
