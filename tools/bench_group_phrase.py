"""k_gphrase (a group clause beside a phrase clause, fg_group_phrase_clauses) next
to the two kernels it is composed from, on a 1M-doc synthetic namespace built
with positions: 1024 queries, top-100, the phrase a span of 2 or 3 tokens of a
document, the group two other terms of the same document --
  must_must    `+phrase +(a b)`
  should       `phrase (a b)`      all Should
  group_first  `+(a b) phrase`     every Must an any-of group; the phrase only adds score
each beside the same phrase with the group replaced by its first member (k_bphrase,
fg_phrase_clauses) and the same group with the phrase replaced by its rarest term
(k_group).  Device time from HIP events around the search kernels of every
execute (fg_plan_profile), warm-up first, the plans of a shape alternating over
two rounds: the spread between the rounds is the noise of the comparison.  There
is no target: without the switch these queries do not run on the device at all,
and the neighbours are different queries.

  python tools/bench_group_phrase.py [--docs N] [--queries Q] [--k K] [--steps S] [--warmup W] [--out FILE]

Prints one JSON line and writes it to --out (default profiles/group_phrase/bench_group_phrase.json).
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_phrase", "bench_group_phrase.json"))
    args = ap.parse_args()
    from fugu_amd import native, synth
    if native.device_count() == 0:
        raise SystemExit("bench_group_phrase: no GPU visible")
    ctx = native.Context((0,))
    c = synth.corpus(args.docs, threads=16)
    ix = native.Index.from_docs(ctx, c.off, c.tok, synth.VOCAB, threads=16, keep_host=False, positions=True)
    r = np.random.default_rng(17)

    def draw(m):  # a span of m tokens of a document, two other distinct terms of it, the span's rarest term
        while True:
            d = int(r.integers(0, args.docs))
            b, e = int(c.off[d]), int(c.off[d + 1])
            if e - b < m + 2:
                continue
            s = int(r.integers(b, e - m + 1))
            ph = [int(x) for x in c.tok[s:s + m]]
            rest = np.setdiff1d(c.tok[b:e], ph)
            if len(rest) >= 2:
                a, g = (int(x) for x in r.choice(rest, 2, replace=False))
                return ph, a, g, min(ph, key=ix.df)

    words = [draw(2 + i % 2) for i in range(args.queries)]
    S, M = native.OCCUR_SHOULD, native.OCCUR_MUST
    ANY = native.CLAUSE_ANY

    def plan(rows):
        """rows: per query [(occur, "p" | "g" | "t", [terms])]"""
        q_off = np.cumsum([0] + [sum(len(t) for _, _, t in q) for q in rows]).astype(np.uint32)
        terms = np.array([x for q in rows for _, _, t in q for x in t], np.uint32)
        occur = np.array([oc for q in rows for oc, _, t in q for _ in t], np.uint8)
        plen = np.array([(len(t) | (ANY if kd == "g" else 0)) if j == 0 else 0 for q in rows for _, kd, t in q
                         for j in range(len(t))], np.uint32)
        ppos = np.array([j if kd == "p" else 0 for q in rows for _, kd, t in q for j in range(len(t))], np.uint32)
        return ix.plan(q_off, terms, args.k, occur=occur, phrase_len=plen, phrase_pos=ppos)

    def shape(op, og, group_first):
        new = [[(op, "p", ph), (og, "g", [a, g])][::-1 if group_first else 1] for ph, a, g, _ in words]
        return {"k_gphrase": new,
                "k_bphrase_first_member": [[(op, "p", ph), (og, "t", [a])][::-1 if group_first else 1] for ph, a, g, _ in words],
                "k_group_rarest_term": [[(op, "t", [t]), (og, "g", [a, g])][::-1 if group_first else 1] for ph, a, g, t in words]}

    shapes = {"must_must": shape(M, M, False), "should": shape(S, S, False), "group_first": shape(S, M, True)}
    fns = (native.group_clauses, native.group_phrase_clauses, native.phrase_clauses)
    was = [f(1) for f in fns]
    out = {"bench": "group_phrase", "version": native.version(), "docs": args.docs, "queries": args.queries,
           "k": args.k, "steps": args.steps, "warmup": args.warmup}
    try:
        for name, rows in shapes.items():
            plans = {kernel: plan(q) for kernel, q in rows.items()}
            rounds = [{kernel: timed(p, args.steps, args.warmup) for kernel, p in plans.items()} for _ in range(2)]
            res = {"rounds_ms": [{n: round(v[0], 4) for n, v in rd.items()} for rd in rounds]}
            for kernel, p in plans.items():
                res[kernel + "_ms_per_batch"] = round(min(rd[kernel][0] for rd in rounds), 4)
                res[kernel + "_work_items"] = int(p.info().total_chunks)
                res[kernel + "_hits_per_query_at_k"] = round(float(p.results()[2].mean()), 2)
            out[name] = res
            for p in plans.values():
                p.close()
    finally:
        for f, w in zip(fns, was):
            f(w)
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
