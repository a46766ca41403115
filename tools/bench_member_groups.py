"""k_mgroup (phrases as group members, fg_group_member_phrases) next to its two
neighbours, on a 1M-doc synthetic namespace built with positions: 1024 queries,
top-100, P a span of 2 or 3 tokens of a document, t and u two other terms of the
same document --
  must    `+(P | t) +u`
  should  `(P | t) u`      all Should
  all     `(P & t) u`      all Should, the group all-of
each beside the same table with P cut down to its rarest term (k_group) and the
group cut down to its first member, P (k_bphrase, fg_phrase_clauses).  Device time
from HIP events around the search kernels of every execute (fg_plan_profile),
warm-up first, the plans of a shape alternating over two rounds: the spread between
the rounds is the noise of the comparison.  There is no target: without the switch
these queries do not run on the device at all, and the neighbours are different
queries.

  python tools/bench_member_groups.py [--docs N] [--queries Q] [--k K] [--steps S] [--warmup W] [--out FILE]

Prints one JSON line and writes it to --out (default profiles/member_groups/bench_member_groups.json).
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "member_groups", "bench_member_groups.json"))
    args = ap.parse_args()
    from fugu_amd import native, synth
    if native.device_count() == 0:
        raise SystemExit("bench_member_groups: no GPU visible")
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
    FLAG = {"any": native.CLAUSE_ANY, "all": native.CLAUSE_ALL}

    def plan(rows):
        """rows: per query [(occur, "any" | "all" | "p" | "t", [members])], a member a term or a list of terms (a phrase)"""
        q_off, terms, occur, plen, ppos = [0], [], [], [], []
        for q in rows:
            for oc, kd, mem in q:
                flat = [(x, j) for m in mem for j, x in enumerate(m if isinstance(m, list) else [m])]
                if kd == "p":
                    flat = [(x, j) for j, x in enumerate(mem)]
                terms += [x for x, _ in flat]
                ppos += [j for _, j in flat]
                occur += [oc] * len(flat)
                plen += [len(flat) | FLAG.get(kd, 0)] + [0] * (len(flat) - 1)
            q_off.append(len(terms))
        return ix.plan(np.array(q_off, np.uint32), np.array(terms, np.uint32), args.k, occur=np.array(occur, np.uint8),
                       phrase_len=np.array(plen, np.uint32), phrase_pos=np.array(ppos, np.uint32))

    def shape(og, ou, kind):
        return {"k_mgroup": [[(og, kind, [ph, a]), (ou, "t", [g])] for ph, a, g, _ in words],
                "k_group_rarest_term": [[(og, kind, [t, a]), (ou, "t", [g])] for ph, a, g, t in words],
                "k_bphrase_first_member": [[(og, "p", ph), (ou, "t", [g])] for ph, a, g, _ in words]}

    shapes = {"must": shape(M, M, "any"), "should": shape(S, S, "any"), "all": shape(S, S, "all")}
    fns = (native.group_clauses, native.group_member_phrases, native.phrase_clauses)
    was = [f(1) for f in fns]
    out = {"bench": "member_groups", "version": native.version(), "docs": args.docs, "queries": args.queries,
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
