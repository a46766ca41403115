"""fg_count_batch with phrase and group clauses (fg_count_clauses) on
tools/bench_count.py's 1M-doc namespace, built with positions: 64 queries x 32
count terms of
  phrase        a two-word phrase alone
  phrase_term   `+"a b" +c`, c from the same doc
  any_term      `+(a b) +c`
  all_or_term   `(a AND b) OR c`
  shared        64 queries `+"a b" +c_i` around ONE phrase (one clause row)
each beside fg_count_batch of the nearest flat query in the same run (`+a +b`,
`+a +b +c`, `+a +c`, `a c`), and `phrase` beside k_phrase on the same phrases at
k = 100.  Device time per kernel from HIP events (fg_count_trace,
fg_count_clause_trace), 20 steps after 5 warm-up.  There is no target: without the
switch these counts do not run on the device at all.

Per workload also k_crow's work per launch: its streamed driver postings (the
rows' driver lists, from the snapshot's doc frequencies), its survivors among the
alive docs (the totals of the rows' conjunctions, counted by fg_count_batch itself)
and a MODEL of its forward-index bytes: survivors x the mean text length x 4 B, an
upper bound -- a wave stops at its first hit and skips a field no longer than the span.

  python tools/bench_count_clauses.py [--docs N] [--steps S] [--warmup W] [--out FILE]

Prints one JSON line and writes it to --out (default profiles/count_clauses/bench_count_clauses.json).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.bench_count import L1, facet_tokens  # noqa: E402
from tools.bench_phrase import timed  # noqa: E402

ANY, ALL = 0x80000000, 0x40000000  # fugu.h FG_CLAUSE_ANY / FG_CLAUSE_ALL


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "count_clauses", "bench_count_clauses.json"))
    args = ap.parse_args()
    from fugu_amd import native, synth
    if native.device_count() == 0:
        raise SystemExit("bench_count_clauses: no GPU visible")
    N, Q = args.docs, args.queries
    corp = synth.corpus(N, threads=16)
    f_off, f_tok, n_ft = facet_tokens(N)
    deleted = (np.random.RandomState(3).random_sample(N) < 0.03).astype(np.uint8)
    ctx = native.Context((0,))
    ix = native.Index.from_docs(ctx, corp.off, corp.tok, synth.VOCAB, deleted=deleted, facets=(f_off, f_tok, n_ft),
                                threads=16, positions=True)
    cts32 = np.concatenate([np.arange(1, 1 + L1), np.arange(1 + L1, 1 + 2 * L1)]).astype(np.uint32)
    mean_len = float(corp.off[-1]) / N
    r = np.random.default_rng(11)

    def span():
        """(a, b, c): two adjacent tokens of a doc and another token of the same doc"""
        while True:
            d = int(r.integers(0, N))
            b, e = int(corp.off[d]), int(corp.off[d + 1])
            if e - b >= 3:
                s = int(r.integers(b, e - 1))
                return int(corp.tok[s]), int(corp.tok[s + 1]), int(corp.tok[int(r.integers(b, e))])

    abc = [span() for _ in range(Q)]
    M, S = native.OCCUR_MUST, native.OCCUR_SHOULD

    def batch(queries):
        """queries: per query a list of (occur, phrase_len entry, terms)"""
        q_off, terms, occur, plen, ppos = [0], [], [], [], []
        for q in queries:
            for oc, first, ts in q:
                terms += ts
                occur += [oc] * len(ts)
                plen += [first] + [0] * (len(ts) - 1)
                ppos += list(range(len(ts))) if first == len(ts) and len(ts) > 1 else [0] * len(ts)
            q_off.append(len(terms))
        u = lambda a: np.array(a, np.uint32)  # noqa: E731
        return dict(q_off=u(q_off), terms=u(terms), occur=np.array(occur, np.uint8), phrase_len=u(plen), phrase_pos=u(ppos))

    T = lambda oc, t: (oc, 1, [t])  # noqa: E731

    def measure(b):
        def once():
            return native.count_batch([ix], b["q_off"], b["terms"], cts32, occur=b["occur"], phrase_len=b["phrase_len"],
                                      phrase_pos=b["phrase_pos"])
        for _ in range(args.warmup):
            once()
        native.count_trace(1)
        native.count_clause_trace(1)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            total, _ = once()
        wall = (time.perf_counter() - t0) * 1e3 / args.steps
        ms, n = native.count_trace(0)
        cms, cn = native.count_clause_trace(0)
        assert n == cn == args.steps
        out = {"wall_ms": round(wall, 4), **{k: round(v / n, 5) for k, v in {**ms, **cms}.items()}}
        out["kernels_ms"] = round(sum(v for k, v in out.items() if k.startswith("k_")), 5)
        out["mean_total"] = round(float(total.mean()), 1)
        return out

    def df(t):
        return int(ix.df(int(t)))

    def row_work(rows):
        """rows: the distinct clause rows as (kind, terms): k_crow's driver postings and survivors per launch"""
        driver = sum(sum(df(t) for t in ts) if kind == "any" else min(df(t) for t in set(ts)) for kind, ts in rows)
        conj = [r_ for r_ in rows if r_[0] != "any"]
        surv = 0
        if conj:
            b = batch([[T(M, t) for t in dict.fromkeys(ts)] for _, ts in conj])
            surv = int(native.count_batch([ix], b["q_off"], b["terms"], occur=b["occur"])[0].sum())
        phrases = [r_ for r_ in rows if r_[0] == "phrase"]
        psurv = 0
        if phrases:
            b = batch([[T(M, t) for t in dict.fromkeys(ts)] for _, ts in phrases])
            psurv = int(native.count_batch([ix], b["q_off"], b["terms"], occur=b["occur"])[0].sum())
        return {"rows": len(rows), "driver_postings": int(driver), "survivors_alive": surv,
                "fwd_bytes_model": int(psurv * mean_len * 4)}

    a0, b0, _ = abc[0]
    workloads = {
        "phrase": ([[(S, 2, [a, b])] for a, b, _ in abc], [[T(M, a), T(M, b)] for a, b, _ in abc],
                   [("phrase", [a, b]) for a, b, _ in abc]),
        "phrase_term": ([[(M, 2, [a, b]), T(M, c)] for a, b, c in abc], [[T(M, a), T(M, b), T(M, c)] for a, b, c in abc],
                        [("phrase", [a, b]) for a, b, _ in abc]),
        "any_term": ([[(M, 2 | ANY, [a, b]), T(M, c)] for a, b, c in abc], [[T(M, a), T(M, c)] for a, _, c in abc],
                     [("any", [a, b]) for a, b, _ in abc]),
        "all_or_term": ([[(S, 2 | ALL, [a, b]), T(S, c)] for a, b, c in abc], [[T(S, a), T(S, c)] for a, _, c in abc],
                        [("all", [a, b]) for a, b, _ in abc]),
        "shared": ([[(M, 2, [a0, b0]), T(M, c)] for _, _, c in abc], [[T(M, a0), T(M, b0), T(M, c)] for _, _, c in abc],
                   [("phrase", [a0, b0])]),
    }
    out = {"bench": "count_clauses", "version": native.version(), "docs": N, "queries": Q, "count_terms": len(cts32),
           "steps": args.steps, "warmup": args.warmup, "mean_text_len": round(mean_len, 2)}
    was = native.count_clauses(1)
    try:
        for name, (clause_q, flat_q, rows) in workloads.items():
            distinct = list({(k, tuple(ts)): (k, ts) for k, ts in rows}.values())
            res = {"clauses": measure(batch(clause_q)), "flat": measure(batch(flat_q)), "k_crow_work": row_work(distinct)}
            if name == "phrase":
                b = batch(clause_q)
                plan = ix.plan(b["q_off"], b["terms"], 100, phrase_len=b["phrase_len"], phrase_pos=b["phrase_pos"])
                res["k_phrase_k100_ms"] = round(timed(plan, args.steps, args.warmup)[0], 5)
                plan.close()
            out[name] = res
    finally:
        native.count_clauses(was)
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
