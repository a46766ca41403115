"""A/B of planner environment settings on one 10M-doc index in one process:
for each (k, setting) a fresh plan of the same OR batch, timed interleaved over
rounds with HIP events (median / min), results hashed to check they agree.

  python tools/ab_env.py VAR v1 v2 ... [--k 20 1000] [--rounds 5] [--mode or|and]

time_plans / results_hash are the timing and hashing other tools share
(tools/conj_threshold_ceiling.py).
"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def results_hash(plan):
    s, d, n = plan.results()
    h = hashlib.sha1()
    for i in range(len(n)):
        h.update(d[i, :n[i]].tobytes())
        h.update(s[i, :n[i]].tobytes())
    return h.hexdigest()[:16]


def time_plans(plans, rounds, steps):
    """{name: plan} timed interleaved: `rounds` rounds of `steps` executes of each
    plan in turn.  Per name: the first kernel's (k_conj / k_disj) median and min
    over all steps, the medians of the rounds and their spread (max - min), the
    final select's median, and the result hash."""
    import numpy as np
    for p in plans.values():
        p.profile(True)
        for _ in range(2):
            p.execute()
        p.kernel_ms()
    t = {v: [[] for _ in range(rounds)] for v in plans}
    tf = {v: [] for v in plans}
    for r in range(rounds):
        for v, p in plans.items():
            for _ in range(steps):
                p.execute()
                ms, n = p.kernel_ms()
                t[v][r].append(float(ms[0]))
                tf[v].append(float(ms[1]))
    res = {}
    for v, p in plans.items():
        allt = [x for r in t[v] for x in r]
        rm = [float(np.median(r)) for r in t[v]]
        res[v] = {"ms_med": round(float(np.median(allt)), 4), "ms_min": round(float(np.min(allt)), 4),
                  "round_med": [round(x, 4) for x in rm], "round_spread": round(max(rm) - min(rm), 4),
                  "final_ms_med": round(float(np.median(tf[v])), 4), "hash": results_hash(p)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("var")
    ap.add_argument("values", nargs="+")
    ap.add_argument("--k", type=int, nargs="+", default=[20, 1000])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--mode", choices=["or", "and"], default="or")
    args = ap.parse_args()
    from fugu_amd import native, synth
    ctx = native.Context((0,))
    corp = synth.corpus(args.docs, threads=16)
    ix = native.Index.from_docs(ctx, corp.off, corp.tok, synth.VOCAB, threads=16, keep_host=False)
    mode = native.MODE_OR if args.mode == "or" else native.MODE_AND
    q_off, terms = synth.queries(1024, 2, 5) if mode == native.MODE_OR else synth.queries(1024, 3, 3)
    out = {}
    for k in args.k:
        plans = {}
        for v in args.values:
            os.environ[args.var] = v
            plans[v] = ix.plan(q_off, terms, k, mode)
        res = time_plans(plans, args.rounds, args.steps)
        res["identical"] = len({r["hash"] for r in res.values()}) == 1
        out[f"k{k}"] = res
        print(f"[ab_env] {args.var} k={k}: {json.dumps(res)}", file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
