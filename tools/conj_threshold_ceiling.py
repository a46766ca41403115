"""The most any threshold work can give k_conj: the headline batch (1024 3-term
ANDs, k = 100, 10M docs) from plans that START at each query's final k-th score
against the same plans as planned, interleaved in one process on one index.

  python tools/conj_threshold_ceiling.py [--also VAR=V[,VAR=V] ...] [--out FILE]

The batch runs once, each query's final k-th score (0 for fewer than k hits) is
seeded into a fresh plan as its starting threshold (fg_plan_seed_thr0: the
lowest key with that score; the bins stay as planned), and both plans are timed
with tools/ab_env.py's interleaved rounds; the output hashes must be equal.
`--also` repeats the pair under planner settings (e.g. FUGU_CONJ_HIST_THR=0),
so a setting's gain and its distance from the ceiling come from one run.
"ratio" is k_conj ms seeded / unseeded; "clears_bar" says whether the seeded
plan is faster by at least 3 x the unseeded plan's round-to-round spread.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--also", nargs="*", default=[], metavar="VAR=V[,VAR=V]")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    from ab_env import time_plans
    from fugu_amd import native, synth
    ctx = native.Context((0,))
    corp = synth.corpus(args.docs, threads=16)
    ix = native.Index.from_docs(ctx, corp.off, corp.tok, synth.VOCAB, threads=16, keep_host=False)
    q_off, terms = synth.queries(args.batch, 3, 3)
    k = args.k
    s, d, n = ix.search_batch(q_off, terms, k)
    kth = np.where(n == k, s[:, k - 1], np.float32(0.0)).astype(np.float32)
    plans = {}
    for name in ["default"] + list(args.also):
        env = dict(kv.split("=", 1) for kv in name.split(",")) if name != "default" else {}
        old = {v: os.environ.get(v) for v in env}
        os.environ.update(env)
        plans[name] = ix.plan(q_off, terms, k)
        plans[name + "+seed"] = ix.plan(q_off, terms, k)
        plans[name + "+seed"].seed_thresholds(kth)
        for v, x in old.items():
            if x is None:
                del os.environ[v]
            else:
                os.environ[v] = x
    res = time_plans(plans, args.rounds, args.steps)
    out = {"docs": args.docs, "batch": args.batch, "k": k, "rounds": args.rounds, "steps": args.steps,
           "queries_with_k_hits": int((n == k).sum()), "lib": native.version(), "plans": res,
           "identical": len({r["hash"] for r in res.values()}) == 1, "ceiling": {}}
    for name in ["default"] + list(args.also):
        a, b = res[name], res[name + "+seed"]
        out["ceiling"][name] = {"k_conj_ms": a["ms_med"], "k_conj_ms_seeded": b["ms_med"],
                                "ratio": round(b["ms_med"] / a["ms_med"], 4), "round_spread": a["round_spread"],
                                "clears_bar": a["ms_med"] - b["ms_med"] >= 3 * a["round_spread"],
                                "k_final_ms": a["final_ms_med"], "k_final_ms_seeded": b["final_ms_med"]}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
