"""Sweep of the one-byte bound tables on one corpus, in one process: the same
batches run against snapshots built under each FUGU_DOCTAB8_DIV, planned under
each FUGU_DOCTAB8_LEAD (the planner reads it when a plan is made), interleaved
round by round (cdna_hip_programming.md §5.4 rule 24: report median and min),
with every variant's output hash checked against the first at every point.

  python tools/ab_doctab8.py [--docs N] [--rounds R] [--steps S] [--divs 0,4,8,16,32] [--leads 0,2,8,32]

A table-less build (DIV 0) plans the same under every LEAD: it runs once.  The
f32 score tables (FUGU_DOCTAB_*) stay at their defaults throughout.
"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--divs", default="0,4,8,16,32")
    ap.add_argument("--leads", default="0,2,8,32")
    ap.add_argument("--workloads", default="and3,mixed,or")
    args = ap.parse_args()
    import numpy as np
    from fugu_amd import native, synth
    ctx = native.Context((0,))
    corp = synth.corpus(args.docs, synth.VOCAB, threads=16)
    divs = [int(x) for x in args.divs.split(",")]
    leads = [int(x) for x in args.leads.split(",")]
    ixs = {}
    for dv in divs:
        os.environ["FUGU_DOCTAB8_DIV"] = str(dv)
        t0 = time.time()
        ix = native.Index.from_docs(ctx, corp.off, corp.tok, synth.VOCAB, threads=16, keep_host=False)
        n_tab, tab_b = ix.bound_tables()
        print(f"[ab] div={dv}: {n_tab} bound tables, {tab_b / 2**30:.3f} GiB of {ix.stats().device_bytes / 2**30:.2f} GiB, "
              f"built in {time.time() - t0:.1f}s", file=sys.stderr, flush=True)
        ixs[dv] = ix
    os.environ.pop("FUGU_DOCTAB8_DIV", None)
    specs = {"and3": (3, 3, 100, native.MODE_AND), "mixed": (1, 5, 100, native.MODE_AND),
             "or": (2, 5, 1000, native.MODE_OR)}
    out = {"docs": args.docs, "divs": divs, "leads": leads, "rounds": args.rounds, "steps": args.steps,
           "tables": {str(dv): ixs[dv].bound_tables() for dv in divs},
           "device_bytes": {str(dv): ixs[dv].stats().device_bytes for dv in divs}, "workloads": {}}
    for wl in args.workloads.split(","):
        m0, m1, k, mode = specs[wl]
        q_off, terms = synth.queries(1024, m0, m1)
        plans = {}
        for dv in divs:
            for ld in (leads if dv else leads[:1]):
                os.environ["FUGU_DOCTAB8_LEAD"] = str(ld)
                plans[f"div{dv}_lead{ld}" if dv else "div0"] = ixs[dv].plan(q_off, terms, k, mode)
        os.environ.pop("FUGU_DOCTAB8_LEAD", None)

        def digest(p):
            s, d, c = p.results()
            h = hashlib.sha1()
            for i in range(len(c)):
                h.update(d[i, :c[i]].tobytes())
                h.update(s[i, :c[i]].tobytes())
            return h.hexdigest()[:16]

        times = {n: [] for n in plans}
        hashes = {n: set() for n in plans}
        for n, p in plans.items():
            p.execute()
            hashes[n].add(digest(p))
        for _ in range(args.rounds):
            for n, p in plans.items():
                p.profile(True)
                for _ in range(args.steps):
                    p.execute()
                ms, cnt = p.kernel_ms()
                times[n].append(ms[0] / cnt)
                hashes[n].add(digest(p))  # (after the timed steps: the read-back is outside them)
        res = {n: {"kernel_ms_med": round(float(np.median(t)), 4), "kernel_ms_min": round(float(np.min(t)), 4),
                   "hash": sorted(hashes[n])} for n, t in times.items()}
        res["identical"] = len(set().union(*hashes.values())) == 1
        out["workloads"][wl] = res
        print(f"[ab] {wl}: {json.dumps(res)}", file=sys.stderr, flush=True)
        del plans
        if not res["identical"]:
            print(json.dumps(out))
            sys.exit(f"[ab] {wl}: output hashes differ")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
