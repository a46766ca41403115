"""k_phrase against its floor: 1024 two- and three-term phrases cut from the docs
of a 1M-doc synthetic namespace built with positions, top-100, and the SAME
terms as a conjunction (k_conj: the candidate generation a phrase cannot do
without) on the same snapshot.  Device time from HIP events around the search
kernels of every execute (fg_plan_profile), summed over the timed steps.

  python tools/bench_phrase.py [--docs N] [--queries Q] [--k K] [--steps S] [--warmup W] [--out FILE]

Prints one JSON line and writes it to --out (default profiles/phrase/bench_phrase.json).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(plan, steps, warmup):
    """(ms per execute of the search kernels, of k_final)"""
    for _ in range(warmup):
        plan.execute()
    plan.results()
    plan.profile(True)
    for _ in range(steps):
        plan.execute()
    plan.results()
    ms, n = plan.kernel_ms()
    plan.profile(False)
    assert n == steps
    return float(ms[0] / n), float(ms[1] / n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "phrase", "bench_phrase.json"))
    args = ap.parse_args()
    from fugu_amd import native, synth
    if native.device_count() == 0:
        raise SystemExit("bench_phrase: no GPU visible")
    ctx = native.Context((0,))
    c = synth.corpus(args.docs, threads=16)
    V = synth.VOCAB
    ix = native.Index.from_docs(ctx, c.off, c.tok, V, threads=16, keep_host=False, positions=True)
    plain = native.Index.from_docs(ctx, c.off, c.tok, V, threads=16, keep_host=False)
    fwd_bytes = ix.stats().device_bytes - plain.stats().device_bytes
    plain.close()
    r = np.random.default_rng(7)
    qs = []
    while len(qs) < args.queries:
        d = int(r.integers(0, args.docs))
        m = 2 + len(qs) % 2
        b, e = int(c.off[d]), int(c.off[d + 1])
        if e - b >= m:
            s = int(r.integers(b, e - m + 1))
            qs.append(c.tok[s:s + m])
    q_off = np.cumsum([0] + [len(q) for q in qs]).astype(np.uint32)
    terms = np.concatenate(qs).astype(np.uint32)
    plen = np.concatenate([[len(q)] + [0] * (len(q) - 1) for q in qs]).astype(np.uint32)
    ppos = np.concatenate([np.arange(len(q)) for q in qs]).astype(np.uint32)
    phrase = ix.plan(q_off, terms, args.k, phrase_len=plen, phrase_pos=ppos)
    conj = ix.plan(q_off, terms, args.k, mode=native.MODE_AND)
    # alternate the two, twice: the spread between the rounds is the noise of the comparison
    rounds = []
    for _ in range(2):
        rounds.append((timed(phrase, args.steps, args.warmup), timed(conj, args.steps, args.warmup)))
    p_ms = min(x[0][0] for x in rounds)
    c_ms = min(x[1][0] for x in rounds)
    # survivors: the docs holding every term of the phrase = the conjunction's hits (no k cut: counted
    # on a plan of its own at the largest k; beyond it the count is a lower bound)
    _, _, n_phrase = phrase.results()
    big = ix.plan(q_off, terms, 1024, mode=native.MODE_AND)
    big.execute()
    _, _, n_conj = big.results()
    out = {
        "bench": "phrase", "version": native.version(), "docs": args.docs, "queries": args.queries, "k": args.k,
        "steps": args.steps, "warmup": args.warmup,
        "k_phrase_ms_per_batch": round(p_ms, 4),
        "k_conj_same_terms_ms_per_batch": round(c_ms, 4),
        "ratio_phrase_over_conj": round(p_ms / c_ms, 3),
        "rounds_ms": [[round(a[0], 4), round(b[0], 4)] for a, b in rounds],
        "k_final_ms": [round(min(x[0][1] for x in rounds), 4), round(min(x[1][1] for x in rounds), 4)],
        "forward_index_bytes": int(fwd_bytes),
        "positions": int(c.off[-1]),
        "phrase_hits_per_query_at_k": round(float(n_phrase.mean()), 2),
        "survivors_per_query_capped_1024": round(float(n_conj.mean()), 2),
        "work_items": [int(phrase.info().total_chunks), int(conj.info().total_chunks)],
    }
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
