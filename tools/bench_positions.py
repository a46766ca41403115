"""The forward index built on the device from positional postings
(fg_index_build_positional) against the two paths beside it, on the
1M-doc synthetic namespace tools/bench_phrase.py uses (63.9M positions), inverted
once on the host outside the timed region:

  (a) fg_index_build_global            the postings without positions (unchanged path);
  (b) fg_index_build_positional        the same postings + their positions;
  (c) fg_index_build_from_docs_global  the token streams with keep_positions.

Wall time of 5 builds each after 1 warm-up, alternating; then one build of (b) and
(c) under FUGU_BUILD_TRACE for (b)'s HIP-event times per kernel and its upload, and
(c)'s host "forward index" phase.  The bytes each kernel must move are counted
from the corpus and set against 8 TB/s.

  python tools/bench_positions.py [--docs N] [--builds B] [--out FILE]

Prints one JSON line and writes it to --out (default profiles/positions/bench_positions.json).
"""
import argparse
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 8e12


def fieldnorm_ids(lens):
    """tantivy fieldnorm/code.rs: the id of each length (0..40, then 8 values per doubling step)"""
    t = list(range(41))
    x, step = 40, 2
    while len(t) < 256:
        for _ in range(8):
            if len(t) == 256:
                break
            x += step
            t.append(x)
        step *= 2
    return (np.searchsorted(np.array(t, np.uint64), lens, side="right") - 1).astype(np.uint8)


def invert(off, tok, n_terms):
    """positional postings of one field's token streams (no gaps): term_off, doc, tf, positions in posting order"""
    n = len(off) - 1
    lens = np.diff(off.astype(np.int64))
    owner = np.repeat(np.arange(n, dtype=np.uint32), lens)
    pos = (np.arange(len(tok), dtype=np.int64) - np.repeat(off[:-1].astype(np.int64), lens)).astype(np.uint32)
    order = np.argsort(tok, kind="stable")  # the tokens are in (doc, position) order already
    term, doc_e, pos = tok[order], owner[order], pos[order]
    first = np.ones(len(term), bool)
    first[1:] = (term[1:] != term[:-1]) | (doc_e[1:] != doc_e[:-1])
    at = np.nonzero(first)[0]
    tf = np.diff(np.append(at, len(term)))
    assert tf.max() <= 0xFFFF
    term_off = np.searchsorted(term[at], np.arange(n_terms + 1)).astype(np.uint64)
    return term_off, doc_e[at], tf.astype(np.uint16), pos, lens


def traced(build):
    """(the build's result, its FUGU_BUILD_TRACE lines) -- stderr redirected to a file for the call"""
    os.environ["FUGU_BUILD_TRACE"] = "1"
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        try:
            out = build()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            del os.environ["FUGU_BUILD_TRACE"]
        f.seek(0)
        lines = [x for x in f.read().decode(errors="replace").splitlines() if x.startswith("[fg build]")]
    return out, lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--builds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "positions", "bench_positions.json"))
    args = ap.parse_args()
    from fugu_amd import native, synth
    if native.device_count() == 0:
        raise SystemExit("bench_positions: no GPU visible")
    ctx = native.Context((0,))
    c = synth.corpus(args.docs, threads=16)
    V = synth.VOCAB
    t0 = time.perf_counter()
    term_off, doc, tf, pos, lens = invert(c.off, c.tok, V)
    invert_s = time.perf_counter() - t0
    fn = fieldnorm_ids(lens.astype(np.uint64))
    post = (args.docs, term_off, doc, tf, None, fn, None, (int(lens.sum()), 0))
    g = native.docs_stats(c.off, c.tok, V, threads=16)

    builds = {
        "a_postings": lambda: native.Index.from_postings(ctx, *post, global_stats=g),
        "b_positional": lambda: native.Index.from_postings(ctx, *post, global_stats=g, positions=(pos, None)),
        "c_token_streams": lambda: native.Index.from_docs(ctx, c.off, c.tok, V, threads=16, keep_host=False, global_stats=g,
                                                          positions=True),
    }
    wall = {k: [] for k in builds}
    for r in range(args.builds + 1):  # round 0 warms up
        for k, f in builds.items():
            t0 = time.perf_counter()
            ix = f()
            dt = (time.perf_counter() - t0) * 1e3
            if r:
                wall[k].append(round(dt, 1))
            ix.close()
    ixb, lines_b = traced(builds["b_positional"])
    ixc, lines_c = traced(builds["c_token_streams"])
    # the two forward indexes are the same array
    a, b = ixb.positions(0, 0, 1000), ixc.positions(0, 0, 1000)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    rows = int(lens.sum())  # (no gaps: a row entry per token)
    kern = {}
    for ln in lines_b:
        m = re.search(r"forward index \(text\): .* ms: (.*)$", ln)
        if m:
            kern = {k: float(v) for k, v in re.findall(r"(\w+) ([0-9.]+)", m.group(1))}

    def phase(lines, name):
        for ln in lines:
            m = re.match(r"\[fg build\] " + re.escape(name) + r"\s+([0-9.]+) ms", ln)
            if m:
                return float(m.group(1))
        return None

    P, n_pos, N = len(doc), len(pos), args.docs
    # the bytes each step must move at least (reads + writes), and the share of 8 TB/s its time is
    must = {
        "scan_tf": 2 * P * 2 + 8 * P,             # tf read by the reduce and the prefix pass, the offsets written
        "k_fwd_len": 2 * P + 8 * P + 4 * P + 4 * P + 4 * P,  # tf, offset, last position, doc, one atomic word per posting
        "scan_len": 2 * 4 * N + 8 * N,
        "k_fwd_fill": 4 * rows,
        "k_fwd_scatter": 2 * P + 4 * P + 8 * P + 16 * P + 4 * n_pos + 4 * n_pos,  # tf, doc, offset, row bounds; positions read, entries written
        "k_fwd_check": 4 * rows,
    }
    med = {k: float(np.median(v)) for k, v in wall.items()}
    out = {
        "bench": "positions", "version": native.version(), "docs": N, "postings": P, "positions": n_pos,
        "forward_rows": rows, "builds": args.builds, "host_inversion_s_untimed": round(invert_s, 1),
        "wall_ms": wall, "wall_ms_median": med,
        "positions_cost_ms_b_minus_a": round(med["b_positional"] - med["a_postings"], 1),
        "token_stream_cost_ms_c_forward_index_phase": phase(lines_c, "forward index"),
        "b_forward_index_phase_ms": phase(lines_b, "forward index (device)"),
        "b_event_ms": kern,
        "upload_bytes": 2 * P + 4 * n_pos,
        "upload_gb_per_s": round((2 * P + 4 * n_pos) / 1e9 / (kern["upload"] / 1e3), 2) if kern.get("upload") else None,
        "must_move_bytes": must,
        "fraction_of_8TBps": {k: round(must[k] / (kern[k] / 1e3) / HBM_BYTES_PER_S, 4) for k in must if kern.get(k)},
    }
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
