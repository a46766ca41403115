"""The corpora and queries of test_bool_ref.py (CPU) and test_gpu_clause_edges.py:
6-16 clause queries on the edges of the ranges k_disj and k_conj read.  One
function builds each case, so both tests see the same inputs; the expected
results come from bool_ref, never from the code under test.

Density classes of the hand-made terms h0..h15, from build.cpp bucket_directory:
a term's bucket shift B is the smallest with df << (B + 1) > 4 N, and k_disj
takes the tile directory when B <= 12 (kDisjTileShift) and the "one bucket holds
the tile" searches when B > 12.  At N = 50,000: df = 24 gives 24 << 13 = 196,608
<= 200,000, so B = 13; df = 25 gives 25 << 13 = 204,800 > 200,000, so B = 12.  At
N = 140,000 the same line lies between df = 68 and 69 (`dir_shift`).
  h0..h3    every 2nd..5th doc: plain rank words by default;
  h4..h7    every 100th..200th doc: sparse rank words by default;
  h8..h11   40-60 (wide corpus: 75-95) random docs: the tile directory; those of
            h8..h10 lie within one or two tiles, so most of their tiles are
            empty (the -0.0f bound);
  h12..h15  2-12 random docs: wide buckets (B >= 13).
Every term also holds every edge doc (so the 16-Must query matches exactly
those, and every clause meets every other there): the first and last doc of a
512-doc block and of a 4096-doc tile, doc 0 and doc N - 1; tf 1-3 by term.
Doc 8191 is deleted, so nine edge docs are alive: they are the all-Should
query's nine best hits, and the ten are its top 10 without the deletion.
"""
from __future__ import annotations

import functools

import numpy as np

import bool_ref as br
import synth_ref as sr

MUST, SHOULD, MUST_NOT = br.MUST, br.SHOULD, br.MUST_NOT
V = 1 << 20
SEED_L, SEED_T = 0x5EED1, 20250808
N = 50_000
E = (0, 511, 512, 4095, 4096, 8191, 8192, 49151, 49152, 49999)
KS = (1, 10, 37, 1000, 1024)
SEG_BOUNDS = (0, 4096, 8191, 8192, 30_000, 49_999, N)  # cuts on and beside the edges, a one-doc segment
N_WIDE0, N_TINY, TINY = 140_000, 63, 64
# (the item boundaries of 16 / 28 / 32 tiles, the last tile's first doc)
E_WIDE = (0, 511, 512, 4095, 4096, 65535, 65536, 114687, 114688, 131071, 131072, 139263, 139264, 139999)


def dir_shift(df, n_docs):
    b = 0
    while b < 31 and (df << (b + 1)) <= 4 * n_docs:
        b += 1
    return b


def _rand_docs(seed, count, lo, hi):
    return lo + np.unique((sr.h2(seed, np.arange(count)) % np.uint64(hi - lo)).astype(np.int64))


def _append(n_docs, off, tok, lists):
    """The corpus with term t appended tf times to doc d for (t, docs, tf) in lists."""
    lens = np.diff(off.astype(np.int64))
    doc = [np.repeat(np.arange(n_docs, dtype=np.int64), lens)]
    tk = [tok]
    for t, ds, tf in lists:
        ds = np.asarray(ds, np.int64)
        tf = np.broadcast_to(np.asarray(tf, np.int64), ds.shape)
        doc.append(np.repeat(ds, tf))
        tk.append(np.full(int(tf.sum()), t, np.uint32))
    doc, tk = np.concatenate(doc), np.concatenate(tk)
    o = np.argsort(doc, kind="stable")
    new_off = np.zeros(n_docs + 1, np.uint64)
    new_off[1:] = np.cumsum(np.bincount(doc, minlength=n_docs))
    return new_off, tk[o].astype(np.uint32)


def _hand_terms(n, edges, n_rand, seed):
    """h0..h15 over docs [0, n): [(docs, tf)]."""
    e = np.array(edges, np.int64)
    out = []
    for j in range(16):
        if j < 4:
            d = np.arange(0, n, 2 + j)
        elif j < 8:
            d = np.arange(j, n, (100, 130, 160, 200)[j - 4])
        elif j < 12:
            # h8..h10 within two tiles, two tiles and one tile (every other tile holds at most
            # edge docs: most are empty), h11 anywhere
            nt = (n - 1) >> 12
            t0, t1 = ((1, 3), (nt - 2, nt), (nt // 2, nt // 2 + 1), (0, nt + 1))[j - 8]
            d = _rand_docs(seed + j, n_rand[j - 8], t0 << 12, min(t1 << 12, n))
        else:
            d = _rand_docs(seed + j, (2, 5, 8, 12)[j - 12], 0, n)
        out.append((np.union1d(d, e), 1 + j % 3))
    return out


def _batch(qs, occ):
    q_off = np.cumsum([0] + [len(q) for q in qs]).astype(np.uint32)
    return q_off, np.array([x for q in qs for x in q], np.uint32), np.array([x for o in occ for x in o], np.uint8)


@functools.lru_cache(maxsize=None)
def edges_case():
    off, tok = sr.corpus(N, V, 1.0, SEED_L, SEED_T)
    # hand-made terms: ids the synthetic corpus does not use, so their lists are exactly these
    free = iter(np.setdiff1d(np.arange(V - 4096, V - 1), tok)[::-1].tolist())
    hand = _hand_terms(N, E, (40, 47, 53, 60), 900)
    H = [next(free) for _ in range(16)]
    lists = [(H[j], d, tf) for j, (d, tf) in enumerate(hand)]
    T = {}
    # a dense term that holds some edge docs only (the MustNot that removes top docs)
    T["hx"] = next(free)
    docs_hx = np.union1d(np.arange(1, N, 3), [0, 4096, N - 1])
    lists.append((T["hx"], docs_hx, 1))
    # tf = 300 (an escaped tf: >= 255) on the last doc of tile 0 and the first of tile 1
    T["esc"] = next(free)
    docs_esc = np.union1d(np.arange(7, N, 500), [4095, 4096])
    lists.append((T["esc"], docs_esc, np.where(np.isin(docs_esc, [4095, 4096]), 300, 1)))
    # a term that is also in the `name` field of a third of its docs
    T["name"] = next(free)
    docs_name = np.union1d(np.arange(3, N, 331), E)
    lists.append((T["name"], docs_name, 2))
    off, tok = _append(N, off, tok, lists)
    name_off, name_tok = sr.names(N, vocab=1 << 9, seed=4245)
    name_off, name_tok = _append(N, name_off, name_tok, [(T["name"], docs_name[::3], 1)])
    # deletions: a seed that keeps every edge doc, then doc 8191 by hand
    seed = 77
    while sr.deleted_mask(N, seed)[list(E)].any():
        seed += 1
    deleted = sr.deleted_mask(N, seed)
    deleted[8191] = 1
    # three facet terms of kFmaskChunk - 1, kFmaskChunk and kFmaskChunk + 1 postings, each
    # with doc N - 1; the last one is missing from half the edge docs
    rest = np.setdiff1d(np.arange(N), E)
    fdocs = []
    for j, n_post in enumerate((8191, 8192, 8193)):
        e = np.array(E if j < 2 else E[::2] + (N - 1,), np.int64)
        fdocs.append(np.union1d(rest[j::6][:n_post - len(e)], e))
        assert len(fdocs[j]) == n_post and fdocs[j][-1] == N - 1
    no_tokens = (np.zeros(N + 1, np.uint64), np.zeros(0, np.uint32))
    facets = _append(N, *no_tokens, [(j, d, 1) for j, d in enumerate(fdocs)]) + (3,)
    ref = br.Corpus(V, off, tok, name_off, name_tok, deleted, facets)
    ref_nodel = br.Corpus(V, off, tok, name_off, name_tok, None, facets)

    # ---- the batch
    qs, occ, Q = [], [], {}

    def add(name, terms, occur):
        if name:
            Q[name] = len(qs)
        qs.append([int(t) for t in terms])
        occ.append(list(occur) if not isinstance(occur, int) else [occur] * len(terms))
        assert len(qs[-1]) == len(occ[-1]) <= 16

    zq = lambda n, m, rank, seed: sr.queries(n, m, m, rank, 1.0, seed)[1].tolist()  # noqa: E731
    df = ref.own.df_text
    rare = [t for t in np.flatnonzero((df >= 5) & (df <= 24)).tolist() if t not in H][:7]
    assert len(rare) == 7
    add("should16", H, SHOULD)
    add("should16_rev", H[::-1], SHOULD)
    add("should15_not1", H[1:] + [T["hx"]], [SHOULD] * 15 + [MUST_NOT])
    add("should15", H[1:], SHOULD)                                   # (its parent)
    z7 = zq(1, 7, 64, 501)
    add("should8_not8", H[0::2] + [T["hx"]] + z7, [SHOULD] * 8 + [MUST_NOT] * 8)
    add("should8", H[0::2], SHOULD)                                  # (its parent)
    add("must16", H, MUST)
    add("must12_should4", H, [MUST] * 12 + [SHOULD] * 4)
    # (Musts: every 60th doc and the edge docs; MustNots: hx and term 10, in about a third of the docs)
    add("must4_not2_should10", H[:4] + [T["hx"], 10] + H[4:14], [MUST] * 4 + [MUST_NOT] * 2 + [SHOULD] * 10)
    add("mixed6", [H[0], H[5], H[9], H[13], H[2], H[15]], SHOULD)
    add("mixed7", [H[12], H[1], H[6], H[10], H[14], H[3], H[8]], SHOULD)
    add("mixed9", [H[4], H[13], H[0], H[9], H[15], H[7], H[2], H[11], H[12]], SHOULD)
    add("mixed11", H[15:4:-1], SHOULD)
    add("must9", [H[4], H[13], H[0], H[9], H[15], H[7], H[2], H[11], H[12]], MUST)
    add("zipf13_hand3", zq(1, 13, 1 << 14, 502) + [H[1], H[6], H[12]], SHOULD)
    add("wide_only", H[12:], SHOULD)
    add("tiledir_only", H[8:12], SHOULD)
    add("dense1_rare15", [H[0]] + H[8:] + rare, SHOULD)
    add("esc8", [T["esc"], H[0], H[4], H[8], H[12], H[2], H[6], H[10]], SHOULD)
    add("esc8_must", [T["esc"], H[0], H[4], H[8], H[12], H[2], H[6], H[10]], [MUST, MUST] + [SHOULD] * 6)
    add("name8", [T["name"], H[1], H[5], H[9], H[13], H[3], H[7], H[11]], SHOULD)
    add("name8_must", [T["name"], H[1], H[5], H[9], H[13], H[3], H[7], H[11]], [MUST, MUST, MUST] + [SHOULD] * 5)
    add("dup16", H[:15] + [H[3]], SHOULD)
    # the rest: 6..16 distinct Zipf terms; OR, AND and mixed occurs by thirds (the AND and mixed
    # thirds from the 64 / 256 most frequent terms, so that they have hits)
    n_fill = 64 - len(qs)
    third = n_fill // 3
    for kind, (n, rank, seed) in enumerate(((n_fill - 2 * third, 1 << 14, 503), (third, 64, 504), (third, 256, 505))):
        fo, ft = sr.queries(n, 6, 16, rank, 1.0, seed)
        for i in range(n):
            t = ft[fo[i]:fo[i + 1]].tolist()
            o = [SHOULD] * len(t) if kind == 0 else [MUST] * len(t) if kind == 1 else \
                [MUST, MUST] + [(SHOULD, SHOULD, MUST_NOT)[(i + j) % 3] for j in range(len(t) - 2)]
            add(None, t, o)
    assert len(qs) == 64 and {len(q) for q in qs} >= set(range(6, 17))
    q_off, terms, occur = _batch(qs, occ)
    return dict(N=N, V=V, off=off, tok=tok, name_off=name_off, name_tok=name_tok, deleted=deleted, facets=facets,
                ref=ref, ref_nodel=ref_nodel, H=H, T=T, Q=Q, qs=qs, occ=occ, q_off=q_off, terms=terms, occur=occur,
                hand=hand, fdocs=fdocs)


@functools.lru_cache(maxsize=None)
def wide_case():
    """140,000 docs (35 tiles, the last of 736 docs) + 63 segments of 64 docs; the
    hand-made terms occur in the first segment only."""
    n = N_WIDE0 + N_TINY * TINY
    off, tok = sr.corpus(n, V, 1.0, SEED_L + 1, SEED_T + 1)
    free = iter(np.setdiff1d(np.arange(V - 4096, V - 1), tok)[::-1].tolist())
    hand = _hand_terms(N_WIDE0, E_WIDE, (75, 82, 88, 95), 950)
    H = [next(free) for _ in range(16)]
    off, tok = _append(n, off, tok, [(H[j], d, tf) for j, (d, tf) in enumerate(hand)])
    bounds = np.concatenate([[0], N_WIDE0 + TINY * np.arange(N_TINY + 1)]).astype(np.uint32)
    assert len(bounds) == 65 and bounds[-1] == n
    ref = br.Corpus(V, off, tok)
    base = [[H[0], H[13]], H[0:16:2], [H[4], H[13], H[0], H[9], H[15], H[7], H[2], H[11], H[12]], H]
    qs = [base[i % 4] for i in range(256)]
    q_off, terms, occur = _batch(qs, [[SHOULD] * len(q) for q in qs])
    return dict(N=n, V=V, off=off, tok=tok, bounds=bounds, ref=ref, H=H, hand=hand, qs=qs, q_off=q_off, terms=terms,
                occur=occur, base=base)
