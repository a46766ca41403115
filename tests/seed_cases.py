"""The cases of the seeded-threshold tests (test_seed_cases.py on the CPU,
test_gpu_seeded_thr.py on the device) and the corpora test_gpu_conj_hist_thr.py
shares with them.

k_conj and k_disj keep a key exactly when key >= threshold and prune only on
upper bounds, so a plan whose starting threshold is seeded (Plan.seed_thresholds)
with the lowest key of a score s must return bool_ref's hits with score >= s,
cut to k.  Seeded with a query's exact k-th score, every chunk, tile and probe
meets the tightest threshold that is still valid, from the first work item on.

A case is a batch of queries with bool_ref's whole hit list per query (all the
scores, in (score desc, doc asc) order, and the docs of the first KEEP hits).
Seeds and expected lists are derived from those lists alone:
  zero   s = 0                         the plain top k, no starting threshold
  loose  s = ws[min(2k, hits) - 1]     a looser valid bound: the plain top k
  kth    s = ws[k - 1]                 the exact k-th score: the plain top k, ties kept
  half   s = ws[ceil(k / 2) - 1]       above the k-th score: the hits with score >= s
  top    s = ws[0]                     the top-score hits only
A query with fewer hits than the rank a row asks for gets seed 0 in that row.
"""
from __future__ import annotations

import functools

import numpy as np

import bool_ref as br
import clause_edges as ce
import synth_ref as sr

F = np.float32
M, S, X = br.MUST, br.SHOULD, br.MUST_NOT
N_BIG, N_TIE, N_FEW = 262_144, 100_000, 20_000
ROWS = ("zero", "loose", "kth", "half", "top")
KEEP = 1024  # docs kept per query: every k here is at most 1000
FACET_SETS = ([0], [1], [2], [1, br.MISSING], [br.MISSING, 2])  # (test_gpu_clause_edges.test_facet_filter's)
FACET_TEXTS = ("should16", "must16", "must4_not2_should10")


# ---- the corpora (test_gpu_conj_hist_thr.py's a. - d.)

def big_case():
    """The corpus of test_gpu_conj_hist_thr's a. and c., its reference, and the
    batch: 64 three-term and 16 five-term ANDs of the 8 most frequent terms."""
    from fugu_amd import synth
    c = synth.corpus(N_BIG)
    ref = br.Corpus(synth.VOCAB, c.off, c.tok)
    top = np.argsort(-ref.own.df_text, kind="stable")[:8]
    rng = np.random.default_rng(20)
    qs = [[int(t) for t in rng.choice(top, 3, replace=False)] for _ in range(64)]
    qs += [[int(t) for t in rng.choice(top, 5, replace=False)] for _ in range(16)]
    return c, ref, top, qs


def tie_case():
    """100,000 docs of six tokens, the query terms 1, 2, 3 once each: every match scores the same."""
    rng = np.random.default_rng(7)
    tok = np.empty((N_TIE, 6), np.uint32)
    tok[:, :3] = [1, 2, 3]
    tok[:, 3:] = rng.integers(10, 5000, (N_TIE, 3))
    off = (np.arange(N_TIE + 1, dtype=np.uint64) * np.uint64(6))
    return off, tok.reshape(-1), 5000, [[1, 2, 3], [1, 2], [3, 1, 2]]


def few_case():
    """A 20,000-doc corpus with facets and queries of fewer than 100 matches:
    (Must, MustNot, Should) around a term of 60-99 docs, two Musts the same way,
    and frequent terms under a rare facet."""
    from fugu_amd import synth
    V = 1 << 16
    c = synth.corpus(N_FEW, V)
    fo, ft, nf = sr.facet_tokens(N_FEW, 4242)
    ref = br.Corpus(V, c.off, c.tok, facets=(fo, ft, nf))
    df = ref.own.df_text
    top = np.argsort(-df, kind="stable")[:8]
    rare = [int(t) for t in np.flatnonzero((df >= 60) & (df < 100))[:4]]
    qs = [([t, int(top[7]), int(top[1])], [M, X, S], []) for t in rare]
    qs += [([t, int(top[0]), int(top[6]), int(top[2])], [M, M, X, S], []) for t in rare]
    qs += [([int(top[7]), int(top[5])], [M, M], [29 + 7 * a]) for a in range(4)]  # org/acme/teamA/proj0
    qs += [([int(top[3]), int(top[4]), int(top[6])], [M, M, M], [29 + 7 * a + 1]) for a in range(4)]
    return c, V, (fo, ft, nf), ref, qs


# ---- a case: queries, whole reference hit lists, seeds, expected lists

def seeds(full, k):
    """{row: f32 [nq]}: the seed scores of every row (0: no starting threshold)."""
    at = lambda ws, r: ws[r - 1] if 1 <= r <= len(ws) else F(0)  # noqa: E731
    rank = {"zero": lambda n: 0, "loose": lambda n: min(2 * k, n), "kth": lambda n: k,
            "half": lambda n: (k + 1) // 2, "top": lambda n: 1}
    out = {row: np.array([at(ws, rank[row](len(ws))) for ws, _ in full], F) for row in ROWS}
    assert all((s >= 0).all() and not np.signbit(s).any() for s in out.values())
    return out


def expect(full, seed, k):
    """[(scores, docs, c)] per query: the hits with score >= seed[q] cut to k,
    and the number c of hits with score >= seed[q]."""
    out = []
    for (ws, wd), s in zip(full, seed):
        c = int(np.searchsorted(-ws, -F(s), side="right"))  # (ws descends)
        assert c == int((ws >= s).sum())
        n = min(c, k)
        out.append((ws[:n], wd[:n], c))
    return out


def strict_drop(full, k):
    """Queries whose (k-1)-th score is above the k-th: the half and top rows return fewer than k."""
    return np.array([len(ws) >= k >= 2 and ws[k - 2] > ws[k - 1] for ws, _ in full])


def tie_across(full, k):
    """Queries whose (k+1)-th hit scores what the k-th does: the exact seed must keep the tie."""
    return np.array([len(ws) > k and ws[k] == ws[k - 1] for ws, _ in full])


class Case:
    """queries: [(terms, occur, facet terms)]; full: [(all scores f32, the first
    KEEP docs)] per query in (score desc, doc asc) order; bounds: the snapshots'
    doc ranges (None: one snapshot), the docs of `full` are global then."""

    def __init__(self, name, ks, queries, ref, bounds=None, stats=None, **data):
        self.name, self.ks, self.queries, self.bounds, self.stats = name, tuple(ks), queries, bounds, stats
        self.data = data
        self.full = []
        for t, o, f in queries:
            ws, wd = ref.search(t, o, ref.n, f if len(f) else None, seg_bounds=bounds, stats=stats)
            self.full.append((ws, wd[:KEEP].astype(np.int64)))
        assert max(self.ks) <= KEEP

    def __len__(self):
        return len(self.queries)

    def batch(self):
        """The arguments of Index.plan / Plan."""
        flat = lambda xs, t: np.array([x for q in xs for x in q], t)  # noqa: E731
        offs = lambda xs: np.cumsum([0] + [len(q) for q in xs]).astype(np.uint32)  # noqa: E731
        ts, os_, fs = zip(*self.queries)
        kw = dict(occur=flat(os_, np.uint8))
        if any(len(f) for f in fs):
            kw.update(f_off=offs(fs), f_terms=flat(fs, np.uint32))
        return offs(ts), flat(ts, np.uint32), kw

    def hits(self):
        return np.array([len(ws) for ws, _ in self.full])

    def seeds(self, k):
        return seeds(self.full, k)

    def expect(self, seed, k):
        return expect(self.full, seed, k)

    def strict_drop(self, k):
        return strict_drop(self.full, k)

    def tie_across(self, k):
        return tie_across(self.full, k)


def split(off, tok, bounds):
    """The snapshots' (off, tok) of a corpus cut at `bounds`."""
    return [(off[b:e + 1] - off[b], tok[int(off[b]):int(off[e])]) for b, e in zip(bounds[:-1], bounds[1:])]


@functools.lru_cache(maxsize=None)
def edges_cases():
    """clause_edges.edges_case() three ways: its 64 queries, the same under the
    statistics of a namespace three times as large (test_query_time_scoring's),
    and test_facet_filter's queries that carry text."""
    c = ce.edges_case()
    qs = [(c["qs"][i], c["occ"][i], []) for i in range(64)]
    more = sr.corpus(100_000, c["V"], 1.0, ce.SEED_L + 7, ce.SEED_T + 7)
    a, b = c["ref"].own, br.Corpus(c["V"], *more).own
    g2 = br.Stats(a.n_docs + b.n_docs, tuple(x + y for x, y in zip(a.tot_tokens, b.tot_tokens)), a.df_text + b.df_text,
                  a.df_name + b.df_name, a.df_facet, a.tot_facet_tokens)
    texts = [(c["qs"][c["Q"][n]], c["occ"][c["Q"][n]]) for n in FACET_TEXTS]
    fq = [(t, o, f) for f in FACET_SETS for t, o in texts]
    ks = (1, 10, 1000)
    return {"plain": Case("edges", ks, qs, c["ref"], c=c),
            "rescored": Case("edges rescored", ks, qs, c["ref"], stats=g2, c=c, more=more),
            "facets": Case("edges facets", ks, fq, c["ref"], c=c)}


def big_queries(top, ands):
    """The big case's batch: the ANDs of big_case(), then two-term ANDs, the single
    terms, 2 Must + 2 Should, 2 Must + 1 MustNot and ORs of 2-5 clauses."""
    rng = np.random.default_rng(21)
    pick = lambda n: [int(t) for t in rng.choice(top, n, replace=False)]  # noqa: E731
    qs = [(q, [M] * len(q), []) for q in ands]
    qs += [(pick(2), [M, M], []) for _ in range(16)]
    qs += [([int(t)], [M], []) for t in top]
    qs += [(pick(4), [M, M, S, S], []) for _ in range(16)]
    qs += [(pick(3), [M, M, X], []) for _ in range(16)]
    for i in range(16):
        n = 2 + i % 4
        qs.append((pick(n), [S] * n, []))
    kinds = ["and3"] * 64 + ["and5"] * 16 + ["and2"] * 16 + ["single"] * 8 + ["must_should"] * 16 + ["must_not"] * 16 + \
        ["or"] * 16
    return qs, kinds


@functools.lru_cache(maxsize=None)
def big_cases():
    """{"one": the big corpus as one snapshot, "two": cut in halves under summed statistics}."""
    from fugu_amd import synth
    c, ref, top, ands = big_case()
    qs, kinds = big_queries(top, ands)
    bounds = np.array([0, N_BIG // 2, N_BIG], np.int64)
    d = dict(c=c, V=synth.VOCAB, top=top, kinds=kinds)
    return {"one": Case("big", (10, 100, 1000), qs, ref, **d),
            "two": Case("big, two snapshots", (10, 100), qs, ref, bounds=bounds, **d)}


@functools.lru_cache(maxsize=None)
def tie_cases():
    off, tok, V, qs = tie_case()
    ref = br.Corpus(V, off, tok)
    qs = [(q, [M] * len(q), []) for q in qs]
    bounds = np.array([0, N_TIE // 2, N_TIE], np.int64)
    d = dict(off=off, tok=tok, V=V)
    return {"one": Case("ties", (10, 100), qs, ref, **d),
            "two": Case("ties, two snapshots", (10, 100), qs, ref, bounds=bounds, **d)}


@functools.lru_cache(maxsize=None)
def few_cases():
    c, V, facets, ref, qs = few_case()
    return Case("few", (100,), qs, ref, c=c, V=V, facets=facets)
