"""Reference for facet filters on phrase, phrase-beside and group queries
(fg_filter_clauses), in numpy f32.  It calls nothing of libfugu.

The filter is Dataset::search's second Must: hits = the text query's hits that
some facet clause matches, score = text score + facet union score.  The text
side comes UNFILTERED from the family's own reference (phrase_ref.search,
bool_phrase_ref.Ref.hits, group_ref.Ref.hits); the facet side is
bool_ref.Corpus._facet_union, which restates the facet score (tf 1, the constant
fieldnorm id 1, the matching clauses summed from 0.0 in clause order).  Deleted
docs are no hits of the text side already; order (score desc, doc asc).

`facets(n, cuts)` generates FacetTokenizer tokens for an n-doc corpus, ancestors
included, in the (facet_off, facet_tok, n_facet_terms) form
native.Index.from_docs(..., facets=...) takes:
  /a (A: more than half the docs) with children /a/x, /a/y; /b with /b/z; /e with
  /e/w (the mid terms); /h (HOT: n/150 docs, the highest mid score); /r (RARE: 5
  docs, fewer than k = 10); /s (SEG: docs of the LAST segment of `cuts` only);
  NODOC: an id of the vocabulary that no doc holds.  A doc may hold several
  branches; about one in eight holds none.
"""
import functools

import numpy as np

import bool_phrase_ref as bpr
import bool_ref as br
import group_ref as gr
import phrase_ref as pr

F = np.float32
MISSING = br.MISSING
A, AX, AY, B, BZ, RARE, SEG, E, EW, HOT, NODOC = range(11)
N_FTERMS = 11
N_RARE = 5
CLAUSE_COUNTS = (1, 2, 3, 5, 8)  # mask shifts 0, 1, 2, 3 and the 256-entry table

# filter contents by clause count; a query takes variant (its index) % len of each count
VARIANTS = {
    1: [[A], [HOT], [B], [RARE], [SEG], [MISSING], [AX], [E]],
    2: [[A, HOT], [MISSING, B], [AX, BZ], [RARE, E], [HOT, SEG], [MISSING, NODOC], [E, A]],
    3: [[A, B, HOT], [AX, MISSING, E], [SEG, RARE, BZ], [HOT, AY, B], [EW, A, MISSING]],
    5: [[A, AX, B, HOT, E], [MISSING, AY, BZ, RARE, SEG], [HOT, EW, AX, NODOC, B]],
    8: [[A, AX, AY, B, BZ, E, EW, HOT], [RARE, MISSING, SEG, A, HOT, NODOC, EW, B],
        [HOT, BZ, AY, MISSING, E, SEG, AX, RARE]],
}
ALL_MISSING = ([MISSING], [MISSING, NODOC])


def facets(n, cuts, seed=5):
    """(facet_off u64 [n + 1], facet_tok u32, N_FTERMS); cuts: the segment bounds, SEG lies in the last segment"""
    r = np.random.default_rng(seed)
    has = np.zeros((n, N_FTERMS), bool)
    a = r.random(n) < 0.62
    u = r.random(n)
    has[:, A] = a
    has[:, AX] = a & (u < 0.35)
    has[:, AY] = a & (u >= 0.35) & (u < 0.6)
    b = r.random(n) < 0.25
    has[:, B] = b
    has[:, BZ] = b & (r.random(n) < 0.4)
    e = r.random(n) < 0.10
    has[:, E] = e
    has[:, EW] = e & (r.random(n) < 0.5)
    has[r.choice(n, max(n // 150, 8), replace=False), HOT] = True
    lo = int(cuts[-2])
    has[lo:, SEG] = r.random(n - lo) < 0.08
    has[r.random(n) < 0.12] = False  # docs without a facet
    has[r.choice(n, N_RARE, replace=False), RARE] = True
    has[:, NODOC] = False
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum(has.sum(1))
    return off, np.nonzero(has)[1].astype(np.uint32), N_FTERMS


def segment(fac, lo, hi):
    """the facet arrays of docs [lo, hi)"""
    off, tok, nf = fac
    return (off[lo:hi + 1] - off[lo]).astype(np.uint64), tok[int(off[lo]):int(off[hi])], nf


class Facets:
    """The facet side of an n-doc corpus: a bool_ref.Corpus without text, for its _facet_union."""

    def __init__(self, n, fac):
        self.n, self.fac = n, fac
        self.corpus = br.Corpus(1, np.zeros(n + 1, np.uint64), np.zeros(0, np.uint32), facets=fac)
        self.df = self.corpus.own.df_facet
        self.tot = self.corpus.own.tot_facet_tokens
        self._memo = {}

    def stats(self, n_docs=None, df=None, tot=None):
        """the statistics _facet_union reads (default: the corpus' own, deleted docs included)"""
        return br.Stats(self.n if n_docs is None else int(n_docs), (0, 0), None, None,
                        self.df if df is None else np.asarray(df, np.int64), self.tot if tot is None else int(tot))

    def union(self, fterms, st):
        key = (tuple(int(t) for t in fterms), id(st))
        if key not in self._memo:
            self._memo[key] = self.corpus._facet_union([int(t) for t in fterms], st) + (st,)  # (st kept: its id is the key)
        return self._memo[key][:2]

    def filtered(self, hits, fterms, st, k):
        """(scores f32, docs) of the top k: `hits` = the UNFILTERED (docs, scores) of the text query"""
        d, s = np.asarray(hits[0], np.int64), np.asarray(hits[1], F)
        if fterms is not None and len(fterms):
            fs, any_f = self.union(fterms, st)
            keep = any_f[d]
            d = d[keep]
            s = (s[keep] + fs[d]).astype(F)
        o = np.lexsort((d, -s))[:k]
        return s[o], d[o]


def cases(n_queries):
    """[(query index, fterms)]: every query with a filter of each clause count, the contents rotating"""
    return [(i, VARIANTS[n][(i + j) % len(VARIANTS[n])]) for i in range(n_queries) for j, n in enumerate(CLAUSE_COUNTS)]


def filter_arrays(flists):
    """(f_off, f_terms) of a batch's filter lists ([] or None: no filter)"""
    f_off = np.cumsum([0] + [len(f or []) for f in flists]).astype(np.uint32)
    f_terms = np.array([t for f in flists for t in (f or [])], np.uint32)
    return f_off, f_terms


def phrase_queries(c):
    """the phrase queries of a phrase_ref.Synth that the filter cases use: the two-term ones (many
    hits, so a filter leaves some) and every eighth of the rest (long spans, missing terms, repeats)"""
    return [q for i, q in enumerate(c.queries) if len(q[0]) == 2 or i % 8 == 0]


# ------------------------------------------------------------------ the three families' corpora, queries and cases
PHRASE_CUTS = (0, 1700, 4300, 6000)  # test_gpu_phrase.py's segments


class Family:
    """A kernel family's corpus side: `queries`, their UNFILTERED hits [(docs, scores)] computed
    once, the facet arrays, their reference and statistics, and the (query, filter) cases."""

    def __init__(self, name, n, cuts, queries, hits, seed=5):
        self.name, self.n, self.cuts, self.queries, self.hits = name, n, tuple(cuts), queries, hits
        self.fac = facets(n, cuts, seed)
        self.facets = Facets(n, self.fac)
        self.fst = self.facets.stats()
        self.cases = cases(len(queries))

    def want(self, case, k, hits=None, fst=None):
        i, fterms = case
        return self.facets.filtered((hits or self.hits)[i], fterms, fst or self.fst, k)


@functools.lru_cache(maxsize=None)
def phrase_synth():
    return pr.Synth()


def phrase_hits(c, queries, deleted=None):
    text, name = pr.Field(c.text, c.text_gaps), pr.Field(c.name, c.name_gaps)
    st = pr.Stats.of(text, name, pr.V)
    out = []
    for t, o in queries:
        s, d, _ = pr.search(text, name, st, t, o, c.n, deleted=c.deleted if deleted is None else deleted)
        out.append((d.astype(np.int64), s))
    return out


@functools.lru_cache(maxsize=None)
def phrase_family():
    c = phrase_synth()
    qs = phrase_queries(c)
    return Family("k_phrase", c.n, PHRASE_CUTS, qs, phrase_hits(c, qs))


def bphrase_queries(c):
    kinds = bpr.queries(c)
    return [q for kind in bpr.KINDS for q in kinds[kind]]


@functools.lru_cache(maxsize=None)
def bphrase_family():
    c = phrase_synth()
    ref = bpr.of_synth(c)
    qs = bphrase_queries(c)
    return Family("k_bphrase", c.n, PHRASE_CUTS, qs, [ref.hits(q) for q in qs])


LONG_LEAD_QUERY = [gr.G(gr.MUST, gr.ANY, [gr.T_LONG, gr.T_ABSENT]), gr.G(gr.MUST, gr.ANY, [gr.T_EVERY, gr.GONE[0]])]


def group_queries():
    kinds = gr.queries()
    return [q for kind in gr.KINDS for q in kinds[kind]]


@functools.lru_cache(maxsize=None)
def group_family():
    c = gr.synth()
    ref = gr.Ref(c.corpus)
    qs = group_queries()
    f = Family("k_group", gr.N, gr.SEG_CUTS, qs, [ref.hits(q) for q in qs])
    # (d) the query of test_group_ref.py's chunk-bound test, which leads from the 8193-posting list alone, with
    # every two- and three-clause filter: HOT docs of its later chunks enter the filtered top 10
    f.cases = f.cases + [(qs.index(LONG_LEAD_QUERY), v) for v in VARIANTS[2] + VARIANTS[3]]
    return f


# (e) a phrase whose lead list is longer than 4 x kChunk = 8192 postings: several work items, one threshold word.
# The batch holds the query BIG_COPIES times (filters rotating): in a batch of >= 256 queries the planner gives
# a query few items of several chunks each, so an item's later chunks are bounded against the threshold its
# earlier ones raised -- with HOT in the filter that threshold lies above every text-only bound.
BIG_N = 20000
BIG_QUERY = ([0, 1], [0, 1])  # the two most frequent terms
BIG_FILTERS = ([A, HOT, B], [HOT], [HOT, A], [E, HOT, BZ, AX])
BIG_COPIES = 256


@functools.lru_cache(maxsize=None)
def big_phrase_family():
    c = pr.Synth(n=BIG_N, seed=pr.SEED + 1)
    f = Family("k_phrase, a long lead list", c.n, (0, BIG_N // 3, 2 * BIG_N // 3, BIG_N), [BIG_QUERY],
               phrase_hits(c, [BIG_QUERY]))
    f.cases = [(0, BIG_FILTERS[i % len(BIG_FILTERS)]) for i in range(BIG_COPIES)]
    f.synth = c
    return f
