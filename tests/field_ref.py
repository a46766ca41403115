"""Reference for queries with field-qualified term clauses (`name:report`, DESIGN.md
§20), in numpy f32, composed from bool_ref the way group_ref is: prepared clause
arrays go behind `group_ref._Clauses`, and `bool_ref.Corpus._match` joins them
unchanged.  It calls nothing of libfugu.

A query is a list of clauses (occur, term, field): field None is the unqualified
term, Should(text:t, name:t), as bool_ref scores it; field 0 (`text`) or 1 (`name`)
is tantivy's TermQuery on that one field.

A field clause gives a doc a score or "absent":
  * present iff the doc holds the term in THAT field (the field's tf > 0); a doc
    that holds the term in the other field only is absent;
  * the score is the field's part alone, w_field * (tf / (tf + cache_field[fn_field]))
    in f32, with the weight and the cache the unqualified clause uses for that
    field under the same statistics: built from `Corpus.fld[field]` alone.  On a
    doc that holds the term in that field only these are the unqualified clause's
    bits (0.0 + s is s).
Cost, used only for the Must order: the clause's docs inside the segment -- a
field clause's in its field's list alone, an unqualified clause's in the text list
plus the name list (as bool_ref).  The field rule is stated as upstream knowledge,
not as checked fact: it is not pinned against tantivy (DESIGN.md §0 row c: parity
is unpinned), as group_ref's group rules are not.

A term the segment lacks in that field (or FG_TERM_MISSING, an id past the
vocabulary, or a `name` clause on a corpus without names) is absent on all its
docs: an absent Must empties the query in that segment, an absent Should or MustNot
drops out; one Should without a Must is that clause as a Must (the same bits).
The join is bool_ref's: Musts in (the segment's cost, position) order, (s0 + s1) +
(0.0 + s2 + ...), then (0.0 + req) + opt; Shoulds alone from 0.0 in clause order;
MustNot excludes; deleted docs never hit; order (score desc, doc asc).
"""
import functools

import numpy as np

import bool_ref as br
import group_ref as gr
from bool_ref import gg

MUST, SHOULD, MUST_NOT = br.MUST, br.SHOULD, br.MUST_NOT
MISSING = br.MISSING
TEXT, NAME = 0, 1
FLAG = {TEXT: 0x20000000, NAME: 0x10000000}  # fugu.h FG_CLAUSE_TEXT / FG_CLAUSE_NAME
F = np.float32
hits_of = br.hits_of


def C(oc, t, field=None):
    return (oc, int(t), field)


def strip(query):
    """the same query with the fields stripped: every clause the unqualified term"""
    return [(oc, t, None) for oc, t, _ in query]


class Ref:
    def __init__(self, corpus: br.Corpus):
        self.c = corpus
        self.n = corpus.n
        self._memo = {}

    def _clause(self, t, field, st):
        """(scores [n] f32, -1 where absent; cost prefix [n + 1]: the clause's docs < d)"""
        if not 0 <= t < self.c.n_terms:
            return np.full(self.n, F(-1.0)), np.zeros(self.n + 1, np.int64)
        if field is None:
            return self.c.clause(t, st)
        key = (t, field, id(st))
        if key not in self._memo:
            s = np.zeros(self.n, F)
            on = np.zeros(self.n, bool)
            cnt = np.zeros(self.n + 1, np.int64)
            if field < len(self.c.fld):
                d, tf = self.c._list(self.c.fld[field], t)
                if len(d):
                    w = gg.weight(int((st.df_text, st.df_name)[field][t]), int(st.n_docs))
                    c = gg.cache(F(st.tot_tokens[field]) / F(st.n_docs))[self.c.fn[field][d]]
                    tff = tf.astype(F)
                    s[d] = s[d] + w * (tff / (tff + c))
                    on[d] = True
                    cnt[d + 1] += 1
            s[~on] = F(-1.0)
            self._memo[key] = (s, np.cumsum(cnt), st)  # (st kept: its id is the key)
        return self._memo[key][:2]

    def hits(self, query, seg_bounds=None, stats=None, deleted=None):
        """(docs, scores) of every hit, by segment"""
        st = stats or self.c.own
        alive = self.c.alive if deleted is None else ~np.asarray(deleted, bool)
        bounds = [0, self.n] if seg_bounds is None else [int(b) for b in seg_bounds]
        occur = [int(oc) for oc, _, _ in query]
        arrays = [self._clause(t, f, st) for _, t, f in query]
        cl = gr._Clauses(self.n, arrays)
        ds, ss = [], []
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            m, sc = br.Corpus._match(cl, list(range(len(query))), occur, lo, hi, None, True)
            d = np.flatnonzero(m & alive[lo:hi])
            ds.append(d + lo)
            ss.append(sc[d])
        return np.concatenate(ds), np.concatenate(ss).astype(F)

    def search(self, query, k, **kw):
        """top k by (score desc, doc asc): (scores f32, docs)"""
        d, s = self.hits(query, **kw)
        o = np.lexsort((d, -s))[:k]
        return s[o], d[o]


def batch(queries):
    """(q_off, terms, occur, phrase_len, phrase_pos) of the queries: the fg_query_batch arrays, a field
    clause as FG_CLAUSE_TEXT / FG_CLAUSE_NAME OR-ed onto its phrase_len entry 1"""
    q_off, terms, occur, plen = [0], [], [], []
    for q in queries:
        for oc, t, f in q:
            terms.append(t)
            occur.append(oc)
            plen.append(1 if f is None else 1 | FLAG[f])
        q_off.append(len(terms))
    return (np.array(q_off, np.uint32), np.array(terms, np.uint32), np.array(occur, np.uint8),
            np.array(plen, np.uint32), np.zeros(len(terms), np.uint32))


# ------------------------------------------------------------------ the corpus of the GPU test
N, V = 12000, 64
# MERGED list lengths (docs in either field) on k_field's edges: a lead chunk is kChunk = 2048 postings, a work
# item at most kPhraseMaxGroup = 4 chunks (8192 postings).  An edge term's docs are, in turn, text only, in both
# fields and name only.
T_LONG, T_2047, T_2048, T_2049, T_FEW, T_ABSENT, T_EVERY = 0, 1, 2, 3, 4, 5, 63
EDGE_LEN = {T_LONG: 8193, T_2047: 2047, T_2048: 2048, T_2049: 2049, T_FEW: 40}
BOTH_OVER = range(6, 12)       # text terms that are in the names of every third of their docs too
BOTH_DISJ = range(12, 16)      # terms whose name docs and text docs are disjoint
TEXT_ONLY = range(16, 48)      # (40..47: rare ones)
NAME_ONLY = range(48, 56)      # terms with `name` postings only
T_ESC_TEXT, T_ESC_NAME = 6, 7  # a tf >= 255 in text (name) in three docs whose name (text) tf of the term is 1
ESC_DOCS = {T_ESC_TEXT: (11, 4011 + 1200, 9011), T_ESC_NAME: (17, 5017 + 300, 10017)}
T_LOW = 40                     # a rare term whose docs all lie below SEG_CUTS[1]
# three segments of unequal size: T_FEW only in the last, T_LOW only in the first, NO name postings in the second
SEG_CUTS = (0, 3000, 5000, N)
GONE = (MISSING, V + 7)        # FG_TERM_MISSING, an id past the vocabulary


class Synth:
    """12,000 docs over 64 terms in two fields, deleted docs, escaped tfs (>= 255) in either field."""

    def __init__(self, seed=20261021):
        r = np.random.default_rng(seed)
        nameless = lambda d: (d >= SEG_CUTS[1]) & (d < SEG_CUTS[2])  # noqa: E731
        text, name = [], []  # (doc, term, tf)

        def put(rows, d, t, tf):
            rows.append((np.asarray(d, np.int64), np.full(len(d), t), np.asarray(tf, np.int64)))

        for t, n in EDGE_LEN.items():
            lo, hi = (SEG_CUTS[2], N) if t == T_FEW else (0, N)
            # the merged list has exactly n docs: the middle segment's docs stay text docs (no names there)
            d = lo + np.sort(r.choice(hi - lo, n, replace=False))
            part = np.arange(n) % 3  # 0: text only, 1: both, 2: name only
            part[nameless(d)] = 0
            tf = r.integers(1, 5, n)
            if t == T_LONG:  # high scores in its first lead chunk only: later chunks fall below a small k's threshold
                tf = np.where(np.arange(n) < 1500, r.integers(3, 5, n), 1)
            if t == T_2047:
                tf[np.flatnonzero(part == 0)[3]] = 300  # an escaped tf byte on an edge list
            put(text, d[part < 2], t, tf[part < 2])
            put(name, d[part > 0], t, r.integers(1, 3, int((part > 0).sum())))
        for t in list(BOTH_OVER) + list(BOTH_DISJ) + list(TEXT_ONLY):
            n = int(r.integers(20, 300)) if t >= 40 else int(r.integers(150, 5000))
            lo, hi = (0, SEG_CUTS[1]) if t == T_LOW else (0, N)
            d = lo + np.sort(r.choice(hi - lo, n, replace=False))
            esc = ESC_DOCS.get(t, ())
            d = np.union1d(d, np.array(esc, np.int64))
            tf = r.integers(1, 5, len(d))
            if t in BOTH_OVER:
                dn = d[::3]
                dn = np.union1d(dn[~nameless(dn)], np.array(esc, np.int64))
                tn = r.integers(1, 3, len(dn))
                if t == T_ESC_TEXT:
                    tf[np.isin(d, esc)] = (255, 300, 1000)
                    tn[np.isin(dn, esc)] = 1
                if t == T_ESC_NAME:
                    tf[np.isin(d, esc)] = 1
                    tn[np.isin(dn, esc)] = (255, 260, 400)
                put(name, dn, t, tn)
            if t in BOTH_DISJ:
                rest = np.setdiff1d(np.arange(N), d)
                dn = np.sort(r.choice(rest[~nameless(rest)], int(r.integers(100, 1500)), replace=False))
                put(name, dn, t, r.integers(1, 3, len(dn)))
            put(text, d, t, tf)
        put(text, np.arange(N), T_EVERY, np.ones(N, np.int64))  # no doc is empty
        for t in NAME_ONLY:
            d = np.sort(r.choice(N, int(r.integers(50, 1500)), replace=False))
            d = d[~nameless(d)]
            put(name, d, t, r.integers(1, 3, len(d)))
        self.text_off, self.text_tok = self._csr(text)
        self.name_off, self.name_tok = self._csr(name)
        self.deleted = (r.random(N) < 0.03).astype(np.uint8)
        for docs in ESC_DOCS.values():
            self.deleted[list(docs)] = 0
        self.corpus = br.Corpus(V, self.text_off, self.text_tok, self.name_off, self.name_tok, self.deleted)

    _csr = staticmethod(gr.Synth._csr)
    segment = gr.Synth.segment
    merged_len = gr.Synth.merged_len


@functools.lru_cache(maxsize=None)
def synth():
    return Synth()


# the kind whose fields decide nothing: `name:a text:a` IS the unqualified `a`, docs and score bits
EQUAL = "same_both"
KINDS = ("lone", "must_nt", "must_nu", EQUAL, "shoulds", "not_name", "must_should", "lacking", "tie")
PER_KIND = 12
KS = (1, 10, 100, 1000)


def queries(per_kind=PER_KIND, seed=43):
    """{kind: [query]} on synth(): every kind leads from the edge lists in some query"""
    r = np.random.default_rng(seed)
    edge = [T_2047, T_2048, T_2049, T_LONG, T_FEW]
    both = list(BOTH_OVER) + list(BOTH_DISJ)
    mid = list(range(16, 40))
    rare = list(range(40, 48))

    def pick(pool, n=1, avoid=()):
        cand = [t for t in pool if t not in avoid]
        return [int(x) for x in r.choice(cand, n, replace=False)]

    out = {k: [] for k in KINDS}
    for i in range(per_kind):
        e = edge[i % len(edge)]
        f = (NAME, TEXT)[i % 2]
        a, b = pick(both, 2)
        m1, m2 = pick(mid, 2)
        n1, = pick(list(NAME_ONLY))
        # a lone `name:t` / `text:t`: an edge term, the escaped terms, a term in both fields
        out["lone"].append([C(SHOULD if i % 3 else MUST, (e, T_ESC_TEXT, T_ESC_NAME, a)[i % 4] if i < 8 else e, f)])
        # +name:a +text:b
        out["must_nt"].append([C(MUST, (e, a)[i % 2], NAME), C(MUST, (b, e)[i % 2], TEXT)])
        # +name:a +b
        out["must_nu"].append([C(MUST, (e, a, n1)[i % 3], NAME), C(MUST, (b, e, T_EVERY)[i % 3])])
        # name:a text:a, the same term in both fields as two Shoulds
        out[EQUAL].append([C(SHOULD, (e, a, T_ESC_TEXT, T_ESC_NAME, m1, n1)[i % 6], NAME if i % 2 else TEXT),
                           C(SHOULD, (e, a, T_ESC_TEXT, T_ESC_NAME, m1, n1)[i % 6], TEXT if i % 2 else NAME)])
        # Should-only mixes of 3-6 clauses
        ts = [e, a, b, m1, n1, T_ESC_NAME][: 3 + i % 4]
        out["shoulds"].append([C(SHOULD, t, (NAME, None, TEXT, NAME, NAME, TEXT)[(j + i) % 6]) for j, t in enumerate(ts)])
        # +a -name:b
        out["not_name"].append([C(MUST, (e, a, T_EVERY)[i % 3]), C(MUST_NOT, (b, e, a)[i % 3], NAME)])
        # +text:a name:b
        out["must_should"].append([C(MUST, (e, a)[i % 2], TEXT), C(SHOULD, (b, e)[i % 2], NAME)]
                                  + ([C(SHOULD, m2)] if i % 3 == 0 else []))
        # a clause on a field the term lacks (or a term that is missing): a Must one in four
        gone = (m1, n1, T_ABSENT, GONE[0], GONE[1], m2)[i % 6]
        gf = TEXT if gone == n1 else NAME
        out["lacking"].append([C(MUST, e, f), C(MUST, gone, gf)] if i % 4 == 3 else
                              [C(SHOULD, gone, gf), C(SHOULD, e, f), C(MUST_NOT if i % 2 else SHOULD, a, NAME)])
        # few distinct scores (tf 1-4, small fieldnorm ids): the k-th and (k+1)-th hits tie at the KS
        out["tie"].append([C(MUST, T_EVERY, TEXT), C(MUST_NOT, e, NAME)] if i % 2 else
                          [C(SHOULD, T_EVERY, TEXT), C(SHOULD, T_EVERY, NAME), C(MUST_NOT, a, TEXT)])
    return out
