"""Reference for queries with field-qualified phrase clauses (`name:"annual report"`,
`name:e-mail`, `+name:"q3 report" +budget`) and field term clauses beside phrase
clauses, in numpy f32.  Composed the way bool_phrase_ref and
field_ref are: `phrase_ref.Field.counts` / `weight` / `tf_cache` give a field
phrase's per-doc scores, `field_ref.Ref._clause` a one-field term clause's,
`bool_phrase_ref.Ref.clause` the unqualified clauses', and `bool_ref.Corpus._match`
joins the prepared clause arrays unchanged.  It calls nothing of libfugu.

A query is a list of clauses (terms, offsets, occur, field): one term is a term
clause, several a phrase; field None is the unqualified clause (both fields), TEXT
or NAME tantivy's TermQuery / PhraseQuery on that one field.

A field phrase clause gives a doc a score or "absent":
  * present iff the phrase count in THAT field's token stream is >= 1; a doc that
    holds the phrase in the other field only is absent;
  * the score is the field's part alone, weight_f * (c / (c + cache_f[fieldnorm_f])),
    weight_f = (sum_j idf(df_f(term_j), N), phrase order, from 0.0, a repeated term
    each time) * (1 + K1): the bits of the unqualified phrase's part for that field
    under the same statistics, and of the whole unqualified clause on a doc that
    holds the phrase in that field only (0.0 + s is s).
Cost, used only for the Must order: a field phrase's is the smallest doc count in
that field among its terms, inside the segment -- bool_phrase_ref's rule with the
other field's summand dropped; a field term's the field's doc count (field_ref);
an unqualified clause keeps bool_phrase_ref's.  The rule is stated as upstream
knowledge, not as checked fact: it is not pinned against tantivy (DESIGN.md §0 row
c), as §14's and §20's are not.

A segment that lacks a term of the clause in that field (FG_TERM_MISSING, an id
past the vocabulary, a `name` clause on a corpus without names) sees the clause
absent on all its docs: an absent Must empties the query there, an absent Should
or MustNot drops out; one Should without a Must is that clause as a Must (the same
bits).  The join is bool_ref's: Musts in (the segment's cost, position) order,
(s0 + s1) + (0.0 + s2 + ...), then (0.0 + req) + opt; Shoulds alone from 0.0 in
clause order; MustNot excludes; deleted docs never hit; order (score desc, doc asc).
"""
import functools

import numpy as np

import bool_phrase_ref as bp
import bool_ref as br
import field_ref as fr
import phrase_ref as pr

MUST, SHOULD, MUST_NOT = br.MUST, br.SHOULD, br.MUST_NOT
MISSING = br.MISSING
TEXT, NAME = fr.TEXT, fr.NAME
FLAG = fr.FLAG  # fugu.h FG_CLAUSE_TEXT / FG_CLAUSE_NAME
F = np.float32
hits_of = br.hits_of


def T(t, oc, field=None):
    return ([int(t)], [0], oc, field)


def P(terms, oc, field=None, offsets=None):
    return ([int(t) for t in terms], list(range(len(terms))) if offsets is None else list(offsets), oc, field)


def strip(query):
    """the same query with the fields stripped: every clause the unqualified one"""
    return [(t, o, oc, None) for t, o, oc, _ in query]


class Ref:
    def __init__(self, n_terms, text, text_gaps=None, name=None, name_gaps=None, deleted=None):
        self.b = bp.Ref(n_terms, text, text_gaps, name, name_gaps, deleted)
        self.f = fr.Ref(self.b.corpus)
        self.n, self.n_terms = self.b.n, n_terms
        self.fields = (self.b.text, self.b.name)
        self.pstats = self.b.pstats
        self._memo = {}

    def clause(self, terms, offsets, field, st):
        """(scores [n] f32, -1 where absent; cost(lo, hi))"""
        terms = [int(t) for t in terms]
        if field is None:
            return self.b.clause(terms, offsets, st)
        key = (tuple(terms), tuple(int(o) for o in offsets), field, id(st))
        if key in self._memo:
            return self._memo[key][:2]
        if len(terms) == 1:  # field_ref's one-field term clause
            s, pre = self.f._clause(terms[0], field, self.b._bstats(st))
            cost = lambda lo, hi: int(pre[hi] - pre[lo])  # noqa: E731
        else:
            s = np.full(self.n, F(-1.0))
            fld = self.fields[field]
            if fld is not None:
                cnt = fld.counts(terms, offsets)
                w = pr.weight((st.df_text, st.df_name)[field], st.n, terms)
                cache = pr.tf_cache(st.tot[field], st.n)
                m = cnt > 0
                c = cnt[m].astype(F)
                s[m] = F(0.0) + w * (c / (c + cache[fld.fn[m]]))
            pres = [self.b._prefix(t, field) for t in terms]
            cost = lambda lo, hi: min(int(p[hi] - p[lo]) for p in pres)  # noqa: E731
        self._memo[key] = (s, cost, st)  # (st kept: its id is the key)
        return s, cost

    def hits(self, query, seg_bounds=None, stats=None, deleted=None):
        """(docs, scores) of every hit, by segment"""
        st = stats or self.pstats
        dele = self.b.deleted if deleted is None else np.asarray(deleted, bool)
        bounds = [0, self.n] if seg_bounds is None else [int(b) for b in seg_bounds]
        cl = [self.clause(t, o, f, st) for t, o, _, f in query]
        occur = [int(oc) for _, _, oc, _ in query]
        ds, ss = [], []
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            arrays = []
            for s, cost in cl:  # the cost as a prefix that differs by it across [lo, hi)
                pre = np.zeros(self.n + 1, np.int64)
                pre[hi:] = cost(lo, hi) if hi > lo else 0
                arrays.append((s, pre))
            m, sc = br.Corpus._match(bp._Clauses(self.n, arrays), list(range(len(cl))), occur, lo, hi, None, True)
            d = np.flatnonzero(m & ~dele[lo:hi])
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
    clause as FG_CLAUSE_TEXT / FG_CLAUSE_NAME OR-ed onto its first phrase_len entry"""
    q_off = np.cumsum([0] + [sum(len(t) for t, _, _, _ in q) for q in queries]).astype(np.uint32)
    terms = np.array([x for q in queries for t, _, _, _ in q for x in t], np.uint32)
    occur = np.array([oc for q in queries for t, _, oc, _ in q for _ in t], np.uint8)
    plen = np.array([(len(t) | (FLAG[f] if f is not None else 0)) if j == 0 else 0
                     for q in queries for t, _, _, f in q for j in range(len(t))], np.uint32)
    ppos = np.array([x for q in queries for _, o, _, _ in q for x in o], np.uint32)
    return q_off, terms, occur, plen, ppos


# ------------------------------------------------------------------ the corpus of the GPU test
N, V = 12000, 64        # the random part: text over ids 0..59, names over all 64 (60..63 in names only)
V_TEXT = 60
# hand-placed terms, outside the random vocabulary.  The MERGED lists (docs in either field) of the three edge terms
# sit on k_fphrase's edges: a lead chunk is kChunk = 2048 postings.  An edge term's docs are, in turn, text only, in
# both fields and name only; each is followed by E_B, so `name:"E E_B"` leads from E's list (E_B is in all of them).
E_2047, E_2048, E_2049, E_B = 64, 65, 66, 67
EDGES = {E_2047: 2047, E_2048: 2048, E_2049: 2049}
T_ABSENT = 68           # in the vocabulary, no posting
X_A, X_B, X_T = 69, 70, 71  # escaped tfs: `X_A`^n X_B in three names, `X_T`^n X_B in three texts, n = 255, 300, 1000
V_ALL = 72
ESC_N = (255, 300, 1000)
ESC_NAME_DOCS, ESC_TEXT_DOCS = (5021, 7301, 10017), (5033, 7313, 10029)  # X_A, X_T: only in the last segment
REP_T, REP_DOC = 30, 2001  # the name `a a a`: `name:"a a"` counts 2
GAP_OFFSETS = [0, 2]    # `E _ E_B` with a dropped token (or another word) in between
# three segments of unequal size: NO name tokens in the second, X_A / X_T only in the last
SEG_CUTS = (0, 3000, 5000, N)
GONE = (MISSING, V_ALL + 7)  # FG_TERM_MISSING, an id past the vocabulary


class Synth:
    """12,000 docs as token streams: text 1-120 tokens, Zipf s = 1 over ids 0..59; a name on every even doc outside
    the second segment, 3-16 tokens, Zipf over all 64 ids with the name-only ids 60..63 at ranks 9..12; 5% deleted;
    a dropped token in a few names; and the hand-placed docs above."""

    def __init__(self, seed=20261021):
        r = np.random.default_rng(seed)
        n = N
        p = 1.0 / np.arange(1, V_TEXT + 1)
        p /= p.sum()
        text = [list(r.choice(V_TEXT, int(l), p=p)) for l in r.integers(1, 121, n)]
        pn = 1.0 / np.arange(1, V + 1)
        pn /= pn.sum()
        perm = np.concatenate([np.arange(0, 8), np.arange(60, 64), np.arange(8, 60)])  # rank -> id
        nameless = lambda d: SEG_CUTS[1] <= d < SEG_CUTS[2]  # noqa: E731
        name = [list(perm[r.choice(V, int(r.integers(3, 17)), p=pn)]) if i % 2 == 0 and not nameless(i) else []
                for i in range(n)]
        self.deleted = r.random(n) < 0.05
        name_gaps = [None] * n
        for i in range(0, n, 150):  # a few names with a dropped token
            if name[i]:
                name_gaps[i] = [1]
        self.hand = set()  # docs that must stay alive
        for e, cnt in EDGES.items():
            docs = np.sort(r.choice(n, cnt, replace=False))
            for i, d in enumerate(docs):
                d = int(d)
                part = 0 if nameless(d) else i % 3  # 0: text only, 1: both, 2: name only
                apart = [e, 9, E_B] if i % 7 == 3 else [e, E_B]  # (every 7th: the terms are there, not adjacent)
                if part < 2:
                    text[d] += apart
                if part > 0:
                    if i % 11 == 5 and len(apart) == 2:  # a dropped token between the two: a gap inside a name
                        name_gaps[d] = sorted((name_gaps[d] or []) + [len(name[d]) + 1])
                    name[d] += apart
        for d, m in zip(ESC_NAME_DOCS, ESC_N):  # tf >= 255 in the name, 1 in the text (no phrase there)
            name[d] = [X_A] * m + [X_B]
            text[d] += [X_A]
            self.hand.add(d)
        for d, m in zip(ESC_TEXT_DOCS, ESC_N):  # and the reverse
            text[d] += [X_T] * m + [X_B]
            name[d] = [X_T]
            self.hand.add(d)
        for j, d in enumerate(range(6000, 6040, 2)):  # the same phrases at tf 1: in the name, in the text, in both
            if j % 3 != 1:
                name[d] += [X_A, X_B] if j % 2 else [X_T, X_B]
            if j % 3 != 0:
                text[d] += [X_A, X_B] if j % 2 else [X_T, X_B]
        name[REP_DOC] = [REP_T] * 3
        self.hand.add(REP_DOC)
        self.deleted[list(self.hand)] = False
        u32 = lambda rows: [np.asarray(x, np.uint32) for x in rows]  # noqa: E731
        self.text, self.name, self.n = u32(text), u32(name), n
        self.text_gaps, self.name_gaps = [None] * n, name_gaps

    csr = pr.Synth.csr

    def ref(self, deleted=None):
        return Ref(V_ALL, self.text, self.text_gaps, self.name, self.name_gaps,
                   self.deleted if deleted is None else deleted)

    def merged_len(self, t):
        return sum(1 for a, b in zip(self.text, self.name) if t in a or t in b)


@functools.lru_cache(maxsize=None)
def synth():
    return Synth()


# the kind whose fields decide nothing: `name:"a b" text:"a b"` IS the unqualified `"a b"`, docs and score bits
EQUAL = "same_both"
LACKING = "lacking"     # a Must on a field the phrase (the term) lacks: no hits, by construction
KINDS = ("lone_name2", "lone_text3", "must_np_t", "must_np_tt", "should_np_t", EQUAL, "not_np", "nt_p", "tp_np",
         LACKING, "tie")
DECIDING = tuple(k for k in KINDS if k not in (EQUAL, LACKING, "tie"))
PER_KIND = 12
KS = (1, 10, 100, 1000)
# frequent name pairs whose hits tie across the cut at k = 10 and at k = 100 (test_field_phrase_ref.py pins it)
TIE_PAIRS = ((1, 0), (1, 2), (3, 0), (0, 4), (1, 1), (2, 2), (0, 3), (1, 4), (2, 1), (2, 0), (1, 3), (4, 0))


def queries(per_kind=PER_KIND, seed=47):
    """{kind: [query]} on synth(): spans cut from alive docs, the hand-placed phrases among them"""
    c = synth()
    r = np.random.default_rng(seed)
    alive = np.nonzero(~c.deleted)[0]
    named = [int(i) for i in alive if len(c.name[i]) >= 4 and len(c.text[i]) >= 8 and c.name_gaps[i] is None
             and i not in c.hand and max(c.name[i]) < V and max(c.text[i]) < V]
    edges = list(EDGES)

    def doc():
        return named[int(r.integers(0, len(named)))]

    def cut(toks, m):
        s = int(r.integers(0, len(toks) - m + 1))
        return [int(x) for x in toks[s:s + m]]

    def other(toks, avoid):
        cand = [int(x) for x in toks if int(x) not in avoid]
        return cand[int(r.integers(0, len(cand)))] if cand else int(toks[0])

    def rare():
        return int(r.integers(40, V_TEXT))

    out = {k: [] for k in KINDS}
    for i in range(per_kind):
        e = edges[i % 3]
        d = doc()
        ab = [e, E_B] if i < 3 else cut(c.name[d], 2)  # a name's two-term span; the first three: the edge lists
        # lone name:"a b": the edges, the escaped tf, the repeated term, the gap
        out["lone_name2"].append([
            P(ab, MUST if i % 2 else SHOULD, NAME) if i < 3 or i > 6 else
            P([X_A, X_B], SHOULD, NAME) if i == 3 else P([REP_T, REP_T], SHOULD, NAME) if i == 4 else
            P([edges[i % 3], E_B], SHOULD, NAME, GAP_OFFSETS)])
        # lone text:"a b c"
        out["lone_text3"].append([P([X_T, X_T, X_B], SHOULD, TEXT) if i == 0 else
                                  P(cut(c.text[doc()], 3), MUST if i % 2 else SHOULD, TEXT)])
        # +name:"a b" +c
        out["must_np_t"].append([P(ab, MUST, NAME), T(0 if i < 3 else other(c.text[d], ab), MUST)])
        # +name:"a b" +text:c
        out["must_np_tt"].append([P(ab, MUST, NAME), T(1 if i < 3 else other(c.text[d], ab), MUST, TEXT)])
        # name:"a b" c
        out["should_np_t"].append([P(ab, SHOULD, NAME), T(rare(), SHOULD)])
        # name:"a b" text:"a b", in either order
        sb = ab if i % 2 == 0 else cut(c.text[d], 2)
        out[EQUAL].append([P(sb, SHOULD, NAME if i % 4 < 2 else TEXT), P(sb, SHOULD, TEXT if i % 4 < 2 else NAME)])
        # +c -name:"a b"
        out["not_np"].append([T(0 if i < 3 else other(c.name[d], ()), MUST), P(ab, MUST_NOT, NAME)])
        # +name:c +"a b": a field term beside a plain phrase
        tb = [e, E_B] if i < 3 else cut(c.text[d], 2)
        out["nt_p"].append([T(E_B if i < 3 else other(c.name[d], ()), MUST, NAME), P(tb, MUST)])
        # +text:"a b" name:"c d"
        out["tp_np"].append([P(tb, MUST, TEXT), P([e, E_B] if i < 3 else cut(c.name[d], 2), SHOULD, NAME)])
        # a Must on a field the phrase (the term) lacks
        out[LACKING].append([
            [P([60, 61], MUST, TEXT), T(0, SHOULD)],
            [P([ab[0], GONE[0]], MUST, NAME), P(ab, SHOULD, NAME)],
            [P([ab[0], GONE[1]], MUST, TEXT), T(1, SHOULD, TEXT)],
            [P([T_ABSENT, 0], MUST, NAME), T(1, MUST)],
            [T(62, MUST, TEXT), P(ab, MUST, NAME)],
            [P(ab, MUST, NAME), P([63, 62], MUST, TEXT)],
        ][i % 6])
        # few distinct scores (count 1-2, a name's 14 lengths): the k-th and (k+1)-th hits tie at the KS
        ta, tb2 = TIE_PAIRS[i % len(TIE_PAIRS)]
        out["tie"].append([P([ta, tb2], SHOULD, NAME)] if i % 2 else
                          [P([ta, tb2], MUST, NAME), T(rare(), MUST_NOT, TEXT)])
    return out
