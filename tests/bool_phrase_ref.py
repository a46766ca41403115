"""Reference for queries that hold a phrase clause beside other clauses
(DESIGN.md §14), in numpy f32: composed from phrase_ref (a phrase clause's
per-doc scores: the forward-index count per field, Bm25Weight::for_terms, summed
from 0.0 text then name) and bool_ref (a term clause's per-doc scores, the
per-segment cost counts, and `Corpus._match`, which joins the clause arrays
unchanged).  It calls nothing of libfugu.

A query is a list of clauses (terms, offsets, occur): one term is a term clause,
several a phrase.  Per clause a per-doc f32 array (-1: absent) and a cost:
  * a term clause: bool_ref.Corpus.clause, cost = its docs in the text list plus
    those in the name list, inside the segment;
  * a phrase clause: phrase_ref.search at k = n; cost = the sum over the two
    fields of the smallest count, inside the segment, among its terms' lists of
    that field (0 when some term has none there).
A segment lacking a term of a clause sees that clause absent on all its docs,
which is what dropping a Should / MustNot clause, or emptying the query for a
Must one, amounts to.  Deleted docs never hit; order (score desc, doc asc).
"""
import numpy as np

import bool_ref as br
import phrase_ref as pr

MUST, SHOULD, MUST_NOT = br.MUST, br.SHOULD, br.MUST_NOT
MISSING = br.MISSING
F = np.float32


class _Clauses(br.Corpus):
    """Prepared clause arrays behind bool_ref.Corpus's interface, so Corpus._match
    itself joins them: 'term' c of the query it is given is clause c."""

    def __init__(self, n, arrays):
        self.n, self.n_terms, self.arrays = n, len(arrays), arrays

    def clause(self, t, st):
        return self.arrays[t]


class Ref:
    def __init__(self, n_terms, text, text_gaps=None, name=None, name_gaps=None, deleted=None):
        self.n, self.n_terms = len(text), n_terms
        self.text = pr.Field(text, text_gaps)
        self.name = pr.Field(name, name_gaps) if name is not None else None
        csr = lambda docs: (np.cumsum([0] + [len(d) for d in docs]).astype(np.int64),  # noqa: E731
                            np.concatenate([np.zeros(0, np.int64)] + [np.asarray(d, np.int64) for d in docs]))
        to, tt = csr(text)
        no, nt = csr(name) if name is not None else (None, None)
        self.corpus = br.Corpus(n_terms, to, tt, no, nt)
        self.deleted = np.zeros(self.n, bool) if deleted is None else np.asarray(deleted, bool)
        self.pstats = pr.Stats.of(self.text, self.name, n_terms)
        self._bst, self._memo, self._pref = {}, {}, {}

    def _bstats(self, st):
        if id(st) not in self._bst:
            self._bst[id(st)] = (br.Stats(st.n, st.tot, np.asarray(st.df_text), np.asarray(st.df_name)), st)
        return self._bst[id(st)][0]

    def _prefix(self, t, f):
        """docs < d in term t's list of field f, for every d [n + 1]"""
        if (t, f) not in self._pref:
            cnt = np.zeros(self.n + 1, np.int64)
            if 0 <= t < self.n_terms:
                cnt[self.corpus.docs(t, f) + 1] = 1
            self._pref[(t, f)] = np.cumsum(cnt)
        return self._pref[(t, f)]

    def clause(self, terms, offsets, st):
        """(scores [n] f32, -1 where absent; cost(lo, hi))"""
        terms = [int(t) for t in terms]
        key = (tuple(terms), tuple(int(o) for o in offsets), id(st))
        if key in self._memo:
            return self._memo[key]
        if len(terms) == 1:
            t = terms[0]
            if t < self.n_terms:
                s, pre = self.corpus.clause(t, self._bstats(st))
            else:
                s, pre = np.full(self.n, F(-1.0)), np.zeros(self.n + 1, np.int64)
            cost = lambda lo, hi: int(pre[hi] - pre[lo])  # noqa: E731
        else:
            ps, pd, _ = pr.search(self.text, self.name, st, terms, offsets, self.n)
            s = np.full(self.n, F(-1.0))
            s[pd] = ps
            pres = [[self._prefix(t, f) for t in terms] for f in (0, 1)]
            cost = lambda lo, hi: sum(min(int(p[hi] - p[lo]) for p in pf) for pf in pres)  # noqa: E731
        self._memo[key] = (s, cost)
        return self._memo[key]

    def conj_clause(self, terms, st):
        """the phrase replaced by the conjunction of its terms (hit sets only)"""
        on = np.ones(self.n, bool)
        for t in terms:
            on &= self.clause([t], [0], st)[0] >= 0
        return np.where(on, F(1.0), F(-1.0)), (lambda lo, hi: 0)

    def hits(self, query, seg_bounds=None, stats=None, deleted=None, as_conj=False):
        """(docs, scores) of every hit"""
        st = stats or self.pstats
        dele = self.deleted if deleted is None else np.asarray(deleted, bool)
        bounds = [0, self.n] if seg_bounds is None else [int(b) for b in seg_bounds]
        cl = [self.conj_clause(t, st) if as_conj and len(t) > 1 else self.clause(t, o, st) for t, o, _ in query]
        occur = [int(oc) for _, _, oc in query]
        ds, ss = [], []
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            arrays = []
            for s, cost in cl:  # the cost as a prefix that differs by it across [lo, hi)
                pre = np.zeros(self.n + 1, np.int64)
                pre[hi:] = cost(lo, hi) if hi > lo else 0
                arrays.append((s, pre))
            m, sc = br.Corpus._match(_Clauses(self.n, arrays), list(range(len(cl))), occur, lo, hi, None, True)
            d = np.flatnonzero(m & ~dele[lo:hi])
            ds.append(d + lo)
            ss.append(sc[d])
        return np.concatenate(ds), np.concatenate(ss).astype(F)

    def search(self, query, k, **kw):
        """top k by (score desc, doc asc): (scores f32, docs)"""
        d, s = self.hits(query, **kw)
        o = np.lexsort((d, -s))[:k]
        return s[o], d[o]


def of_synth(c, deleted=None):
    return Ref(pr.V, c.text, c.text_gaps, c.name, c.name_gaps, c.deleted if deleted is None else deleted)


def T(t, oc):
    return ([int(t)], [0], oc)


def P(terms, oc, offsets=None):
    return ([int(t) for t in terms], list(range(len(terms))) if offsets is None else list(offsets), oc)


def batch(queries):
    """(q_off, terms, occur, phrase_len, phrase_pos) of the queries: the fg_query_batch arrays"""
    q_off = np.cumsum([0] + [sum(len(t) for t, _, _ in q) for q in queries]).astype(np.uint32)
    terms = np.array([x for q in queries for t, _, _ in q for x in t], np.uint32)
    occur = np.array([oc for q in queries for t, _, oc in q for _ in t], np.uint8)
    plen = np.array([len(t) if j == 0 else 0 for q in queries for t, _, _ in q for j in range(len(t))], np.uint32)
    ppos = np.array([x for q in queries for _, o, _ in q for x in o], np.uint32)
    return q_off, terms, occur, plen, ppos


# every kind but mt_sp: a phrase clause decides which docs hit (the generator's conditions in
# test_bool_phrase_ref.py; a Should phrase beside a Must term only adds score)
DECIDING = ("sp_st", "sp_sp", "mp_mt", "mp_mp", "mp_st", "mt_xp", "st_st_xp", "name", "missing", "repeat", "t16")
KINDS = DECIDING + ("mt_sp",)
PER_KIND = 16


def queries(c, per_kind=PER_KIND, seed=77):
    """{kind: [query]} on a phrase_ref.Synth: phrases cut from alive gap-free docs, Should
    phrases paired with rarer terms (ids >= 40) so the top-k is not one dense list's."""
    r = np.random.default_rng(seed)
    alive = np.nonzero(~c.deleted)[0]
    plain = [int(i) for i in alive if c.text_gaps[i] is None and len(c.text[i]) >= 12]
    named = [int(i) for i in alive if len(c.name[i]) >= 2 and c.name_gaps[i] is None and max(c.name[i]) >= pr.V_TEXT]

    def doc():
        return c.text[plain[int(r.integers(0, len(plain)))]]

    def cut(toks, m, lo=0, hi=None):
        hi = len(toks) if hi is None else hi
        s = int(r.integers(lo, hi - m + 1))
        return [int(x) for x in toks[s:s + m]]

    def rare():
        return int(r.integers(40, pr.V_TEXT))

    def other(toks, avoid):
        cand = [int(x) for x in toks if int(x) not in avoid]
        return cand[int(r.integers(0, len(cand)))] if cand else int(toks[0])

    out = {k: [] for k in KINDS}
    for i in range(per_kind):
        m = 2 + i % 2
        d = doc()
        out["sp_st"].append([P(cut(d, m), SHOULD), T(rare(), SHOULD)])
        out["sp_sp"].append([P(cut(d, m), SHOULD), P(cut(doc(), 2), SHOULD)])
        d = doc()
        ph = cut(d, m)
        out["mp_mt"].append([P(ph, MUST), T(other(d, ph), MUST)])
        d = doc()
        h = len(d) // 2
        out["mp_mp"].append([P(cut(d, m, 0, h), MUST), P(cut(d, 2, h), MUST)])
        out["mp_st"].append([P(cut(doc(), m), MUST), T(rare(), SHOULD)])
        d = doc()
        ph = cut(d, m)
        out["mt_sp"].append([T(other(d, ph), MUST), P(ph, SHOULD)])
        d = doc()
        ph = cut(d, 2)
        out["mt_xp"].append([T(other(d, ph), MUST), P(ph, MUST_NOT)])
        d = doc()
        ph = cut(d, 2)
        out["st_st_xp"].append([T(other(d, ph), SHOULD), T(rare(), SHOULD), P(ph, MUST_NOT)])
        nm = c.name[named[int(r.integers(0, len(named)))]]
        while True:
            ph = cut(nm, 2)
            if max(ph) >= pr.V_TEXT:
                break
        out["name"].append([P(ph, MUST if i % 2 else SHOULD), T(rare() if i % 4 < 2 else ph[0], SHOULD)])
        # a clause with a missing term (FG_TERM_MISSING / past the vocabulary), as Must, Should, MustNot
        gone = MISSING if i % 2 else pr.V + 7
        oc = (MUST, SHOULD, MUST_NOT, SHOULD)[(i + i // 4) % 4]  # (a missing Must empties the query: one in four)
        d = doc()
        miss = T(gone, oc) if i % 4 < 2 else P(cut(d, 2) + [gone], oc)
        out["missing"].append([P(cut(d, 2), MUST if oc != MUST and i % 2 else SHOULD), miss, T(int(d[0]), SHOULD)])
        # a term repeated in a phrase and present as its own clause
        t = i % 4
        ph = [t, t] if i % 3 == 0 else [t, (t + 1) % 4, t] if i % 3 == 1 else [t, t, t]
        # (both Should, one query in four, is the term's list: the phrase decides nothing there)
        out["repeat"].append([[P(ph, MUST), T(t, SHOULD)], [P(ph, MUST), T(t, MUST)], [T(t, MUST), P(ph, MUST_NOT)],
                              [P(ph, SHOULD), T(t, SHOULD)]][(i // 4 + i) % 4])
        # 16 terms: a phrase of 5 and one of 4 and seven term clauses
        d = doc()
        q16 = [P(cut(d, 5), MUST if i % 2 else SHOULD), P(cut(doc(), 4), SHOULD)]
        q16 += [T(rare() if j % 2 else int(r.integers(0, 40)), MUST_NOT if (j == 6 and i % 4 == 0) else SHOULD)
                for j in range(7)]
        out["t16"].append(q16)
    return out
