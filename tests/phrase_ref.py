"""Reference for phrase queries (tantivy 0.24 PhraseQuery / PhraseWeight /
PhraseScorer at slop 0), in numpy f32, from token streams, gap lists, deletions
and statistics.  Written from the semantics in DESIGN.md §11 alone: it calls
nothing of libfugu.

- a field's tokens sit at analyzer positions; a gap entry `i` of a doc means one
  dropped token immediately before the doc's token `i` (it consumes a position);
- the phrase count of a field is the number of positions p with
  tok[p + off_j] == term_j for every j (overlaps count, repeats allowed);
- weight_f = (sum_j idf(df_f(term_j), N), f32, phrase order, from 0.0) * (1 + K1);
- score_f = weight_f * (c / (c + cache_f[fieldnorm_id])), c the count as f32;
- the doc's score is 0.0 + text part + name part, each only when its count > 0;
- N, df and token totals are given (the namespace's current ones, deleted docs
  included); deleted docs are no hits; order: score desc, doc asc.
"""
import ctypes
import ctypes.util

import numpy as np

_libm = ctypes.CDLL(ctypes.util.find_library("m"))
_libm.logf.restype = ctypes.c_float
_libm.logf.argtypes = [ctypes.c_float]

K1 = np.float32(1.2)
B = np.float32(0.75)
F1 = np.float32(1.0)
HALF = np.float32(0.5)
NONE = -1  # a dropped position


def fieldnorm_table():
    """tantivy fieldnorm/code.rs FIELD_NORMS_TABLE: 0..40, then 8 values per doubling step."""
    t = list(range(41))
    x, step = 40, 2
    while len(t) < 256:
        for _ in range(8):
            if len(t) == 256:
                break
            x += step
            t.append(x)
        step *= 2
    return np.array(t, np.uint32)


TABLE = fieldnorm_table()


def fieldnorm_id(n):
    return int(np.searchsorted(TABLE, np.uint32(min(n, 0xFFFFFFFF)), side="right") - 1)


def idf(df, n):
    """ln in f32 is libm's logf (tantivy's f32::ln, as gen_golden.idf): a double log rounded to f32 is another
    float for some arguments (df 5553 of 6000 docs: one ulp), and a weight off by an ulp is every score's bits"""
    x = (np.float32(n - df) + HALF) / (np.float32(df) + HALF)
    return np.float32(_libm.logf(ctypes.c_float(F1 + x)))


def tf_cache(tot, n):
    avgdl = np.float32(tot) / np.float32(n)
    return (K1 * ((F1 - B) + (B * TABLE.astype(np.float32)) / avgdl)).astype(np.float32)


class Field:
    """One field of a corpus laid out by position: `docs` a list of token id
    sequences, `gaps` per doc the ascending token indices a dropped token came
    before (or None)."""

    def __init__(self, docs, gaps=None):
        self.n = len(docs)
        self.len = np.array([len(d) for d in docs], np.int64)  # kept tokens: the fieldnorm's length
        flat, owner = [], []
        for i, d in enumerate(docs):
            g = list(gaps[i]) if gaps is not None and gaps[i] is not None else []
            row = []
            for j, t in enumerate(d):
                row.extend([NONE] * g.count(j))
                row.append(int(t))
            flat.extend(row)
            owner.extend([i] * len(row))
        self.flat = np.array(flat, np.int64)
        self.owner = np.array(owner, np.int64)
        self.fn = np.array([fieldnorm_id(int(x)) for x in self.len], np.int64)

    def df(self, n_terms):
        out = np.zeros(n_terms, np.int64)
        keep = self.flat >= 0
        pairs = np.unique(np.stack([self.owner[keep], self.flat[keep]]), axis=1)
        np.add.at(out, pairs[1], 1)
        return out

    def counts(self, terms, offsets):
        """phrase count per doc [n]"""
        span = int(max(offsets))
        m = len(self.flat) - span
        out = np.zeros(self.n, np.int64)
        if m <= 0:
            return out
        ok = self.owner[:m] == self.owner[span:span + m]
        for t, o in zip(terms, offsets):
            ok &= self.flat[o:o + m] == int(t)
        np.add.at(out, self.owner[:m][ok], 1)
        return out


class Stats:
    """N, token totals and doc frequencies per field (deleted docs included)."""

    def __init__(self, n, tot, df_text, df_name):
        self.n, self.tot, self.df_text, self.df_name = int(n), (int(tot[0]), int(tot[1])), df_text, df_name

    @classmethod
    def of(cls, text, name, n_terms):
        dfn = name.df(n_terms) if name is not None else np.zeros(n_terms, np.int64)
        return cls(text.n, (text.len.sum(), name.len.sum() if name is not None else 0), text.df(n_terms), dfn)


def weight(df, n, terms):
    """Bm25Weight::for_terms: the idfs summed in phrase order, then * (1 + K1)."""
    s = np.float32(0.0)
    for t in terms:
        s = np.float32(s + idf(int(df[t]) if 0 <= t < len(df) else 0, n))
    return np.float32(s * (F1 + K1))


def search(text, name, st, terms, offsets, k, deleted=None):
    """(scores f32 [m], docs [m], counts (text [n], name [n])) of the phrase, m = min(k, hits)."""
    n = text.n
    terms = [int(t) for t in terms]
    ct = text.counts(terms, offsets)
    cn = name.counts(terms, offsets) if name is not None else np.zeros(n, np.int64)
    score = np.zeros(n, np.float32)
    wt, wn = weight(st.df_text, st.n, terms), weight(st.df_name, st.n, terms)
    cache_t = tf_cache(st.tot[0], st.n)
    m = ct > 0
    c = ct[m].astype(np.float32)
    score[m] = score[m] + wt * (c / (c + cache_t[text.fn[m]]))
    if name is not None and (cn > 0).any():
        cache_n = tf_cache(st.tot[1], st.n)
        m = cn > 0
        c = cn[m].astype(np.float32)
        score[m] = score[m] + wn * (c / (c + cache_n[name.fn[m]]))
    hit = (ct > 0) | (cn > 0)
    if deleted is not None:
        hit &= ~np.asarray(deleted, bool)
    docs = np.nonzero(hit)[0]
    order = np.lexsort((docs, -score[docs].astype(np.float64)))[:k]
    docs = docs[order]
    return score[docs], docs.astype(np.uint32), (ct, cn)


# ---------------------------------------------------------------- the test corpora
def kat_corpus():
    """SURVEY Appendix C's corpus plus `a a a`: a=0 b=1 c=2 d=3 e=4."""
    return [[0, 1, 2], [0, 0, 1], [1, 2, 3, 4], [0, 0, 0]]


SEED = 20240611
V = 64
V_TEXT = 60  # ids 60..63 occur in `name` only: a phrase holding one is present only there


class Synth:
    """6000 docs, vocabulary 64, Zipf s = 1, lengths 1-300, names on a third,
    5% deleted, dropped tokens in ~2% of the docs; and 256 phrase queries."""

    def __init__(self, n=6000, seed=SEED):
        r = np.random.default_rng(seed)
        p = 1.0 / np.arange(1, V_TEXT + 1)
        p /= p.sum()
        lens = r.integers(1, 301, n)
        self.text = [r.choice(V_TEXT, int(l), p=p).astype(np.uint32) for l in lens]
        pn = 1.0 / np.arange(1, V + 1)
        pn /= pn.sum()
        perm = np.concatenate([np.arange(60, 64), np.arange(0, 60)])  # the name-only ids are the frequent ones
        self.name = [perm[r.choice(V, int(r.integers(2, 9)), p=pn)].astype(np.uint32) if i % 3 == 0
                     else np.zeros(0, np.uint32) for i in range(n)]
        self.deleted = r.random(n) < 0.05
        self.text_gaps = [None] * n
        for i in np.nonzero(r.random(n) < 0.02)[0]:
            l = len(self.text[i])
            self.text_gaps[i] = sorted(int(x) for x in r.integers(0, l, int(r.integers(1, 3))))
        self.name_gaps = [None] * n
        for i in range(0, n, 150):  # a few names with a dropped token too
            self.name_gaps[i] = [1]
        self.n = n
        self.queries = self._queries(r)

    def _queries(self, r):
        qs = []  # (terms, offsets)
        alive = np.nonzero(~self.deleted)[0]
        plain = [int(i) for i in alive if self.text_gaps[i] is None]

        def cut(doc_tokens, m):
            s = int(r.integers(0, len(doc_tokens) - m + 1))
            return [int(x) for x in doc_tokens[s:s + m]]

        while len(qs) < 192:  # spans cut from alive docs: >= 1 hit each
            m = int(r.integers(2, 6))
            d = plain[int(r.integers(0, len(plain)))]
            if len(self.text[d]) >= m:
                qs.append((cut(self.text[d], m), list(range(m))))
        for _ in range(16):  # random phrases
            m = int(r.integers(2, 6))
            qs.append(([int(x) for x in r.integers(0, V_TEXT, m)], list(range(m))))
        for i in range(12):  # a repeated term
            t = i % 4
            qs.append(([t] * (2 + i % 3), list(range(2 + i % 3))) if i < 8 else ([t, (t + 1) % 4, t], [0, 1, 2]))
        for i in range(12):  # a missing term: past the vocabulary, or FG_TERM_MISSING
            d = plain[int(r.integers(0, len(plain)))]
            sp = cut(self.text[d], 2) if len(self.text[d]) >= 2 else [0, 1]
            qs.append((sp + [V + 7 if i % 2 else 0xFFFFFFFF], [0, 1, 2]))
        while len(qs) < 244:  # an offset gap: the tokens at p and p + 2 (and p + 3)
            d = plain[int(r.integers(0, len(plain)))]
            if len(self.text[d]) >= 4:
                sp = cut(self.text[d], 4)
                qs.append(([sp[0], sp[2], sp[3]], [0, 2, 3]) if len(qs) % 2 else ([sp[0], sp[2]], [0, 2]))
        named = [int(i) for i in alive if len(self.name[i]) >= 2 and self.name_gaps[i] is None]
        while len(qs) < 256:  # present only in `name`
            d = named[int(r.integers(0, len(named)))]
            m = min(len(self.name[d]), int(r.integers(2, 4)))
            sp = cut(self.name[d], m)
            if max(sp) >= V_TEXT:
                qs.append((sp, list(range(m))))
        return qs

    def csr(self, docs, gaps, lo=0, hi=None):
        """(off u64, tok u32, gap u64) of docs[lo:hi]: the fg_docs_input arrays"""
        hi = len(docs) if hi is None else hi
        off = np.cumsum([0] + [len(d) for d in docs[lo:hi]]).astype(np.uint64)
        tok = np.concatenate([np.zeros(0, np.uint32)] + list(docs[lo:hi])).astype(np.uint32)
        gap = [int(off[i - lo]) + g for i in range(lo, hi) if gaps[i] is not None for g in gaps[i]]
        return off, tok, np.array(gap, np.uint64)

    def batch(self, queries=None):
        """(q_off, terms, phrase_len, phrase_pos) of the queries"""
        queries = self.queries if queries is None else queries
        q_off = np.cumsum([0] + [len(t) for t, _ in queries]).astype(np.uint32)
        terms = np.array([x for t, _ in queries for x in t], np.uint32)
        plen = np.array([len(t) if j == 0 else 0 for t, _ in queries for j in range(len(t))], np.uint32)
        ppos = np.array([x for _, o in queries for x in o], np.uint32)
        return q_off, terms, plen, ppos
