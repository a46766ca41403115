"""Vectorised brute-force reference of the boolean search (test infrastructure).

Plain numpy over whole per-doc arrays: no cursors, no cost-ordered leapfrog, no
union heap, no pruning -- none of the habits the C oracle (oracle/fugu_oracle.c)
shares with the kernels it checks.  The formulas are those of
tests/golden/gen_golden.py (the restatement pinned to the Appendix C KAT), whose
`weight` / `cache` / `fieldnorm_id` it imports; the combination follows
gen_golden.Index.search_occ / search_filtered:
  * a term's score on a doc: 0.0 + w_text * (tf / (tf + cache_text[fn])) + w_name * (...), f32;
  * Musts in (cost, position) order, (s0 + s1) + (0.0 + s2 + ...); then
    (0.0 + req) + opt when a Should matches; Shoulds alone from 0.0 in clause
    order; MustNot excludes; deleted docs never hit;
  * facet clauses: a union summed from 0.0 in clause order; text + facet, the
    union alone without text terms, 1.0 (AllQuery) without either.
The statistics (N, per-field df, token totals) are arguments (`Stats`, the
fields of native.ShardStats), so a segment scores under its namespace's
statistics and a snapshot under those it was rescored to.  A segmented search
orders the Musts by each segment's own cost; the statistics stay global.
"""
from __future__ import annotations

import os
import sys
from dataclasses import dataclass

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import gen_golden as gg  # noqa: E402

F = np.float32
MUST, SHOULD, MUST_NOT = 0, 1, 2
MISSING = 0xFFFFFFFF


@dataclass
class Stats:
    n_docs: int
    tot_tokens: tuple            # (text, name)
    df_text: np.ndarray
    df_name: np.ndarray
    df_facet: "np.ndarray | None" = None
    tot_facet_tokens: int = 0


def _invert(n_docs, off, tok):
    """(terms, term_off, doc, tf) of one field: postings by (term, doc)."""
    lens = np.diff(np.asarray(off, np.int64))
    key = (np.asarray(tok, np.uint64) << np.uint64(32)) | np.repeat(np.arange(n_docs, dtype=np.uint64), lens)
    key, tf = np.unique(key, return_counts=True)
    term = (key >> np.uint64(32)).astype(np.int64)
    terms, first = np.unique(term, return_index=True)
    return terms, np.append(first, len(key)), (key & np.uint64(0xFFFFFFFF)).astype(np.int64), tf, lens


class Corpus:
    def __init__(self, n_terms, text_off, text_tok, name_off=None, name_tok=None, deleted=None, facets=None):
        """facets: (facet_off, facet_tok, n_facet_terms) or None."""
        self.n, self.n_terms = len(text_off) - 1, n_terms
        self.fld = [_invert(self.n, text_off, text_tok)]
        if name_off is not None:
            self.fld.append(_invert(self.n, name_off, name_tok))
        self.fn = [gg.fieldnorm_id(f[4]) for f in self.fld]
        self.alive = np.ones(self.n, bool) if deleted is None else np.asarray(deleted) == 0
        self.fac, self.n_fterms, ftot = None, 0, 0
        if facets is not None:
            self.fac, self.n_fterms, ftot = _invert(self.n, facets[0], facets[1]), int(facets[2]), len(facets[1])
        df = [np.zeros(n_terms, np.int64), np.zeros(n_terms, np.int64)]
        for f, fl in enumerate(self.fld):
            df[f][fl[0]] = np.diff(fl[1])
        dff = np.zeros(self.n_fterms, np.int64)
        if self.fac is not None:
            dff[self.fac[0]] = np.diff(self.fac[1])
        tot = tuple(int(f[4].sum()) for f in self.fld) + (0,) * (2 - len(self.fld))
        self.own = Stats(self.n, tot, df[0], df[1], dff, ftot)
        self._memo = {}

    @staticmethod
    def _list(inv, t):
        i = np.searchsorted(inv[0], t)
        if i == len(inv[0]) or inv[0][i] != t:
            return np.zeros(0, np.int64), np.zeros(0, np.int64)
        return inv[2][inv[1][i]:inv[1][i + 1]], inv[3][inv[1][i]:inv[1][i + 1]]

    def docs(self, t, field=0):
        return self._list(self.fld[field], t)[0] if field < len(self.fld) else np.zeros(0, np.int64)

    def facet_docs(self, t):
        return self._list(self.fac, t)[0] if self.fac is not None else np.zeros(0, np.int64)

    def clause(self, t, st):
        """(f32 per-doc score, -1 on absent docs; cost prefix: docs < d in the text + name lists)."""
        key = (int(t), id(st))
        if key not in self._memo:
            s = np.zeros(self.n, F)
            cnt = np.zeros(self.n + 1, np.int64)
            on = np.zeros(self.n, bool)
            for f, (fl, dfs) in enumerate(zip(self.fld, (st.df_text, st.df_name))):
                d, tf = self._list(fl, t)
                if len(d) == 0:
                    continue
                w = gg.weight(int(dfs[t]), int(st.n_docs))
                c = gg.cache(F(st.tot_tokens[f]) / F(st.n_docs))[self.fn[f][d]]
                tff = tf.astype(F)
                s[d] = s[d] + w * (tff / (tff + c))
                on[d] = True
                cnt[d + 1] += 1
            s[~on] = F(-1.0)
            self._memo[key] = (s, np.cumsum(cnt), st)  # (st kept: its id is the key)
        return self._memo[key][:2]

    def _facet_union(self, fterms, st):
        fs, any_f = np.zeros(self.n, F), np.zeros(self.n, bool)
        fc1 = gg.cache(F(st.tot_facet_tokens) / F(st.n_docs))[1]  # no fieldnorms: the constant id 1
        for t in fterms:
            d = self.facet_docs(t) if t != MISSING else []
            if len(d):
                fs[d] = fs[d] + gg.weight(int(st.df_facet[t]), int(st.n_docs)) * (F(1.0) / (F(1.0) + fc1))
                any_f[d] = True
        return fs, any_f

    def _match(self, terms, occur, lo, hi, st, with_should):
        """(match mask, score) over docs [lo, hi), text clauses only; None without text terms."""
        nothing = (np.full(self.n, F(-1.0)), np.zeros(self.n + 1, np.int64))  # a term outside the vocabulary
        cl = [self.clause(t, st) if t < self.n_terms else nothing for t in terms]
        M = [c for c, o in zip(cl, occur) if o == MUST]
        S = [c[0][lo:hi] for c, o in zip(cl, occur) if o == SHOULD]
        X = [c[0][lo:hi] for c, o in zip(cl, occur) if o == MUST_NOT]
        n = hi - lo
        if not M and not S:
            return np.zeros(n, bool), np.zeros(n, F)
        opt, any_s = np.zeros(n, F), np.zeros(n, bool)
        if with_should or not M:
            for s in S:
                opt = np.where(s >= 0, opt + s, opt)
                any_s |= s >= 0
        if M:
            M.sort(key=lambda c: c[1][hi] - c[1][lo])  # (the segment's cost, position): the sort is stable
            ms = [c[0][lo:hi] for c in M]
            m = np.logical_and.reduce([s >= 0 for s in ms])
            req = ms[0]
            if len(ms) > 1:
                others = np.zeros(n, F)
                for s in ms[2:]:
                    others = others + s
                req = (ms[0] + ms[1]) + others
            sc = F(0.0) + req
            sc = np.where(any_s, sc + opt, sc)
        else:
            m, sc = any_s, opt
        for s in X:
            m = m & (s < 0)
        return m, sc

    def _hits(self, terms, occur, fterms, seg_bounds, st, with_should=True):
        """(docs, scores) of every hit, by segment."""
        st = st or self.own
        terms = [int(t) for t in terms]
        occur = [int(o) for o in (occur if occur is not None else [MUST] * len(terms))]
        bounds = [0, self.n] if seg_bounds is None else [int(b) for b in seg_bounds]
        fs = any_f = None
        if fterms is not None and len(fterms):
            fs, any_f = self._facet_union([int(t) for t in fterms], st)
        ds, ss = [], []
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            if terms:
                m, sc = self._match(terms, occur, lo, hi, st, with_should)
                if fs is not None:
                    m, sc = m & any_f[lo:hi], sc + fs[lo:hi]
            elif fs is not None:
                m, sc = any_f[lo:hi], fs[lo:hi]
            else:
                m, sc = np.ones(hi - lo, bool), np.ones(hi - lo, F)  # AllQuery
            d = np.flatnonzero(m & self.alive[lo:hi])
            ds.append(d + lo)
            ss.append(sc[d])
        return np.concatenate(ds), np.concatenate(ss).astype(F)

    def search(self, terms, occur, k, fterms=None, seg_bounds=None, stats=None):
        """Top k by (score desc, doc asc): (scores f32, docs)."""
        d, s = self._hits(terms, occur, fterms, seg_bounds, stats)
        o = np.lexsort((d, -s))[:k]
        return s[o], d[o]

    def count(self, terms, occur, fterms=None, count_terms=()):
        """count_batch semantics: (|match|, |match & postings(count term)| per count
        term); with a Must clause the Should clauses are ignored."""
        d, _ = self._hits(terms, occur, fterms, None, None, with_should=False)
        return len(d), [len(np.intersect1d(d, self.facet_docs(int(t)))) if t != MISSING else 0 for t in count_terms]


def hits_of(scores, docs):
    return [[int(d), int(np.float32(s).view(np.uint32))] for s, d in zip(scores, docs)]
