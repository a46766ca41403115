"""Reference for fg_count_batch with phrase and group clauses (fg_count_clauses,
DESIGN.md §17), written from the specification alone: plain numpy set algebra
over per-doc boolean masks, nothing of libfugu.

A query is (clauses, filter).  A clause is (kind, occur, terms, offsets):
  T(oc, t)                 a term          -- the docs of its merged (text U name) list
  P(oc, terms, offsets)    a phrase        -- the docs where, in the text field or in
                                              the name field, some start s has
                                              field[s + offsets[j]] == terms[j] for every j,
                                              all inside that doc's field: phrase_ref.Field.counts > 0
  ANY(oc, terms)           an any-of group -- the union of its members' term sets
  ALL(oc, terms)           an all-of group -- the intersection of its members' term sets
occur 0 Must, 1 Should, 2 MustNot; a term None is a term the dictionary lacks.

A clause can be ABSENT: a term the corpus lacks; a phrase with such a term; an
any-of group drops such members and is absent when none is left; an all-of group
with one is absent.  The match set is count_ref's rule over clause doc sets: with
a Must clause the intersection of the Must sets (an absent Must: nothing), else
the union of the present Should sets; minus every present MustNot set; no positive
clause: nothing; then the facet union when the query has facet clauses; alive
docs only.  total = |match|, count[j] = |match & facet postings(count_terms[j])|.
Snapshots hold disjoint docs and absence amounts to the empty set, so totals and
counts over several snapshots are the sums (count_segments).
"""
from __future__ import annotations

import numpy as np

import count_ref as cr
import phrase_ref as pr

MUST, SHOULD, MUST_NOT = cr.MUST, cr.SHOULD, cr.MUST_NOT
FLAG = {"any": 0x80000000, "all": 0x40000000}  # fugu.h FG_CLAUSE_ANY / FG_CLAUSE_ALL
MISSING = 0xFFFFFFFF


def T(oc, t):
    return ("t", oc, [t], [0])


def P(oc, terms, offsets=None):
    return ("p", oc, list(terms), list(range(len(terms))) if offsets is None else list(offsets))


def ANY(oc, terms):
    return ("any", oc, list(terms), [0] * len(terms))


def ALL(oc, terms):
    return ("all", oc, list(terms), [0] * len(terms))


class Corpus(cr.Corpus):
    """count_ref.Corpus (token lists per field, facet paths, deleted flags) with the
    fields laid out by position: text_gaps / name_gaps per doc the ascending token
    indices a dropped token came before (phrase_ref.Field), or None."""

    def __init__(self, text, name, facets, deleted, n_terms, text_gaps=None, name_gaps=None, fdict=None):
        super().__init__(text, name, facets, deleted, n_terms, fdict)
        self.text_gaps = [None] * self.n if text_gaps is None else text_gaps
        self.name_gaps = [None] * self.n if name_gaps is None else name_gaps
        self.ftext = pr.Field(text, self.text_gaps)
        self.fname = pr.Field([nm or [] for nm in name], self.name_gaps)
        self.alive_mask = self.deleted == 0

    def slice(self, a, b, deleted=None):
        return Corpus(self.text[a:b], self.name[a:b], self.facets[a:b], self.deleted[a:b] if deleted is None else deleted,
                      self.n_terms, self.text_gaps[a:b], self.name_gaps[a:b], self.fdict)

    def gaps_csr(self):
        """(text_gaps, name_gaps) as fg_docs_input takes them: ascending indices into text_tok / name_tok"""
        out = []
        for docs, gaps in ((self.text, self.text_gaps), ([nm or [] for nm in self.name], self.name_gaps)):
            off = np.cumsum([0] + [len(d) for d in docs])
            out.append(np.array([int(off[i]) + g for i in range(self.n) if gaps[i] is not None for g in gaps[i]], np.uint64))
        return out

    def mask(self, docs):
        m = np.zeros(self.n, bool)
        if docs:
            m[np.fromiter(docs, np.int64, len(docs))] = True
        return m

    def present(self, t):
        return t is not None and t in self.post


def clause_set(c: Corpus, clause):
    """the clause's docs as a mask [n], or None when the clause is absent"""
    kind, _, terms, offsets = clause
    if kind == "t":
        return c.mask(c.post[terms[0]]) if c.present(terms[0]) else None
    if kind == "p":
        if not all(c.present(t) for t in terms):
            return None
        return (c.ftext.counts(terms, offsets) > 0) | (c.fname.counts(terms, offsets) > 0)
    sets = [c.mask(c.post[t]) for t in terms if c.present(t)]
    if kind == "any":
        return np.logical_or.reduce(sets) if sets else None
    return np.logical_and.reduce(sets) if len(sets) == len(terms) else None


def match_mask(c: Corpus, clauses, flt):
    none = np.zeros(c.n, bool)
    union = lambda ts: np.logical_or.reduce([c.mask(c.fpost.get(t, ())) for t in ts] + [none])  # noqa: E731
    if clauses:
        sets = [(cl[1], clause_set(c, cl)) for cl in clauses]
        must = [s for oc, s in sets if oc == MUST]
        should = [s for oc, s in sets if oc == SHOULD and s is not None]
        if must:
            if any(s is None for s in must):
                return none
            m = np.logical_and.reduce(must)
        elif should:
            m = np.logical_or.reduce(should)
        else:
            return none
        for oc, s in sets:
            if oc == MUST_NOT and s is not None:
                m = m & ~s
        if flt:
            m = m & union(flt)
    elif flt:
        m = union(flt)
    else:
        m = np.ones(c.n, bool)
    return m & c.alive_mask


def count_batch(c: Corpus, queries, count_terms):
    """(total [nq], count [nq, n_count]) as uint64"""
    total = np.zeros(len(queries), np.uint64)
    count = np.zeros((len(queries), len(count_terms)), np.uint64)
    fm = [c.mask(c.fpost.get(t, ())) for t in count_terms]
    for i, (clauses, flt) in enumerate(queries):
        m = match_mask(c, clauses, flt)
        total[i] = m.sum()
        for j, f in enumerate(fm):
            count[i, j] = (m & f).sum()
    return total, count


def count_segments(c: Corpus, bounds, queries, count_terms):
    """the same over the docs as snapshots [bounds[i], bounds[i + 1]): summed"""
    parts = [count_batch(c.slice(a, b), queries, count_terms) for a, b in zip(bounds[:-1], bounds[1:])]
    return sum(p[0] for p in parts), sum(p[1] for p in parts)


def batch_arrays(queries):
    """(q_off, terms, occur, phrase_len, phrase_pos, f_off, f_terms): the fg_query_batch arrays"""
    q_off, terms, occur, plen, ppos, f_off, f_terms = [0], [], [], [], [], [0], []
    for clauses, flt in queries:
        for kind, oc, ts, offs in clauses:
            terms += [MISSING if t is None else t for t in ts]
            occur += [oc] * len(ts)
            plen += [len(ts) | FLAG.get(kind, 0)] + [0] * (len(ts) - 1)
            ppos += offs
        q_off.append(len(terms))
        f_terms += [MISSING if t is None else t for t in flt or ()]
        f_off.append(len(f_terms))
    u32 = lambda a: np.array(a, np.uint32)  # noqa: E731
    return u32(q_off), u32(terms), np.array(occur, np.uint8), u32(plen), u32(ppos), u32(f_off), u32(f_terms)


# ---------------------------------------------------------------- corpora (seeded)
VOCAB = 64
ZIPF = 50                  # ids 0..49: Zipf(1) in text and names
T2048, T2049 = 50, 51      # merged lists of exactly 2048 and 2049 postings (k_crow's chunk is 2048)
DA, DB = 52, 53            # two dense terms in the same 4100 docs: a whole chunk survives the probes
H1, H2 = 54, 55            # the span docs (SPAN0 ..)
N1, N2 = 60, 61            # in names only
RARE, LACK = 62, 63        # LACK: inside the vocabulary, in no doc
DENSE_DOCS, SPAN0 = 4100, 5000
FULL = 6000                # corpora of at least this many docs carry the special docs


def corpus(n, seed):
    """Zipf text of 1-30 tokens, names on a third of the docs, ~2% of the docs with a
    dropped token, facets /org/{0..4}[/team/{0..2}] and /kind/{a,b}, 5% deleted.
    Always: doc n-1 is alive and ends in `4 5`, doc n-2 is deleted and ends in `4 5`,
    doc n-3 ends in `5 4`; names `60 61` and, reversed, `61 60` on some docs.  With
    n >= FULL also: T2048 / T2049 in exactly that many docs (`50 7` opens a quarter of
    the former, `3 51` ends a quarter of the latter), `52 53` ends every third of the
    first 4100 docs and `53 x 52` the others, and from doc SPAN0 on: `54 55` (field
    length 2), `54 9 55` (3), `54 55` with a token dropped between them (positions 0
    and 2), `55 54 9`."""
    rng = np.random.RandomState(seed)
    w = 1.0 / np.arange(1, ZIPF + 1)
    cdf = np.cumsum(w / w.sum())
    draw = lambda k: np.minimum(np.searchsorted(cdf, rng.random_sample(k)), ZIPF - 1).tolist()  # noqa: E731
    full = n >= FULL
    per = 24 if full else 6
    text, name, facets, tg = [], [], [], [None] * n
    for d in range(n):
        t = draw(int(rng.randint(1, 31)))
        if d % 500 == 3:
            t.insert(0, RARE)
        if len(t) > 4 and rng.random_sample() < 0.02:
            tg[d] = [int(rng.randint(1, len(t)))]
        if full and 100 <= d < 100 + 2 * 2048 and d % 2 == 0:
            t = ([T2048, 7] if d % 8 == 0 else [T2048]) + t
            tg[d] = None
        if full and 101 <= d < 101 + 2 * 2049 and d % 2 == 1:
            t += [3, T2049] if d % 8 == 1 else [T2049]
        if full and d < DENSE_DOCS:
            t += [DA, DB] if d % 3 == 0 else [DB, draw(1)[0], DA]
        text.append(t)
        if d % per == 1:
            name.append([N1, N2])
        elif d % per == per // 2 + 1:
            name.append([N2, N1])
        elif d % 3 == 1:
            name.append(draw(int(rng.randint(1, 4))))
        else:
            name.append(None)
        fl = []
        r = rng.random_sample()
        org, team = int(rng.randint(0, 5)), int(rng.randint(0, 3))
        if r < 0.5:
            fl.append(f"/org/{org}/team/{team}")
        elif r < 0.8:
            fl.append(f"/org/{org}")
        if rng.random_sample() < 0.6:
            fl.append("/kind/" + "ab"[int(rng.randint(0, 2))])
        facets.append(fl)
    deleted = (rng.random_sample(n) < 0.05).astype(np.uint8)
    if full:
        for i, (t, g) in enumerate((([H1, H2], None), ([H1, 9, H2], None), ([H1, H2], [1]), ([H2, H1, 9], None))):
            text[SPAN0 + i], tg[SPAN0 + i], deleted[SPAN0 + i] = t, g, 0
            facets[SPAN0 + i] = ["/org/3", "/kind/a"]  # (inside both filters of query_batch)
    text[n - 1] += [4, 5]
    text[n - 2] += [4, 5]
    text[n - 3] += [5, 4]
    deleted[n - 1], deleted[n - 2] = 0, 1
    return Corpus(text, name, facets, deleted, VOCAB, tg)


def main_corpus():
    return corpus(12007, 20261021)


def query_batch(c: Corpus, full=True):
    """[(label, clauses, filter)]: every clause kind under every occur, beside terms,
    beside each other and alone, absent clauses, then each once more with a filter.
    full=False leaves out the queries on the special docs of corpus(n >= FULL)."""
    M, S, X = MUST, SHOULD, MUST_NOT
    ph = lambda oc: P(oc, [4, 5])  # noqa: E731
    ph2 = lambda oc: P(oc, [1, 0])  # noqa: E731
    anyg = lambda oc: ANY(oc, [2, 6])  # noqa: E731
    allg = lambda oc: ALL(oc, [1, 3])  # noqa: E731
    qs = [
        ("S ph", [ph(S)]), ("M ph", [ph(M)]), ("X ph", [ph(X)]), ("M t X ph", [T(M, 0), ph(X)]),
        ("S t X ph", [T(S, 5), ph(X)]), ("M ph M t", [ph(M), T(M, 0)]), ("M ph S t", [ph(M), T(S, 9)]),
        ("S ph S t", [ph(S), T(S, 30)]), ("M ph X t", [ph(M), T(X, 0)]), ("S ph X t", [ph(S), T(X, 1)]),
        ("M ph M ph2", [ph(M), ph2(M)]), ("S ph S ph2", [ph(S), ph2(S)]), ("M ph X ph2", [ph(M), ph2(X)]),
        ("S ph S ph2 X t X any", [ph(S), ph2(S), T(X, 2), ANY(X, [7, 8])]),
        ("M any M ph", [anyg(M), ph(M)]), ("S any S ph", [anyg(S), ph(S)]), ("M all X ph", [allg(M), ph(X)]),
        ("M ph X any", [ph(M), anyg(X)]), ("M ph M all M t", [ph(M), allg(M), T(M, 0)]),
        ("M t M any", [T(M, 0), anyg(M)]), ("M t M all", [T(M, 2), allg(M)]), ("S any", [anyg(S)]), ("M any", [anyg(M)]),
        ("M all", [allg(M)]), ("S all", [allg(S)]), ("X any", [anyg(X)]), ("X all", [allg(X)]),
        ("S t X any", [T(S, 0), anyg(X)]), ("M t X all", [T(M, 0), allg(X)]), ("M any M all", [anyg(M), allg(M)]),
        ("S any S all S t", [anyg(S), allg(S), T(S, 40)]), ("M any X all", [anyg(M), allg(X)]),
        ("S ph_repeat", [P(S, [0, 0])]), ("M ph_repeat3 M t", [P(M, [0, 1, 0]), T(M, 2)]),
        ("S ph_gap", [P(S, [0, 1], [0, 2])]), ("M ph_long", [P(M, [0, 1], [0, 500])]),
        ("S ph_long S t", [P(S, [0, 1], [0, 500]), T(S, RARE)]),
        ("S ph_name", [P(S, [N1, N2])]), ("M ph_name M t", [P(M, [N1, N2]), T(M, 0)]), ("S t X ph_name", [T(S, N1), P(X, [N1, N2])]),
        ("any rare name", [ANY(S, [RARE, N1])]), ("all name", [ALL(M, [N1, N2])]),
        ("M ph_missing", [P(M, [4, None])]), ("S ph_missing S t", [P(S, [4, None]), T(S, 4)]),
        ("S t X ph_missing", [T(S, 4), P(X, [None, 5])]), ("M ph_lack M t", [P(M, [4, LACK]), T(M, 4)]),
        ("S ph_lack S ph", [P(S, [LACK, 4]), ph(S)]),
        ("M any_member_missing M t", [ANY(M, [8, None]), T(M, 0)]), ("S any_member_lack", [ANY(S, [LACK, 8])]),
        ("M all_member_missing M t", [ALL(M, [8, None]), T(M, 0)]), ("S all_member_lack S t", [ALL(S, [8, LACK]), T(S, 8)]),
        ("M any_absent", [ANY(M, [None, LACK])]), ("S t X any_absent", [T(S, 8), ANY(X, [None, LACK])]),
        ("S any_absent", [ANY(S, [LACK, None])]), ("M t M t", [T(M, 0), T(M, 1)]), ("S t S t X t", [T(S, 2), T(S, 6), T(X, 0)]),
        ("M t_missing M ph", [T(M, None), ph(M)]), ("all dup", [ALL(M, [3, 3])]),
    ]
    if full:
        hole = lambda oc: P(oc, [H1, H2], [0, 2])  # noqa: E731
        qs += [
            ("S ph_hole", [hole(S)]), ("M ph_hole X t", [hole(M), T(X, 9)]), ("S ph_h_adjacent", [P(S, [H1, H2])]),
            ("S ph_dense", [P(S, [DA, DB])]), ("M ph_dense M t", [P(M, [DA, DB]), T(M, 0)]), ("S t X ph_dense", [T(S, DB), P(X, [DA, DB])]),
            ("S ph_2048", [P(S, [T2048, 7])]), ("M ph_2049", [P(M, [3, T2049])]), ("all 2048", [ALL(M, [T2048, 0])]),
            ("all 2049 X ph", [ALL(M, [0, T2049]), P(X, [3, T2049])]), ("any 2048 2049", [ANY(S, [T2048, T2049])]),
            ("M any_2048 M ph_dense", [ANY(M, [T2048, T2049]), P(M, [DA, DB])]),
        ]
    f = c.fid
    flt1, flt3 = [f("/org/3")], [f("/kind/a"), None, f("/org/1/team/2")]
    out = [(lab, cl, None) for lab, cl in qs]
    out += [(lab + "|f", cl, flt3 if i % 2 else flt1) for i, (lab, cl) in enumerate(qs)]
    out += [("M ph|f_missing", [ph(M)], [None]), ("all", [], None), ("facet1", [], [f("/org/2")])]
    return out


EMPTY_BY_DESIGN = ("X ph", "X any", "X all", "M ph_long", "M ph_missing", "M ph_lack M t", "M all_member_missing M t",
                   "M any_absent", "S any_absent", "M t_missing M ph", "M ph|f_missing")


def empty_by_design(label):
    return label in EMPTY_BY_DESIGN or (label.endswith("|f") and label[:-2] in EMPTY_BY_DESIGN)


def phrases_of(queries):
    """the distinct phrase clauses of a query list as (terms, offsets)"""
    seen = []
    for _, clauses, _ in queries:
        for kind, _, terms, offs in clauses:
            if kind == "p" and (terms, offs) not in seen:
                seen.append((terms, offs))
    return seen
