"""Reference for queries with group clauses, in numpy f32,
composed from bool_ref the way bool_phrase_ref is: prepared clause arrays go
behind `_Clauses`, and `bool_ref.Corpus._match` joins them unchanged.  It calls
nothing of libfugu.

A query is a list of clauses (occur, body): body is a term id, or a group
(kind, [term ids]) with kind ANY (the members are all Should: a nested
Should-only BooleanQuery) or ALL (all Must: a nested Must-only one).  One level
of grouping: a group's members are plain terms.

A group gives a doc a score or "absent": the `_match` result of its members taken
as a query of their own over the same segment [lo, hi).
  * ANY: absent when no member matches; the score is the members' scores summed
    from 0.0 in written order, skipping absent members.
  * ALL: absent unless every member matches; the members in (the segment's cost,
    position) order, (s0 + s1) + (0.0 + s2 + ...); the leading `0.0 +` that _match
    adds is a bitwise no-op.
The outer level then treats the group as one clause, by the same `_match`.

Cost, used only for the Must order:
  * a term: its docs in the text list plus those in the name list, inside the
    segment (as bool_ref);
  * an ANY group: the SUM of its members' costs.  This is the project's own
    convention -- it already costs a term, itself a two-field union, as the sum of
    its two lists;
  * an ALL group: the SMALLEST member cost -- the phrase clause's rule, an
    intersection's size hint.
Neither group rule is checked against tantivy here: they are stated as upstream
knowledge, not as checked fact (DESIGN.md §0 row c: parity is unpinned).

A member the segment lacks (or FG_TERM_MISSING, or an id past the vocabulary) is
absent on all its docs: an ANY group goes on without it, an ALL group is absent.
An absent Must clause empties the query in that segment, an absent Should or
MustNot clause drops out; one Should without a Must is that clause as a Must (the
same bits: 0.0 + s either way).  A MustNot group excludes the docs the group
matches.  Deleted docs never hit; order (score desc, doc asc).
"""
import functools

import numpy as np

import bool_ref as br

MUST, SHOULD, MUST_NOT = br.MUST, br.SHOULD, br.MUST_NOT
MISSING = br.MISSING
ANY, ALL = "any", "all"
FLAG = {ANY: 0x80000000, ALL: 0x40000000}  # fugu.h FG_CLAUSE_ANY / FG_CLAUSE_ALL
F = np.float32
hits_of = br.hits_of


class _Clauses(br.Corpus):
    """Prepared clause arrays behind bool_ref.Corpus's interface, so Corpus._match
    itself joins them: 'term' c of the query it is given is clause c."""

    def __init__(self, n, arrays):
        self.n, self.n_terms, self.arrays = n, len(arrays), arrays

    def clause(self, t, st):
        return self.arrays[t]


def T(oc, t):
    return (oc, int(t))


def G(oc, kind, terms):
    return (oc, (kind, [int(t) for t in terms]))


def is_group(body):
    return isinstance(body, tuple)


def flatten(query):
    """the same terms without the grouping: every member a clause of its group's occur"""
    return [(oc, t) for oc, body in query for t in (body[1] if is_group(body) else [body])]


def n_terms_of(query):
    return len(flatten(query))


class Ref:
    def __init__(self, corpus: br.Corpus):
        self.c = corpus
        self.n = corpus.n

    def _term(self, t, st):
        """(scores [n], cost prefix [n + 1]) of a term; one outside the vocabulary is absent everywhere"""
        if 0 <= t < self.c.n_terms:
            return self.c.clause(t, st)
        return np.full(self.n, F(-1.0)), np.zeros(self.n + 1, np.int64)

    def _clause(self, body, lo, hi, st):
        """(scores [n] f32, -1 where absent; the clause's cost inside [lo, hi))"""
        if not is_group(body):
            s, pre = self._term(body, st)
            return s, int(pre[hi] - pre[lo])
        kind, members = body
        costs = [int(p[hi] - p[lo]) for p in (self._term(t, st)[1] for t in members)]
        occ = [SHOULD if kind == ANY else MUST] * len(members)
        m, sc = br.Corpus._match(self.c, members, occ, lo, hi, st, True)
        s = np.full(self.n, F(-1.0))
        s[lo:hi] = np.where(m, sc, F(-1.0))
        return s, (sum(costs) if kind == ANY else min(costs))

    def hits(self, query, seg_bounds=None, stats=None, deleted=None):
        """(docs, scores) of every hit, by segment"""
        st = stats or self.c.own
        alive = self.c.alive if deleted is None else ~np.asarray(deleted, bool)
        bounds = [0, self.n] if seg_bounds is None else [int(b) for b in seg_bounds]
        occur = [int(oc) for oc, _ in query]
        ds, ss = [], []
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            arrays = []
            for _, body in query:  # the cost as a prefix that differs by it across [lo, hi)
                s, cost = self._clause(body, lo, hi, st)
                pre = np.zeros(self.n + 1, np.int64)
                pre[hi:] = cost
                arrays.append((s, pre))
            m, sc = br.Corpus._match(_Clauses(self.n, arrays), list(range(len(query))), occur, lo, hi, None, True)
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
    """(q_off, terms, occur, phrase_len, phrase_pos) of the queries: the fg_query_batch arrays, a group
    as FG_CLAUSE_ANY / FG_CLAUSE_ALL OR-ed onto its member count at its first term, then zeros"""
    q_off, terms, occur, plen = [0], [], [], []
    for q in queries:
        for oc, body in q:
            mem = body[1] if is_group(body) else [body]
            terms += mem
            occur += [oc] * len(mem)
            plen += [len(mem) | FLAG[body[0]] if is_group(body) else 1] + [0] * (len(mem) - 1)
        q_off.append(len(terms))
    return (np.array(q_off, np.uint32), np.array(terms, np.uint32), np.array(occur, np.uint8),
            np.array(plen, np.uint32), np.zeros(len(terms), np.uint32))


# ------------------------------------------------------------------ the corpus of the GPU test
N, V = 12000, 64
# merged list lengths on k_group's edges: a lead chunk is kChunk = 2048 postings, a work item at most
# kPhraseMaxGroup = 4 chunks (8192 postings)
T_LONG, T_2047, T_2048, T_2049, T_FEW, T_ABSENT, T_EVERY = 0, 1, 2, 3, 4, 5, 63
EDGE_LEN = {T_LONG: 8193, T_2047: 2047, T_2048: 2048, T_2049: 2049, T_FEW: 40}
T_LOW = 40           # a rare term whose docs all lie below SEG_CUTS[1]
NAME_ONLY = range(48, 56)      # terms with `name` postings only
NAME_TOO = range(6, 16)        # text terms that are in some of their docs' names too
SEG_CUTS = (0, 3000, 5000, N)  # three segments of unequal size: T_FEW only in the last, T_LOW only in the first
GONE = (MISSING, V + 7)        # FG_TERM_MISSING, an id past the vocabulary


class Synth:
    """<= 12,000 docs over 64 terms with `name` postings, deleted docs and one escaped tf (>= 255)."""

    def __init__(self, seed=20251020):
        r = np.random.default_rng(seed)
        lens = {t: int(r.integers(150, 5000)) for t in range(6, 40)}
        lens.update({t: int(r.integers(20, 300)) for t in range(40, 48)})
        lens.update(EDGE_LEN)
        rows = []  # (doc, term, tf)
        for t, n in sorted(lens.items()):
            lo, hi = (SEG_CUTS[2], N) if t == T_FEW else (0, SEG_CUTS[1]) if t == T_LOW else (0, N)
            d = lo + np.sort(r.choice(hi - lo, n, replace=False))
            tf = r.integers(1, 5, n)
            if t == T_2047:
                tf[7] = 300  # an escaped tf byte
            if t == T_LONG:  # high scores in its first lead chunk only: later chunks fall below a small k's threshold
                tf = np.where(np.arange(n) < 1500, r.integers(3, 5, n), 1)
            rows.append((d, np.full(n, t), tf))
        rows.append((np.arange(N), np.full(N, T_EVERY), np.ones(N, np.int64)))  # no doc is empty
        self.text_off, self.text_tok = self._csr(rows)
        rows = []
        for t in NAME_ONLY:
            n = int(r.integers(50, 1500))
            rows.append((np.sort(r.choice(N, n, replace=False)), np.full(n, t), r.integers(1, 3, n)))
        inv = br._invert(N, self.text_off, self.text_tok)
        for t in NAME_TOO:
            d = br.Corpus._list(inv, t)[0][::3]
            rows.append((d, np.full(len(d), t), r.integers(1, 3, len(d))))
        self.name_off, self.name_tok = self._csr(rows)
        self.deleted = (r.random(N) < 0.03).astype(np.uint8)
        self.corpus = br.Corpus(V, self.text_off, self.text_tok, self.name_off, self.name_tok, self.deleted)

    @staticmethod
    def _csr(rows):
        doc = np.concatenate([np.repeat(d, tf) for d, _, tf in rows]).astype(np.int64)
        tok = np.concatenate([np.repeat(t, tf) for _, t, tf in rows]).astype(np.uint32)
        o = np.argsort(doc, kind="stable")
        off = np.zeros(N + 1, np.uint64)
        off[1:] = np.cumsum(np.bincount(doc, minlength=N))
        return off, tok[o]

    def merged_len(self, t):
        """docs of term t in either field: the length of the list k_group leads from"""
        return len(np.union1d(self.corpus.docs(t, 0), self.corpus.docs(t, 1)))

    def segment(self, lo, hi):
        """(text_off, text_tok, name_off, name_tok) of docs [lo, hi)"""
        out = []
        for off, tok in ((self.text_off, self.text_tok), (self.name_off, self.name_tok)):
            a, b = int(off[lo]), int(off[hi])
            out += [(off[lo:hi + 1] - off[lo]).astype(np.uint64), tok[a:b]]
        return out


@functools.lru_cache(maxsize=None)
def synth():
    return Synth()


# the kinds whose grouping decides which docs hit: the hit set differs from the same terms flattened
DECIDING = ("many_mt", "many_many", "sall_sall", "xall", "miss_any", "miss_all", "repeat", "t16", "name", "tie")
# a Should group beside a Must only adds score; a MustNot any-of group is `-b -c` (an identity of the reference)
KINDS = DECIDING + ("sgrp_must", "xany")
MUST_KINDS = ("many_mt", "many_many")  # the nested sum's bits differ from the flat sum's on a shared doc
PER_KIND = 12
KS = (1, 10, 100, 1000)


def queries(c=None, per_kind=PER_KIND, seed=41):
    """{kind: [query]} on synth(): every kind leads from the edge lists in some query"""
    r = np.random.default_rng(seed)
    edge = [T_2047, T_2048, T_2049, T_LONG, T_FEW]
    mid = list(range(6, 40))
    rare = list(range(40, 48))

    def pick(pool, n=1, avoid=()):
        cand = [t for t in pool if t not in avoid]
        return [int(x) for x in r.choice(cand, n, replace=False)]

    out = {k: [] for k in KINDS}
    for i in range(per_kind):
        e = edge[i % len(edge)]
        a, b, cc, d = pick(mid, 4)
        # Must any-of beside a Must term: one lead, the term's list (an edge list every time)
        out["many_mt"].append([G(MUST, ANY, [a, b] + ([cc] if i % 3 == 0 else [])), T(MUST, e)])
        # two Must any-of groups, no Must term: a pass per member of the cheaper group
        out["many_many"].append([G(MUST, ANY, [e, a] if i % 2 else [a, e, b]), G(MUST, ANY, [T_LONG, cc, d][i % 2:])]
                                + ([T(SHOULD, pick(rare)[0])] if i % 4 == 0 else []))
        # DNF: Should all-of groups, sometimes beside a Should term: a pass per clause
        q = [G(SHOULD, ALL, [e, a]), G(SHOULD, ALL, [b, cc] + ([d] if i % 2 else []))]
        out["sall_sall"].append(q + ([T(SHOULD, pick(rare)[0])] if i % 3 == 0 else []))
        # a Should group beside a Must (term or all-of group): score only
        out["sgrp_must"].append([T(MUST, e) if i % 2 else G(MUST, ALL, [e, T_EVERY]),
                                 G(SHOULD, ANY if i % 4 < 2 else ALL, [a, b, cc][: 2 + i % 2])])
        # MustNot groups
        out["xany"].append([T(SHOULD, e), T(SHOULD, a), G(MUST_NOT, ANY, [b, cc])] if i % 2 else
                           [T(MUST, e), G(MUST_NOT, ANY, [a, b, pick(rare)[0]])])
        out["xall"].append([T(SHOULD, e), T(SHOULD, a), G(MUST_NOT, ALL, [b, T_EVERY])] if i % 2 else
                           [T(MUST, e), G(MUST_NOT, ALL, [a, T_LONG])])
        # a missing member (FG_TERM_MISSING, an id past the vocabulary, a term without postings)
        gone = (GONE + (T_ABSENT,))[i % 3]
        out["miss_any"].append([G(MUST, ANY, [gone, a] if i % 2 else [a, gone, b]), T(MUST, e)] if i % 4 < 2 else
                               [G(SHOULD, ANY, [a, gone]), G(SHOULD, ALL, [e, b])])
        oc = (SHOULD, MUST_NOT, SHOULD, MUST, MUST_NOT, SHOULD)[i % 6]  # (a missing Must empties the query: one in six)
        out["miss_all"].append([T(SHOULD, e), G(oc, ALL, [a, gone] if i % 2 else [gone, a, b])] + (
            [T(SHOULD, cc)] if oc != MUST_NOT else [G(MUST_NOT, ALL, [a, T_EVERY])]))
        # a term repeated in two clauses
        out["repeat"].append([[G(MUST, ANY, [a, e]), T(SHOULD, a), T(MUST, b)],
                              [G(SHOULD, ALL, [a, e]), T(SHOULD, a)],
                              [G(MUST, ANY, [a, e]), G(MUST, ANY, [e, b])],
                              [G(SHOULD, ANY, [a, b]), G(SHOULD, ALL, [a, e]), G(MUST_NOT, ALL, [b, cc])]][i % 4])
        # 16 terms in 4 groups
        ts = pick(mid + rare, 13, avoid=(e,))
        kinds = [(MUST, ANY), (MUST, ANY), (SHOULD, ALL), (MUST_NOT, ALL)] if i % 2 else \
                [(SHOULD, ANY), (SHOULD, ALL), (SHOULD, ALL), (MUST_NOT, ALL)]
        mem = [[e] + ts[0:3], [T_LONG] + ts[3:6], ts[6:10], ts[10:13] + [T_EVERY]]
        out["t16"].append([G(oc_, kd, m) for (oc_, kd), m in zip(kinds, mem)])
        # `name`-field members: name-only terms and terms in both fields
        n1, n2 = pick(list(NAME_ONLY), 2)
        n3, n4 = pick(list(NAME_TOO), 2)
        out["name"].append([[G(MUST, ANY, [n1, n3]), G(MUST, ANY, [n2, n4, a])],
                            [G(SHOULD, ALL, [n3, n4]), G(SHOULD, ALL, [n1, a]), T(SHOULD, n2)],
                            [G(MUST, ALL, [n3, e]), G(SHOULD, ANY, [n1, n2])][::-1] + [G(MUST, ANY, [n4, n1])],
                            [G(MUST, ANY, [n1, n2, n3]), T(MUST, e)]][i % 4])
        # few distinct scores (tf 1-4, small fieldnorm ids): the k-th and (k+1)-th hits tie at the KS
        out["tie"].append([G(MUST, ANY, [e, T_ABSENT]), G(MUST, ANY, [T_EVERY, GONE[0]])] if i % 2 else
                          [G(SHOULD, ALL, [e, T_EVERY]), G(SHOULD, ALL, [T_FEW, T_EVERY])])
    return out
