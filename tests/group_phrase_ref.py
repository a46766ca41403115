"""Reference for queries that hold a group clause beside a phrase clause
(DESIGN.md §18), in numpy f32.  Nothing new is stated here: every clause gives a
doc a score or "absent" --
  * a term or a phrase clause by bool_phrase_ref.Ref.clause (§11 / §14: the
    forward-index count per field, Bm25Weight::for_terms, text then name from 0.0;
    cost: the sum over the two fields of the terms' smallest doc count there),
  * a group clause by group_ref.Ref._clause (§15: any-of its present members from
    0.0 in written order, cost the sum; all-of (s0 + s1) + (0.0 + s2 + ...) in
    (cost, position) order, cost the smallest) --
and bool_ref.Corpus._match joins the clause arrays unchanged, per segment, with
the segment's own costs for the Must order.  It calls nothing of libfugu.

A query is a list of clauses (occur, body): body a term id, a group
(ANY | ALL, [term ids]) as group_ref's, or a phrase (PHR, [term ids], [offsets]).
A phrase or all-of group with a term the segment lacks is absent there; an
absent Must empties the query, an absent Should or MustNot drops out.

Two corpora: A = phrase_ref.Synth() (6000 docs of 1 to 300 tokens, names, gaps,
deletions) and B = group_ref.synth() read by position: its docs list their tokens
in ascending term id, each repeated by its tf, so the phrase "t t" (offsets 0, 1)
matches exactly the docs with tf(t) >= 2, with count tf - 1 -- a verified phrase
on the 2047 / 2048 / 2049 / 8193-posting lead lists and on the escaped-tf doc.
"""
import functools

import numpy as np

import bool_phrase_ref as bp
import bool_ref as br
import group_ref as gr
import phrase_ref as pr

MUST, SHOULD, MUST_NOT = br.MUST, br.SHOULD, br.MUST_NOT
M, S, X = MUST, SHOULD, MUST_NOT
MISSING = br.MISSING
ANY, ALL, PHR = gr.ANY, gr.ALL, "phr"
F = np.float32
hits_of = br.hits_of
KS = (1, 10, 100, 1000)


def T(oc, t):
    return (oc, int(t))


def G(oc, kind, terms):
    return (oc, (kind, [int(t) for t in terms]))


def P(oc, terms, offsets=None):
    terms = [int(t) for t in terms]
    return (oc, (PHR, terms, list(range(len(terms))) if offsets is None else [int(o) for o in offsets]))


def is_phrase(body):
    return isinstance(body, tuple) and body[0] == PHR


def is_group(body):
    return isinstance(body, tuple) and body[0] in (ANY, ALL)


def terms_of(body):
    return list(body[1]) if isinstance(body, tuple) else [body]


def n_terms_of(query):
    return sum(len(terms_of(b)) for _, b in query)


def phrases_as_groups(query):
    """every phrase replaced by the all-of group of its terms: what a kernel without positions would match"""
    return [(oc, (ALL, list(b[1]))) if is_phrase(b) else (oc, b) for oc, b in query]


def without_groups(query):
    return [(oc, b) for oc, b in query if not is_group(b)]


def flatten_groups(query):
    """every group member a clause of its group's occur; the phrases stay"""
    return [(oc, t) if is_group(b) else (oc, b) for oc, b in query for t in (b[1] if is_group(b) else [None])]


class Ref:
    def __init__(self, base: bp.Ref):
        self.b, self.g, self.n = base, gr.Ref(base.corpus), base.n

    def _clause(self, body, lo, hi, st):
        """(scores [n] f32, -1 where absent; the clause's cost inside [lo, hi))"""
        if is_phrase(body):
            s, cost = self.b.clause(body[1], body[2], st)
            return s, (cost(lo, hi) if hi > lo else 0)
        return self.g._clause(body, lo, hi, self.b._bstats(st))

    def hits(self, query, seg_bounds=None, stats=None, deleted=None):
        """(docs, scores) of every hit, by segment"""
        st = stats or self.b.pstats
        dele = self.b.deleted if deleted is None else np.asarray(deleted, bool)
        bounds = [0, self.n] if seg_bounds is None else [int(x) for x in seg_bounds]
        occur = [int(oc) for oc, _ in query]
        ds, ss = [], []
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            arrays = []
            for _, body in query:  # the cost as a prefix that differs by it across [lo, hi)
                s, cost = self._clause(body, lo, hi, st)
                pre = np.zeros(self.n + 1, np.int64)
                pre[hi:] = cost
                arrays.append((s, pre))
            m, sc = br.Corpus._match(gr._Clauses(self.n, arrays), list(range(len(query))), occur, lo, hi, None, True)
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
    """(q_off, terms, occur, phrase_len, phrase_pos) of the queries: the fg_query_batch arrays; a group as
    group_ref.batch writes it, a phrase as bool_phrase_ref.batch does"""
    q_off, terms, occur, plen, ppos = [0], [], [], [], []
    for q in queries:
        for oc, body in q:
            mem = terms_of(body)
            terms += mem
            occur += [oc] * len(mem)
            plen += [len(mem) | gr.FLAG[body[0]] if is_group(body) else len(mem)] + [0] * (len(mem) - 1)
            ppos += list(body[2]) if is_phrase(body) else [0] * len(mem)
        q_off.append(len(terms))
    return (np.array(q_off, np.uint32), np.array(terms, np.uint32), np.array(occur, np.uint8),
            np.array(plen, np.uint32), np.array(ppos, np.uint32))


# ------------------------------------------------------------------ the two corpora
class World:
    """A corpus by position (text / name token lists, gaps, deletions), its reference and the generator's pools"""

    def __init__(self, name, V, text, text_gaps, namef, name_gaps, deleted, pools, cuts):
        self.name, self.V, self.text, self.text_gaps, self.namef, self.name_gaps = name, V, text, text_gaps, namef, name_gaps
        self.deleted = np.asarray(deleted, bool)
        self.n = len(text)
        self.base = bp.Ref(V, text, text_gaps, namef, name_gaps, self.deleted)
        self.ref = Ref(self.base)
        self.pools = pools      # "mid", "rare", "name_only": term ids
        self.cuts = cuts        # three unequal segments, one lacking a term

    def csr(self, lo=0, hi=None):
        """((text_off, text_tok, V, name_off, name_tok), dict(text_gaps, name_gaps)) of docs [lo, hi): Index.from_docs"""
        hi = self.n if hi is None else hi
        out, gaps = [], []
        for docs, gp in ((self.text, self.text_gaps), (self.namef, self.name_gaps)):
            off = np.cumsum([0] + [len(d) for d in docs[lo:hi]]).astype(np.uint64)
            tok = np.concatenate([np.zeros(0, np.uint32)] + [np.asarray(d, np.uint32) for d in docs[lo:hi]]).astype(np.uint32)
            out += [off, tok]
            gaps.append(np.array([int(off[i - lo]) + g for i in range(lo, hi) if gp[i] is not None for g in gp[i]], np.uint64))
        return (out[0], out[1], self.V, out[2], out[3]), dict(text_gaps=gaps[0], name_gaps=gaps[1])


# A as three unequal segments: the first is so short that it lacks some of the rarer terms the queries use
SEG_CUTS_A = (0, 5, 2500, 6000)


@functools.lru_cache(maxsize=None)
def world_a():
    c = pr.Synth()
    pools = dict(mid=list(range(8, 40)), rare=list(range(40, pr.V_TEXT)), name_only=list(range(pr.V_TEXT, pr.V)))
    return World("A", pr.V, c.text, c.text_gaps, c.name, c.name_gaps, c.deleted, pools, SEG_CUTS_A)


@functools.lru_cache(maxsize=None)
def world_b():
    c = gr.synth()
    rows = lambda off, tok: [tok[int(off[i]):int(off[i + 1])] for i in range(gr.N)]  # noqa: E731
    none = [None] * gr.N
    pools = dict(mid=list(range(6, 40)), rare=list(range(40, 48)), name_only=list(gr.NAME_ONLY))
    return World("B", gr.V, rows(c.text_off, c.text_tok), none, rows(c.name_off, c.name_tok), none, c.deleted != 0, pools,
                 gr.SEG_CUTS)


def world(name):
    return {"A": world_a, "B": world_b}[name]()


# ------------------------------------------------------------------ the queries
# the kinds whose phrase AND whose group decide which docs hit (the generator's conditions, below)
DECIDING = ("mp_many", "mp_mall", "sp_sany", "sany_sp", "sp_sall", "xp_many", "xany_mp", "two_p", "repeat", "name", "t16",
            "pos_edge", "lead_edge")
# many_sp: the Should phrase only adds score; miss: a clause with a missing term; tie: the k-th and (k+1)-th hits tie
KINDS = DECIDING + ("many_sp", "miss", "tie")
MUST_KINDS = ("mp_many", "mp_mall")  # the nested sum's bits differ from the flat sum's on a shared doc
ONLY_ON = {"pos_edge": "A", "lead_edge": "B"}
PER_KIND = 8
EDGE_TERMS = (gr.T_2047, gr.T_2048, gr.T_2049, gr.T_LONG)
# FG_TERM_MISSING, an id past both vocabularies, (B) a term without postings
GONE = {"A": (MISSING, 64 + 7), "B": (MISSING, 64 + 7, gr.T_ABSENT)}
POS_EDGE_FORMS = ("late", "last", "next_doc")


def kinds_of(name):
    return [k for k in KINDS if ONLY_ON.get(k, name) == name]


def hit_set(ref, q):
    return set(ref.hits(q)[0].tolist())


def decides(ref, q):
    """the verification decides, and so do the groups"""
    h = hit_set(ref, q)
    return bool(h) and h != hit_set(ref, phrases_as_groups(q)) and h != hit_set(ref, without_groups(q))


def holds_all_not_phrase_hits(w, q):
    """a doc that holds every term of the (first) phrase, does not match it, and is a hit (through the group)"""
    ph = next(b for _, b in q if is_phrase(b))
    st = w.base.pstats
    on = np.logical_and.reduce([w.base.clause([t], [0], st)[0] >= 0 for t in ph[1]])
    hit = np.zeros(w.n, bool)
    hit[w.ref.hits(q)[0]] = True
    return bool((on & (w.base.clause(ph[1], ph[2], st)[0] < 0) & hit).any())


def ties(ref, q):
    s = ref.search(q, 1001)[0]
    return any(len(s) > k and s[k - 1] == s[k] for k in (10, 100))


def starts_of(doc, terms):
    """the positions of a gap-free doc where the consecutive phrase starts"""
    m = len(terms)
    return [p for p in range(len(doc) - m + 1) if all(int(doc[p + j]) == terms[j] for j in range(m))]


def pos_edge_form(w, q):
    """which of POS_EDGE_FORMS the query shows (its phrase is consecutive), or None"""
    ph = next(b for _, b in q if is_phrase(b))[1]
    hits = hit_set(w.ref, q)
    out = set()
    for d in sorted(hits):
        if w.text_gaps[d] is not None:
            continue
        st = starts_of(w.text[d], ph)
        if st and min(st) >= 64 and not starts_of(w.namef[d], ph):
            out.add("late")
        if st and st[-1] + len(ph) == len(w.text[d]):
            out.add("last")
    for d in range(w.n - 1):  # the phrase over the seam of docs d, d + 1 and nowhere inside d: d must not hit
        if w.deleted[d] or w.text_gaps[d] is not None or w.text_gaps[d + 1] is not None or len(w.text[d + 1]) == 0:
            continue
        for cut in range(1, len(ph)):
            a, b = ph[:cut], ph[cut:]
            if len(w.text[d]) >= len(a) and len(w.text[d + 1]) >= len(b) and \
                    [int(x) for x in w.text[d][len(w.text[d]) - len(a):]] == a and [int(x) for x in w.text[d + 1][:len(b)]] == b \
                    and not starts_of(w.text[d], ph) and not starts_of(w.namef[d], ph) and d not in hits \
                    and d in hit_set(w.ref, phrases_as_groups(q)):
                out.add("next_doc")
    return out


LONG_LEAD = 7   # lead_edge[7] on B: -"u u" +(T_LONG a), a pass over the 8193-posting list whose later chunks score low
KCHUNK = 2048   # fg_internal.h kChunk: the postings of a lead chunk


def long_lead_bound(w, q, k):
    """For q = [P(X, ...), G(M, ANY, [T_LONG, a])] on B, in the reference's numbers: (whether some later chunk of the
    pass over T_LONG's list is skipped at the exact k-th score, the chunks' bounds, the k-th score).  A chunk's bound
    is the score sum over upper bounds, 0.0 + ((0.0 + max T_LONG score in the chunk) + max score of a), times 1 + 2^-17."""
    (_, ph), (_, (_, (e, a))) = q
    assert e == gr.T_LONG and is_phrase(ph)
    st = w.base._bstats(w.base.pstats)
    se, sa = (w.base.corpus.clause(t, st)[0] for t in (e, a))
    lead = np.flatnonzero(se >= 0)
    z = F(0.0)
    bounds = [F(F(z + F(F(z + se[lead[c:c + KCHUNK]].max()) + sa.max())) * F(1.00000762939453125))
              for c in range(0, len(lead), KCHUNK)]
    s = w.ref.search(q, k)[0]
    kth = s[k - 1] if len(s) >= k else z
    return any(b < kth for b in bounds[1:]), bounds, kth


def pos_edge_doc(w, q, form, d):
    """whether doc d shows `form` for query q (its phrase is consecutive)"""
    ph = next(b for _, b in q if is_phrase(b))[1]
    st = starts_of(w.text[d], ph)
    hit = d in hit_set(w.ref, q)
    if form == "late":
        return hit and bool(st) and min(st) >= 64 and not starts_of(w.namef[d], ph)
    if form == "last":
        return hit and bool(st) and st[-1] + len(ph) == len(w.text[d])
    return not hit and not st and not starts_of(w.namef[d], ph) and d in hit_set(w.ref, phrases_as_groups(q))


@functools.lru_cache(maxsize=None)
def queries(name, per_kind=PER_KIND, seed=4118):
    """{kind: [query]} on world(name).  A candidate of a deciding kind is drawn again until it meets the kind's
    condition (test_group_phrase_ref.py states and checks them); the conditions are never lowered."""
    w = world(name)
    ref = w.ref
    r = np.random.default_rng(seed + (name == "B"))
    alive = np.flatnonzero(~w.deleted)
    plain = [int(i) for i in alive if w.text_gaps[i] is None and len(w.text[i]) >= 8]
    named = [int(i) for i in alive if len(w.namef[i]) >= 2 and w.name_gaps[i] is None
             and any(int(t) in w.pools["name_only"] for t in w.namef[i])]
    mid, rare, name_only = w.pools["mid"], w.pools["rare"], w.pools["name_only"]

    target = [0]  # pos_edge: the doc the candidate was cut from

    def doc():
        return plain[int(r.integers(0, len(plain)))]

    def cut(toks, m, lo=0, hi=None):
        hi = len(toks) if hi is None else hi
        s = int(r.integers(lo, hi - m + 1))
        return [int(x) for x in toks[s:s + m]]

    def pick(pool, n=1, avoid=()):
        cand = [t for t in pool if t not in avoid]
        return [int(x) for x in r.choice(cand, n, replace=False)]

    def phrase(i):
        return cut(w.text[doc()], 2 + i % 2)

    def draw(kind, i):
        ph = phrase(i)
        a, b, c3 = pick(mid + rare, 3, avoid=ph)
        if kind == "mp_many":
            return [P(M, ph), G(M, ANY, [a, b] + ([c3] if i % 3 == 0 else []))]
        if kind == "mp_mall":
            return [P(M, ph), G(M, ALL, [a, pick(mid)[0]])] + ([T(S, c3)] if i % 2 else [])
        if kind == "many_sp":
            return [G(M, ANY, [a, b]), P(S, ph)] + ([G(M, ANY, [c3, pick(mid)[0]])] if i % 2 else [])
        if kind == "sp_sany":
            return [P(S, ph), G(S, ANY, [a, b])]
        if kind == "sany_sp":
            return [G(S, ANY, [a, b]), P(S, ph)] + ([T(S, c3)] if i % 2 else [])
        if kind == "sp_sall":
            return [P(S, ph), G(S, ALL, [a, pick(mid)[0]])]
        if kind == "xp_many":
            return [P(X, ph), G(M, ANY, [a, b])] if i % 2 else [P(X, ph), G(S, ANY, [a, b]), T(S, c3)]
        if kind == "xany_mp":
            return [G(X, ANY, [a, b]), P(M, ph)] if i % 2 else [G(X, ALL, [a, b]), P(S, ph), T(S, c3)]
        if kind == "two_p":
            ph2 = phrase(i + 1)
            return [[P(M, ph), P(S, ph2), G(M, ANY, [a, b])], [P(S, ph), P(S, ph2), G(S, ALL, [a, b])],
                    [P(M, ph), P(X, ph2), G(M, ALL, [a, pick(mid)[0]])], [P(S, ph), G(S, ANY, [a, b]), P(X, ph2)]][i % 4]
        if kind == "repeat":  # a term both in a phrase and in a group; "t t"
            t = int(ph[0])
            return [[P(M, [t, t]), G(M, ALL, [t, a])], [P(S, [t, t]), G(S, ALL, [t, a])],
                    [P(X, ph), G(M, ANY, [ph[0], a])], [P(M, [t, t]), G(X, ALL, [t, a]), G(S, ANY, [t, b])]][i % 4]
        if kind == "name":  # a phrase present only in `name`, name-only members
            nm = w.namef[named[int(r.integers(0, len(named)))]]
            while True:
                nph = cut(nm, 2)
                if max(nph) in name_only or min(nph) in name_only:
                    break
            n1, n2 = pick(name_only, 2)
            return [[P(M, nph), G(M, ANY, [n1, a])], [P(S, nph), G(S, ANY, [n1, n2])],
                    [P(S, ph), G(S, ALL, [n1, a]), G(S, ANY, [n2, b])], [P(M, nph), G(X, ANY, [n1, n2]), T(S, a)]][i % 4]
        if kind == "t16":  # 16 terms: phrases of 4 and 3, groups of 4 and 3, two terms
            d = w.text[doc()]
            ts = pick(mid + rare, 9)
            return [P(M if i % 2 else S, cut(d, 4)), P(S, cut(w.text[doc()], 3)), G(M if i % 2 else S, ANY, ts[0:4]),
                    G(S, ALL, ts[4:6] + pick(mid)), T(S, ts[7]), T(X if i % 4 == 0 else S, ts[8])]
        if kind == "tie":  # name fields: few distinct (tf, length) pairs, so few distinct scores
            nph = cut(w.namef[named[int(r.integers(0, len(named)))]], 2)
            return [P(S, nph), G(S, ANY, pick(name_only, 2))] if i % 2 else [P(M, nph), G(M, ANY, pick(name_only, 2))]
        if kind == "miss":  # a missing term in the phrase or in the group, under Must and under Should
            gone = GONE[name][i % len(GONE[name])]
            return [[P(M, ph + [gone]), G(S, ANY, [a, b])], [P(S, ph + [gone]), G(S, ANY, [a, b])],
                    [P(M, ph), G(M, ALL, [a, gone])], [P(S, ph), G(S, ALL, [gone, a]), T(S, b)],
                    [P(M, ph), G(M, ANY, [gone, a])], [P(S, ph), G(S, ANY, [a, gone]), G(X, ALL, [b, gone])]][i % 6]
        if kind == "pos_edge":
            form = POS_EDGE_FORMS[i % 3]
            while True:
                dd = doc()
                toks = w.text[dd]
                if form == "late" and len(toks) >= 70:
                    ph = cut(toks, 3, 64)
                elif form == "last":
                    ph = [int(x) for x in toks[-(2 + i % 2):]]
                elif form == "next_doc" and dd + 1 < w.n and w.text_gaps[dd + 1] is None and len(w.text[dd + 1]) >= 1:
                    ph = [int(toks[-1]), int(w.text[dd + 1][0])]
                else:
                    continue
                break
            target[0] = dd
            others = [int(x) for x in toks if int(x) not in ph and int(x) >= 8] or [int(toks[0])]
            return [P(M, ph), G(M, ANY, [others[int(r.integers(0, len(others)))], pick(rare)[0]])]
        if kind == "lead_edge":  # +"t t" +(a b) for t on each edge list; a group member on an edge list beside "u u"
            e = EDGE_TERMS[i % 4]
            u, a = pick(mid, 2)
            return [P(M, [e, e]), G(M, ANY, [a, b])] if i < 4 else \
                   [G(S, ANY, [e, a]), P(S, [u, u])] if i in (5, 6) else [P(X, [u, u]), G(M, ANY, [e, a])]
        raise KeyError(kind)

    def ok(kind, q, i):
        if kind in ("sp_sany", "sany_sp") and not holds_all_not_phrase_hits(w, q):
            return False
        if kind == "tie":
            return ties(ref, q)
        if kind == "lead_edge" and i == LONG_LEAD and not all(long_lead_bound(w, q, k)[0] for k in (1, 10)):
            return False
        if kind == "pos_edge":  # (the drawn doc alone is looked at here; pos_edge_form looks at every doc)
            return pos_edge_doc(w, q, POS_EDGE_FORMS[i % 3], target[0]) and decides(ref, q)
        return kind not in DECIDING or decides(ref, q)

    out = {}
    for kind in kinds_of(name):
        out[kind] = []
        for i in range(per_kind):
            for _ in range(400):
                q = draw(kind, i)
                if n_terms_of(q) <= 16 and ok(kind, q, i):
                    break
            else:
                raise AssertionError(f"{name}/{kind}[{i}]: no candidate met the kind's condition")
            out[kind].append(q)
    return out
