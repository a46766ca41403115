"""Reference for queries whose groups hold PHRASE MEMBERS (`(e-mail OR email)
server`: DESIGN.md §19), in numpy f32.  Nothing new is stated here: every member
gives a doc a score or "absent" --
  * a term member as everywhere (group_ref.Ref._term),
  * a phrase member by bool_phrase_ref.Ref.clause (the forward-index count per field,
    Bm25Weight::for_terms, text then name from 0.0; cost: the sum over the two
    fields of its terms' smallest doc count there) --
the group joins its members through bool_ref.Corpus._match as group_ref.Ref._clause
does (any-of: Shoulds, the present members from 0.0 in written order, cost the sum;
all-of: Musts in (cost, position) order, (s0 + s1) + (0.0 + s2 + ...), cost the
smallest), and the query joins its clauses through _match unchanged, per segment,
with that segment's costs.  It calls nothing of libfugu.

A query is a list of clauses (occur, body): body a term id, a phrase
(PHR, [term ids], [offsets]) or a group (ANY | ALL, [members]), a member a term id
or a phrase (PHR, [term ids], [offsets]).  A phrase member with a term the segment
lacks matches no doc there, which is what "absent" means to _match: the any-of
group goes on without it, the all-of group is absent.

The corpora are group_phrase_ref's: A = phrase_ref.Synth(), B = group_ref.synth()
read by position, where "t t" matches exactly the docs with tf(t) >= 2.
"""
import functools

import numpy as np

import bool_ref as br
import group_phrase_ref as gp
import group_ref as gr
import phrase_ref as pr

MUST, SHOULD, MUST_NOT = br.MUST, br.SHOULD, br.MUST_NOT
M, S, X = MUST, SHOULD, MUST_NOT
MISSING = br.MISSING
ANY, ALL, PHR = gp.ANY, gp.ALL, gp.PHR
F = np.float32
hits_of = br.hits_of
KS = gp.KS
T, P = gp.T, gp.P            # a term clause, a phrase clause
is_phrase, is_group = gp.is_phrase, gp.is_group
world = gp.world


def Ph(terms, offsets=None):
    """a phrase MEMBER of a group"""
    terms = [int(t) for t in terms]
    return (PHR, terms, list(range(len(terms))) if offsets is None else [int(o) for o in offsets])


def G(oc, kind, members):
    return (oc, (kind, [m if is_phrase(m) else int(m) for m in members]))


def rows_of(body):
    """[(term, offset)] as the ABI lists the clause: an offset 0 begins a member of a group"""
    if is_phrase(body):
        return list(zip(body[1], body[2]))
    if is_group(body):
        return [r for m in body[1] for r in (rows_of(m) if is_phrase(m) else [(m, 0)])]
    return [(body, 0)]


def n_rows_of(query):
    return sum(len(rows_of(b)) for _, b in query)


def phrase_members(query):
    return [m for _, b in query if is_group(b) for m in b[1] if is_phrase(m)]


def batch(queries):
    """(q_off, terms, occur, phrase_len, phrase_pos): FG_CLAUSE_ANY / FG_CLAUSE_ALL OR-ed onto the group's number of
    ROWS at its first term, zeros after; phrase_pos 0 at a member's first row, a phrase member's offsets after it"""
    q_off, terms, occur, plen, ppos = [0], [], [], [], []
    for q in queries:
        for oc, body in q:
            rows = rows_of(body)
            terms += [t for t, _ in rows]
            ppos += [o for _, o in rows]
            occur += [oc] * len(rows)
            plen += [len(rows) | gr.FLAG[body[0]] if is_group(body) else len(rows)] + [0] * (len(rows) - 1)
        q_off.append(len(terms))
    return (np.array(q_off, np.uint32), np.array(terms, np.uint32), np.array(occur, np.uint8),
            np.array(plen, np.uint32), np.array(ppos, np.uint32))


class Ref(gp.Ref):
    def _member(self, m, lo, hi, st):
        """(scores [n] f32, -1 where absent; the member's cost inside [lo, hi))"""
        if is_phrase(m):
            s, cost = self.b.clause(m[1], m[2], st)
            return s, (cost(lo, hi) if hi > lo else 0)
        s, pre = self.g._term(m, self.b._bstats(st))
        return s, int(pre[hi] - pre[lo])

    def _clause(self, body, lo, hi, st):
        if not is_group(body):
            return super()._clause(body, lo, hi, st)
        kind, members = body
        arrays, costs = [], []
        for m in members:  # the cost as a prefix that differs by it across [lo, hi)
            s, cost = self._member(m, lo, hi, st)
            pre = np.zeros(self.n + 1, np.int64)
            pre[hi:] = cost
            arrays.append((s, pre))
            costs.append(cost)
        occ = [SHOULD if kind == ANY else MUST] * len(members)
        m, sc = br.Corpus._match(gr._Clauses(self.n, arrays), list(range(len(members))), occ, lo, hi, None, True)
        s = np.full(self.n, F(-1.0))
        s[lo:hi] = np.where(m, sc, F(-1.0))
        return s, (sum(costs) if kind == ANY else min(costs))


@functools.lru_cache(maxsize=None)
def ref_of(name):
    return Ref(world(name).base)


# ------------------------------------------------------------------ the bound, restated
INFLATE = F(1.00000762939453125)  # fg_internal.h inflate_bound: 1 + 2^-17


def member_ub(w, m, st=None):
    """a member's largest score: a term's, over its docs; a phrase's two field weights (0.0 for a field where some term
    has no posting), summed as its score sums the fields"""
    st = st or w.base.pstats
    if is_phrase(m):
        wt = pr.weight(st.df_text, st.n, m[1]) if min(int(st.df_text[t]) if t < w.V else 0 for t in m[1]) else F(0.0)
        wn = pr.weight(st.df_name, st.n, m[1]) if min(int(st.df_name[t]) if t < w.V else 0 for t in m[1]) else F(0.0)
        return F(F(F(0.0) + wt) + wn)
    s = ref_of(w.name)._member(m, 0, w.n, st)[0]
    return F(max(F(s.max()), F(0.0)))


def clause_ub(w, body, st=None):
    st = st or w.base.pstats
    if not is_group(body):
        return member_ub(w, body, st)
    kind, members = body
    z = F(0.0)
    if kind == ANY:
        a = z
        for m in members:
            a = F(a + member_ub(w, m, st))
        return a
    r = ref_of(w.name)
    order = sorted(range(len(members)), key=lambda j: r._member(members[j], 0, w.n, st)[1])  # (stable: cost, position)
    u = [member_ub(w, members[j], st) for j in order]
    rest = z
    for x in u[2:]:
        rest = F(rest + x)
    return F(z + F(F(u[0] + u[1]) + rest))


def bound(w, query, st=None):
    """the score sum over upper bounds, every clause and member present: >= every hit's score, bit for bit"""
    st = st or w.base.pstats
    r = ref_of(w.name)
    z = F(0.0)
    must = [(r._clause(b, 0, w.n, st)[1], j, b) for j, (oc, b) in enumerate(query) if oc == M]
    should = [b for oc, b in query if oc == S]
    opt = z
    for b in should:
        opt = F(opt + clause_ub(w, b, st))
    if not must:
        return opt
    u = [clause_ub(w, b, st) for _, _, b in sorted(must, key=lambda x: x[:2])]
    req = u[0]
    if len(u) > 1:
        rest = z
        for x in u[2:]:
            rest = F(rest + x)
        req = F(F(u[0] + u[1]) + rest)
    return F(F(z + req) + opt)


KCHUNK = 2048   # fg_internal.h kChunk: the postings of a lead chunk
LONG_LEAD = 7   # repeat[7] on B: ("u u" | T_LONG), whose second pass sweeps the 8193-posting list


def long_lead_bound(w, q, k):
    """For q = [G(M, ANY, [Ph([u, u]), T_LONG])] on B: (whether some chunk of the pass over T_LONG's list -- the docs
    the phrase does not match -- lies below the k-th score, the chunks' bounds, the k-th score).  The pass knows the
    phrase absent, so a chunk's bound is (0.0 + (0.0 + max T_LONG score in the chunk)) + 0.0, times 1 + 2^-17."""
    (_, (kind, (ph, e))), = q
    assert kind == ANY and e == gr.T_LONG and is_phrase(ph)
    se = ref_of(w.name)._member(e, 0, w.n, w.base.pstats)[0]
    lead = np.flatnonzero(se >= 0)
    z = F(0.0)
    bounds = [F(F(F(z + F(z + se[lead[c:c + KCHUNK]].max())) + z) * INFLATE) for c in range(0, len(lead), KCHUNK)]
    s = ref_of(w.name).search(q, k)[0]
    kth = s[k - 1] if len(s) >= k else z
    return any(b < kth for b in bounds), bounds, kth


# ------------------------------------------------------------------ what a query decides
def member_on(w, m):
    """the docs the member matches [n] bool (deleted docs included)"""
    return ref_of(w.name)._member(m, 0, w.n, w.base.pstats)[0] >= 0


def holds_all(w, ph):
    return np.logical_and.reduce([member_on(w, t) for t in ph[1]])


def hit_mask(w, q, **kw):
    m = np.zeros(w.n, bool)
    m[ref_of(w.name).hits(q, **kw)[0]] = True
    return m


def first_member_group(q):
    """(P, [term members]) of the first any-of / all-of group that holds a phrase member"""
    for _, b in q:
        if is_group(b) and any(is_phrase(m) for m in b[1]):
            return next(m for m in b[1] if is_phrase(m)), [m for m in b[1] if not is_phrase(m)]
    raise ValueError("no group with a phrase member")


def through_other(w, q):
    """a hit holds every term of P without the phrase and has a term member of P's group"""
    ph, others = first_member_group(q)
    other = np.logical_or.reduce([member_on(w, t) for t in others]) if others else np.zeros(w.n, bool)
    return bool((hit_mask(w, q) & holds_all(w, ph) & ~member_on(w, ph) & other).any())


def p_hits(w, q):
    """a hit matches P"""
    return bool((hit_mask(w, q) & member_on(w, first_member_group(q)[0])).any())


def phrase_rank(w, grp):
    """the position of the all-of group's (first) phrase member in (cost, position) order"""
    r = ref_of(w.name)
    order = sorted(range(len(grp[1])), key=lambda j: r._member(grp[1][j], 0, w.n, w.base.pstats)[1])
    return order.index(next(j for j, m in enumerate(grp[1]) if is_phrase(m)))


def nested_differs(w, q):
    """q = [T(S, v), G(S, ALL, members)]: some hit's bits differ from the flat sum ((0.0 + v) + m0) + m1 + ... of the same
    scores in the same (cost, position) order"""
    (_, v), (_, grp) = q
    r = ref_of(w.name)
    st = w.base.pstats
    order = sorted(range(len(grp[1])), key=lambda j: r._member(grp[1][j], 0, w.n, st)[1])
    arrs = [r._member(grp[1][j], 0, w.n, st)[0] for j in order]
    sv = r._member(v, 0, w.n, st)[0]
    d, s = r.hits(q)
    both = np.logical_and.reduce([a[d] >= 0 for a in arrs] + [sv[d] >= 0])
    flat = F(0.0) + sv[d]
    for a in arrs:
        flat = (flat + a[d]).astype(F)
    return bool((flat[both].view(np.uint32) != s[both].view(np.uint32)).any())


def seg_lacking(w):
    """[(segment index, term)]: the term has postings in the corpus and none in that segment"""
    out = []
    for si, (lo, hi) in enumerate(zip(w.cuts[:-1], w.cuts[1:])):
        for t in range(w.V):
            on = member_on(w, t)
            if on.any() and not on[lo:hi].any():
                out.append((si, t))
    return out


def seg_hits(w, q, si):
    """(docs, scores) of the hits inside segment si when the corpus is cut at w.cuts"""
    d, s = ref_of(w.name).hits(q, seg_bounds=w.cuts)
    keep = (d >= w.cuts[si]) & (d < w.cuts[si + 1])
    return d[keep], s[keep]


# ------------------------------------------------------------------ the queries
KINDS = ("any_pt", "any_tp", "any_pq", "m_any_m", "m_any_s", "all_pt", "all3", "x_any_m", "s_any_s", "s_any_sp",
         "s_any_sall", "hole", "repeat", "seg", "name", "t16")
ONLY_ON = {"repeat": "B"}
PER_KIND = 8
EDGE_TERMS = gp.EDGE_TERMS
GONE = gp.GONE


def kinds_of(name):
    return [k for k in KINDS if ONLY_ON.get(k, name) == name]


@functools.lru_cache(maxsize=None)
def queries(name, per_kind=PER_KIND, seed=5119):
    """{kind: [query]} on world(name).  A candidate is drawn again until it meets its kind's condition
    (test_member_group_ref.py states and checks them); the conditions are never lowered."""
    w = world(name)
    ref = ref_of(name)
    r = np.random.default_rng(seed + (name == "B"))
    alive = np.flatnonzero(~w.deleted)
    plain = [int(i) for i in alive if w.text_gaps[i] is None and len(w.text[i]) >= 8]
    named = [int(i) for i in alive if len(w.namef[i]) >= 2 and w.name_gaps[i] is None
             and any(int(t) in w.pools["name_only"] for t in w.namef[i])]
    mid, rare, name_only = w.pools["mid"], w.pools["rare"], w.pools["name_only"]
    plain_set = set(plain)
    with_term = {}  # per term a segment lacks: the plain docs whose text holds it
    for _, x in seg_lacking(w):
        with_term[x] = [int(d) for d in w.base.corpus.docs(x, 0) if int(d) in plain_set]
    lacking = [(si, x) for si, x in seg_lacking(w) if with_term[x]]
    seg_of = [None]  # seg: the segment the candidate's phrase is absent from

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
        if kind == "any_pt":
            return [G(S, ANY, [Ph(ph), a] + ([b] if i % 4 == 3 else []))]
        if kind == "any_tp":
            return [G(S if i % 2 else M, ANY, [a, Ph(ph)])]
        if kind == "any_pq":
            return [G(S, ANY, [Ph(ph), Ph(phrase(i + 1))] + ([a] if i % 2 else []))]
        if kind == "m_any_m":
            return [G(M, ANY, [Ph(ph), a]), T(M, b)] if i % 2 else [T(M, b), G(M, ANY, [a, Ph(ph)])]
        if kind == "m_any_s":
            return [G(M, ANY, [Ph(ph), a]), T(S, b), T(S, c3)]
        if kind == "all_pt":
            return [G(S, ALL, [Ph(ph), a])] if i % 2 else [G(M, ALL, [a, Ph(ph)])]
        if kind == "all3":
            t, u = pick(mid, 2, avoid=ph) if i % 3 == 0 else pick(rare, 2, avoid=ph) if i % 3 == 2 else \
                (pick(rare, 1, avoid=ph) + pick(mid, 1, avoid=ph))[::1 if i % 2 else -1]
            return [T(S, c3), G(S, ALL, [t, u, Ph(ph)])]
        if kind == "x_any_m":
            return [G(X, ANY, [Ph(ph), a]), T(M, b)]
        if kind == "s_any_s":
            return [G(S, ANY, [Ph(ph), a]), T(S, b)] if i % 2 else [T(S, b), G(S, ANY, [a, Ph(ph)])]
        if kind == "s_any_sp":
            return [G(S, ANY, [Ph(ph), a]), P(S, phrase(i + 1))]
        if kind == "s_any_sall":
            return [G(S, ANY, [Ph(ph), a]), G(S, ALL, [b, Ph(phrase(i + 1))])]
        if kind == "hole":
            sp = cut(w.text[doc()], 3)
            hole = Ph([sp[0], sp[2]], [0, 2])
            return [G(S, ANY, [hole, a])] if i % 2 else [G(M, ALL, [hole, a]), T(S, b)]
        if kind == "repeat":  # "e e" on each edge list, on the escaped-tf doc's list, and ("u u" | T_LONG)
            e = EDGE_TERMS[i % 4]
            u = pick(mid)[0]
            return [[G(M, ANY, [Ph([e, e]), a])], [G(M, ANY, [Ph([e, e]), a])], [G(M, ANY, [Ph([e, e]), a])],
                    [G(M, ANY, [Ph([e, e]), a])], [G(M, ALL, [Ph([e, e]), a])], [G(M, ALL, [a, Ph([e, e])]), T(S, b)],
                    [G(S, ANY, [a, Ph([e, e])]), T(S, b)], [G(M, ANY, [Ph([u, u]), gr.T_LONG])]][i]
        if kind == "seg":
            if i % 4 >= 2:
                gone = GONE[name][i % len(GONE[name])]
                return [G(S, ANY, [Ph(ph + [gone]), a])] if i % 4 == 2 else [G(M, ALL, [a, Ph(ph + [gone])]), T(S, b)]
            si, x = lacking[int(r.integers(0, len(lacking)))]
            seg_of[0] = si
            toks = w.text[with_term[x][int(r.integers(0, len(with_term[x])))]]  # a phrase that holds x, cut from a doc
            at = [p for p in range(len(toks) - 1) if int(toks[p]) == x or int(toks[p + 1]) == x]
            p = at[int(r.integers(0, len(at)))]
            ph = [int(toks[p]), int(toks[p + 1])]
            inside = [int(t) for d in range(w.cuts[si], min(w.cuts[si + 1], w.cuts[si] + 50)) for t in w.text[d]
                      if int(t) not in ph]
            t1, t2 = (inside[int(r.integers(0, len(inside)))] for _ in range(2))
            return [G(S, ANY, [Ph(ph), t1])] if i % 4 == 0 else [G(S, ALL, [Ph(ph), t1]), T(S, t2)]
        if kind == "name":  # a phrase member present only in `name`
            nm = w.namef[named[int(r.integers(0, len(named)))]]
            while True:
                nph = cut(nm, 2)
                if max(nph) in name_only or min(nph) in name_only:
                    break
            n1 = pick(name_only)[0]
            return [[G(S, ANY, [Ph(nph), a])], [G(M, ANY, [n1, Ph(nph)]), T(S, b)], [G(S, ALL, [Ph(nph), n1])],
                    [G(M, ANY, [Ph(nph), Ph(ph)]), T(M, a)]][i % 4]
        if kind == "t16":  # 16 rows: a group of two phrases and two terms, a phrase clause, an all-of group, a term
            ts = pick(mid + rare, 4)
            return [G(M if i % 2 else S, ANY, [Ph(cut(w.text[doc()], 4)), ts[0], Ph(cut(w.text[doc()], 3)), ts[1]]),
                    P(S, cut(w.text[doc()], 3)), G(S, ALL, [ts[2], Ph(phrase(0))]), T(X if i % 4 == 0 else S, ts[3])]
        raise KeyError(kind)

    def ok(kind, q, i):
        if kind in ("any_pt", "any_tp", "m_any_s", "s_any_s"):
            return through_other(w, q) and p_hits(w, q)
        if kind == "any_pq":
            p, q2 = q[0][1][1][:2]
            h = hit_mask(w, q)
            return bool((h & member_on(w, p) & ~member_on(w, q2)).any() and (h & ~member_on(w, p) & member_on(w, q2)).any())
        if kind == "m_any_m":
            term = next(b for _, b in q if not is_group(b))
            return through_other(w, q) and p_hits(w, q) and not np.array_equal(hit_mask(w, q), hit_mask(w, [T(M, term)]))
        if kind == "all_pt":
            ph, (a,) = first_member_group(q)
            dropped = holds_all(w, ph) & ~member_on(w, ph) & member_on(w, a) & ~w.deleted
            return bool(hit_mask(w, q).any() and dropped.any())
        if kind == "all3":
            return phrase_rank(w, q[1][1]) == i % 3 and nested_differs(w, q)
        if kind == "x_any_m":
            ph, (a,) = first_member_group(q)
            u = member_on(w, q[1][1]) & ~w.deleted
            h = hit_mask(w, q)
            return bool((u & member_on(w, ph) & ~member_on(w, a) & ~h).any()
                        and (u & holds_all(w, ph) & ~member_on(w, ph) & ~member_on(w, a) & h).any())
        if kind == "s_any_sp":
            return through_other(w, q) and p_hits(w, q) and bool((hit_mask(w, q) & member_on(w, q[1][1])).any())
        if kind == "s_any_sall":
            allg = ref._clause(q[1][1], 0, w.n, w.base.pstats)[0] >= 0
            return through_other(w, q) and p_hits(w, q) and bool((hit_mask(w, q) & allg).any())
        if kind == "hole":
            ph = first_member_group(q)[0]
            tight = [(oc, (b[0], [Ph(m[1]) if is_phrase(m) else m for m in b[1]])) if is_group(b) else (oc, b) for oc, b in q]
            return p_hits(w, q) and not np.array_equal(hit_mask(w, q), hit_mask(w, tight))
        if kind == "repeat":
            return p_hits(w, q) and (i != LONG_LEAD or long_lead_bound(w, q, 1)[0])
        if kind == "seg" and i % 4 < 2:
            si = seg_of[0]
            d, s = seg_hits(w, q, si)
            if i % 4 == 0:
                return len(d) > 0
            d2, s2 = seg_hits(w, [q[1]], si)
            return len(d) > 0 and np.array_equal(d, d2) and np.array_equal(s.view(np.uint32), s2.view(np.uint32))
        if kind == "seg":
            return True
        if kind == "name":
            ph = phrase_members(q)[0]
            h = hit_mask(w, q)
            return bool((h & (w.base.name.counts(ph[1], ph[2]) > 0) & (w.base.text.counts(ph[1], ph[2]) == 0)).any())
        if kind == "t16":
            return n_rows_of(q) == 16 and bool(hit_mask(w, q).any())
        raise KeyError(kind)

    out = {}
    for kind in kinds_of(name):
        out[kind] = []
        for i in range(per_kind):
            for _ in range(400):
                q = draw(kind, i)
                if n_rows_of(q) <= 16 and ok(kind, q, i):
                    break
            else:
                raise AssertionError(f"{name}/{kind}[{i}]: no candidate met the kind's condition")
            out[kind].append(q)
    return out


def all_queries(name):
    kinds = queries(name)
    return [q for kind in kinds_of(name) for q in kinds[kind]]
