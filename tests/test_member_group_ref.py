"""What tests/member_group_ref.py's queries decide (no GPU): the conditions its
generator draws candidates against, stated here independently -- over doc sets
taken from the token lists (count_clause_ref.Corpus), not from the reference's score
arrays -- so that the device tests (test_gpu_member_group.py,
test_gpu_seeded_member_group.py) cannot pass on a kernel that skips a member's
phrase verification, treats a phrase member as the conjunction of its terms, hands
a doc to the wrong pass or joins the members in another order.  Every query of
every kind must meet its kind's condition; none is left out."""
import numpy as np
import pytest

import count_clause_ref as ccr
import group_ref as gr
import member_group_ref as mg

M, S, X = mg.M, mg.S, mg.X
ANY, ALL = mg.ANY, mg.ALL
F = np.float32


@pytest.fixture(scope="module", params=["A", "B"])
def gen(request):
    w = mg.world(request.param)
    ints = lambda rows: [[int(x) for x in r] for r in rows]  # noqa: E731
    c = ccr.Corpus(ints(w.text), [r or None for r in ints(w.namef)], [[] for _ in range(w.n)], w.deleted.astype(np.uint8),
                   w.V, w.text_gaps, w.name_gaps)
    return w, mg.queries(w.name), c


def mset(c, m):
    """the docs a member matches, from the token lists"""
    if mg.is_phrase(m):
        s = ccr.clause_set(c, ccr.P(M, [int(t) if t < c.n_terms else None for t in m[1]], m[2]))
    else:
        s = ccr.clause_set(c, ccr.T(M, int(m) if m < c.n_terms else None))
    return np.zeros(c.n, bool) if s is None else s


def holds(c, ph):
    return np.logical_and.reduce([mset(c, t) for t in ph[1]])


def hits(w, q, **kw):
    m = np.zeros(w.n, bool)
    m[mg.ref_of(w.name).hits(q, **kw)[0]] = True
    return m


def group_of(q):
    """(the group body, its first phrase member, its term members) of the first group with a phrase member"""
    b = next(b for _, b in q if mg.is_group(b) and any(mg.is_phrase(m) for m in b[1]))
    return b, next(m for m in b[1] if mg.is_phrase(m)), [m for m in b[1] if not mg.is_phrase(m)]


def test_kinds_and_sizes(gen):
    w, qs, _ = gen
    assert mg.PER_KIND == 8 and set(qs) == set(mg.kinds_of(w.name))
    assert len(mg.KINDS) == 16 and mg.kinds_of("B") == list(mg.KINDS) and set(mg.KINDS) - set(mg.kinds_of("A")) == {"repeat"}
    for kind, v in qs.items():
        assert len(v) == mg.PER_KIND, kind
        for q in v:
            assert mg.n_rows_of(q) <= 16 and mg.phrase_members(q), (kind, q)
            for _, b in q:
                assert not mg.is_group(b) or len(b[1]) >= 2
    assert all(mg.n_rows_of(q) == 16 for q in qs["t16"])
    hit = [hits(w, q).any() for v in qs.values() for q in v]
    assert np.mean(hit) >= 0.9


def test_shapes(gen):
    """the kinds are the shapes the issue lists"""
    w, qs, _ = gen
    P, G = mg.is_phrase, mg.is_group
    shape = lambda q: [(oc, b[0], [P(m) for m in b[1]]) if G(b) else (oc, "p" if P(b) else "t") for oc, b in q]  # noqa: E731
    for q in qs["any_pt"]:
        assert len(q) == 1 and shape(q)[0][1:] in ((ANY, [True, False]), (ANY, [True, False, False]))
    for q in qs["any_tp"]:
        assert len(q) == 1 and shape(q)[0][1:] == (ANY, [False, True])
    for q in qs["any_pq"]:
        assert len(q) == 1 and shape(q)[0][2][:2] == [True, True]
    for q in qs["m_any_m"]:
        assert sorted(shape(q), key=str) == sorted([(M, ANY, [True, False]), (M, "t")], key=str) or \
            sorted(shape(q), key=str) == sorted([(M, ANY, [False, True]), (M, "t")], key=str)
    for q in qs["m_any_s"]:
        assert shape(q) == [(M, ANY, [True, False]), (S, "t"), (S, "t")]
    for q in qs["all_pt"]:
        assert len(q) == 1 and q[0][1][0] == ALL and sorted(shape(q)[0][2]) == [False, True]
    for q in qs["all3"]:
        assert shape(q) == [(S, "t"), (S, ALL, [False, False, True])]
    for q in qs["x_any_m"]:
        assert shape(q) == [(X, ANY, [True, False]), (M, "t")]
    for q in qs["s_any_s"]:
        assert {str(x) for x in shape(q)} in ({str((S, ANY, [True, False])), str((S, "t"))},
                                              {str((S, ANY, [False, True])), str((S, "t"))})
    for q in qs["s_any_sp"]:
        assert shape(q) == [(S, ANY, [True, False]), (S, "p")]
    for q in qs["s_any_sall"]:
        assert shape(q) == [(S, ANY, [True, False]), (S, ALL, [False, True])]
    for q in qs["hole"]:
        assert group_of(q)[1][2] == [0, 2]
    if "repeat" in qs:
        for q in qs["repeat"]:
            ph = group_of(q)[1]
            assert ph[1][0] == ph[1][1] and ph[2] == [0, 1]


def test_a_doc_hits_through_the_other_member(gen):
    """(P | t) kinds: a hit holds every term of P without the phrase and hits through the other member, P adding
    nothing: its score is the query's with P taken out of the group; and some hit matches P"""
    w, qs, c = gen
    for kind in ("any_pt", "any_tp", "m_any_m", "m_any_s", "s_any_s", "s_any_sp", "s_any_sall"):
        for q in qs[kind]:
            grp, ph, others = group_of(q)
            h = hits(w, q)
            through = h & holds(c, ph) & ~mset(c, ph) & np.logical_or.reduce([mset(c, t) for t in others])
            assert through.any() and (h & mset(c, ph)).any(), (kind, q)
            without = [(oc, (b[0], [m for m in b[1] if m is not ph]) if b is grp else b) for oc, b in q]
            d, s = mg.ref_of(w.name).hits(q)
            d2, s2 = mg.ref_of(w.name).hits(without)
            x = int(np.flatnonzero(through)[0])
            assert s[d == x].view(np.uint32) == s2[d2 == x].view(np.uint32), (kind, q, x)


def test_the_all_of_form_drops_that_doc(gen):
    """(P & t): a live doc holds every term of P and t, not the phrase -- a hit of (P | t) -- and is no hit"""
    w, qs, c = gen
    for q in qs["all_pt"]:
        grp, ph, (a,) = group_of(q)
        doc = holds(c, ph) & ~mset(c, ph) & mset(c, a) & ~w.deleted
        h = hits(w, q)
        assert h.any() and doc.any() and not (h & doc).any(), q
        assert (hits(w, [mg.G(S, ANY, grp[1])]) & doc).sum() == doc.sum()
        assert np.array_equal(h, mset(c, ph) & mset(c, a) & ~w.deleted)


def test_two_phrase_members_and_exclusion(gen):
    w, qs, c = gen
    for q in qs["any_pq"]:
        p, p2 = q[0][1][1][:2]
        h = hits(w, q)
        assert (h & mset(c, p) & ~mset(c, p2)).any() and (h & ~mset(c, p) & mset(c, p2)).any(), q
    for q in qs["m_any_m"]:
        term = next(b for _, b in q if not mg.is_group(b))
        assert not np.array_equal(hits(w, q), mset(c, term) & ~w.deleted), q
    for q in qs["x_any_m"]:
        grp, ph, (a,) = group_of(q)
        u = mset(c, q[1][1]) & ~w.deleted
        h = hits(w, q)
        assert (u & mset(c, ph) & ~mset(c, a) & ~h).any(), q   # excluded by the phrase alone
        assert (u & holds(c, ph) & ~mset(c, ph) & ~mset(c, a) & h).any(), q  # every term, not the phrase: kept
    for q in qs["s_any_sp"]:
        assert (hits(w, q) & mset(c, q[1][1])).any(), q
    for q in qs["s_any_sall"]:
        assert (hits(w, q) & np.logical_and.reduce([mset(c, m) for m in q[1][1][1]])).any(), q
    for q in qs["hole"]:
        grp, ph, _ = group_of(q)
        tight = [(oc, (b[0], [mg.Ph(m[1]) if m is ph else m for m in b[1]]) if b is grp else b) for oc, b in q]
        assert (hits(w, q) & mset(c, ph)).any() and not np.array_equal(hits(w, q), hits(w, tight)), q


def test_all3_cost_order_and_nested_sum(gen):
    """(t & u & P) beside a Should term: the phrase stands first, second and third in (cost, position) order -- its cost
    the sum over the two fields of its terms' smallest doc count there, from the token lists -- and some hit's bits
    differ from the flat sum of the same scores"""
    w, qs, c = gen
    df = lambda docs, t: sum(1 for d in docs if d is not None and t in d)  # noqa: E731
    text = [set(int(x) for x in d) for d in w.text]
    name = [set(int(x) for x in d) for d in w.namef]
    ranks = []
    for i, q in enumerate(qs["all3"]):
        members = q[1][1][1]
        cost = [sum(min(df(f, t) for t in m[1]) for f in (text, name)) if mg.is_phrase(m) else df(text, m) + df(name, m)
                for m in members]
        order = sorted(range(3), key=lambda j: cost[j])
        ranks.append(order.index(2))
        assert ranks[-1] == i % 3 == mg.phrase_rank(w, q[1][1]), (i, cost)
        assert mg.nested_differs(w, q), q
    assert set(ranks) == {0, 1, 2}


def test_name_only_and_text_only_matches(gen):
    w, qs, c = gen
    for q in qs["name"]:
        ph = mg.phrase_members(q)[0]
        assert (hits(w, q) & (c.fname.counts(ph[1], ph[2]) > 0) & (c.ftext.counts(ph[1], ph[2]) == 0)).any(), q
    text_only = 0
    for q in qs["any_pt"]:
        ph = mg.phrase_members(q)[0]
        text_only += bool((hits(w, q) & (c.ftext.counts(ph[1], ph[2]) > 0) & (c.fname.counts(ph[1], ph[2]) == 0)).any())
    assert text_only >= 1


def test_a_member_missing_from_a_segment(gen):
    """seg: a phrase member holds a term that one of the three unequal segments lacks: the any-of group goes on there
    (hits through the other member), the all-of group is absent there (the hits and bits of the Should term alone); a
    term no snapshot holds: the any-of group is its other member, the all-of Must empties the query"""
    w, qs, c = gen
    assert len(set(np.diff(w.cuts))) == 3
    ref = mg.ref_of(w.name)
    for i, q in enumerate(qs["seg"]):
        grp, ph, others = group_of(q)
        if i % 4 >= 2:
            assert set(ph[1]) & set(mg.GONE[w.name])
            if i % 4 == 2:
                assert np.array_equal(hits(w, q), mset(c, others[0]) & ~w.deleted) and hits(w, q).any()
            else:
                assert not hits(w, q).any()
            continue
        segs = [si for si, (lo, hi) in enumerate(zip(w.cuts[:-1], w.cuts[1:]))
                if any(not mset(c, t)[lo:hi].any() for t in ph[1])]
        assert segs and mset(c, ph).any(), q
        found = False
        for si in segs:
            d, s = mg.seg_hits(w, q, si)
            if i % 4 == 0:
                found |= len(d) > 0 and grp[0] == ANY
            else:
                d2, s2 = mg.seg_hits(w, [q[1]], si)
                found |= len(d) > 0 and grp[0] == ALL and np.array_equal(d, d2) and \
                    np.array_equal(s.view(np.uint32), s2.view(np.uint32))
        assert found, q


def rewritten(c, q):
    """each group over member doc sets: a phrase member becomes a term of its own whose postings are the phrase's docs"""
    out, nxt = [], [1 << 20]
    t = lambda x: None if x >= c.n_terms else int(x)  # noqa: E731 (a term the dictionary lacks)
    for oc, b in q:
        if mg.is_phrase(b):
            out.append(ccr.P(oc, [t(x) for x in b[1]], b[2]))
        elif mg.is_group(b):
            ids = []
            for m in b[1]:
                if not mg.is_phrase(m):
                    ids.append(t(m))
                    continue
                s = ccr.clause_set(c, ccr.P(M, [t(x) for x in m[1]], m[2]))
                nxt[0] += 1
                c.post.pop(nxt[0], None)  # (an absent phrase stays a term without postings)
                if s is not None:
                    c.post[nxt[0]] = set(np.flatnonzero(s).tolist())
                ids.append(nxt[0])
            out.append((ccr.ANY if b[0] == ANY else ccr.ALL)(oc, ids))
        else:
            out.append(ccr.T(oc, t(b)))
    return out


def test_match_sets_equal_the_count_reference(gen):
    """an independent statement of the match rule: count_clause_ref.match_mask over the rewritten clauses"""
    w, qs, c = gen
    for kind, v in qs.items():
        for q in v:
            m = ccr.match_mask(c, rewritten(c, q), [])
            assert np.array_equal(np.flatnonzero(m), np.sort(mg.ref_of(w.name).hits(q)[0])), (kind, q)


def test_the_bound_is_at_least_every_score(gen):
    """the member-level bound, restated in numpy (member_group_ref.bound), >= every hit's score"""
    w, qs, _ = gen
    for kind, v in qs.items():
        for q in v:
            s = mg.ref_of(w.name).hits(q)[1]
            if len(s):
                assert mg.bound(w, q) >= s.max(), (kind, q, float(mg.bound(w, q)), float(s.max()))


def test_repeats_on_the_edge_lists_and_the_chunk_bound():
    """repeat on B: "e e" as a member on the 2047 / 2048 / 2049 / 8193-posting lists and on the escaped-tf doc's list;
    and, in the reference's numbers, the chunk bound lies below the k-th score on the 8193-posting list at k = 1"""
    w = mg.world("B")
    qs = mg.queries("B")["repeat"]
    syn = gr.synth()
    assert [syn.merged_len(t) for t in mg.EDGE_TERMS] == [2047, 2048, 2049, 8193]
    for i, t in enumerate(mg.EDGE_TERMS):
        assert group_of(qs[i])[1][1] == [t, t]
    t = gr.T_2047
    assert group_of(qs[4])[1][1] == [t, t]
    ct = w.base.text.counts([t, t], [0, 1])
    assert ct.max() == 299  # the escaped tf
    q = qs[mg.LONG_LEAD]
    assert q[0][1][0] == ANY and q[0][1][1][1] == gr.T_LONG and mg.is_phrase(q[0][1][1][0])
    fires, bounds, kth = mg.long_lead_bound(w, q, 1)
    print(f"k=1: chunk bounds {[float(b) for b in bounds]}, k-th score {float(kth)}")
    assert fires and len(bounds) == 5


# ------------------------------------------------------------------ a hand case
def test_four_docs_by_hand():
    """a b c / b a c / a b / c d with ("a b" | c): d1 holds a and b, not the phrase, and hits through c with c's score
    alone; ("a b" & c) keeps d0 only; the ABI rows"""
    import bool_phrase_ref as bp
    a, b, c, d = 0, 1, 2, 3
    docs = [[a, b, c], [b, a, c], [a, b], [c, d]]
    ref = mg.Ref(bp.Ref(4, docs))
    q = [mg.G(S, ANY, [mg.Ph([a, b]), c])]
    hd, hs = ref.hits(q)
    assert hd.tolist() == [0, 1, 2, 3]
    cd, cs = ref.hits([mg.T(S, c)])
    pd, ps = ref.hits([mg.P(S, [a, b])])
    assert cd.tolist() == [0, 1, 3] and pd.tolist() == [0, 2]
    assert hs[1].view(np.uint32) == F(F(0.0) + cs[1]).view(np.uint32) and hs[2].view(np.uint32) == ps[1].view(np.uint32)
    assert hs[0] == F(F(F(0.0) + ps[0]) + cs[0])  # members from 0.0 in written order
    ad, as_ = ref.hits([mg.G(S, ALL, [mg.Ph([a, b]), c])])
    assert ad.tolist() == [0]
    qo, terms, occur, plen, ppos = mg.batch([q, [mg.G(M, ALL, [c, mg.Ph([a, b], [0, 2])]), mg.T(S, d)]])
    assert (qo.tolist(), terms.tolist()) == ([0, 3, 7], [a, b, c, c, a, b, d])
    assert plen.tolist() == [3 | gr.FLAG[ANY], 0, 0, 3 | gr.FLAG[ALL], 0, 0, 1] and ppos.tolist() == [0, 1, 0, 0, 0, 2, 0]
    assert occur.tolist() == [S] * 3 + [M] * 3 + [S]
