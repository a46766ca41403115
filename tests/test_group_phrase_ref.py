"""What tests/group_phrase_ref.py's queries decide (no GPU): the conditions its
generator draws candidates against, stated here independently, so that the device
tests (test_gpu_group_phrase.py, test_gpu_seeded_group_phrase.py) cannot pass on a
kernel that skips the phrase verification, ignores the groups, runs over a doc's
end or joins the clauses in another order."""
import numpy as np
import pytest

import count_clause_ref as ccr
import group_phrase_ref as gp
import group_ref as gr

M, S, X = gp.M, gp.S, gp.X
ANY, ALL = gp.ANY, gp.ALL
F = np.float32


@pytest.fixture(scope="module", params=["A", "B"])
def gen(request):
    w = gp.world(request.param)
    return w, gp.queries(w.name)


def test_kinds_and_sizes(gen):
    w, qs = gen
    assert gp.PER_KIND >= 4 and set(qs) == set(gp.kinds_of(w.name)) and len(qs) == 15
    assert {"mp_many", "mp_mall", "many_sp", "sp_sany", "sany_sp", "sp_sall", "xp_many", "xany_mp", "two_p", "miss",
            "repeat", "name", "t16", "tie", "pos_edge", "lead_edge"} == set(gp.KINDS)
    for kind, v in qs.items():
        assert len(v) == gp.PER_KIND, kind
        for q in v:
            assert gp.n_terms_of(q) <= 16 and any(gp.is_group(b) for _, b in q) and any(gp.is_phrase(b) for _, b in q)
    assert any(gp.n_terms_of(q) == 16 for q in qs["t16"])
    assert all(sum(gp.is_phrase(b) for _, b in q) == 2 for q in qs["two_p"])
    hit = [len(w.ref.hits(q)[0]) > 0 for v in qs.values() for q in v]
    assert np.mean(hit) >= 0.9


def test_deciding_kinds(gen):
    """per query: the verification decides (the phrases as all-of groups of their terms hit other docs), and so do
    the groups (dropped, other docs hit)"""
    w, qs = gen
    for kind in gp.DECIDING:
        for q in qs.get(kind, []):
            h = gp.hit_set(w.ref, q)
            assert h and h != gp.hit_set(w.ref, gp.phrases_as_groups(q)), (kind, q)
            assert h != gp.hit_set(w.ref, gp.without_groups(q)), (kind, q)
    for q in qs["many_sp"]:  # the Should phrase only adds score
        assert gp.hit_set(w.ref, q) == gp.hit_set(w.ref, gp.phrases_as_groups(q))


def test_should_phrase_docs_that_hit_through_the_group(gen):
    """sp_sany / sany_sp: a doc holds every term of the phrase, not the phrase, and hits through the group -- the doc
    stage (a) must queue although it may belong to another pass"""
    w, qs = gen
    st = w.base.pstats
    for kind in ("sp_sany", "sany_sp"):
        for q in qs[kind]:
            ph = next(b for _, b in q if gp.is_phrase(b))
            grp = next(b for _, b in q if gp.is_group(b))
            has = lambda t: w.base.clause([t], [0], st)[0] >= 0  # noqa: E731
            all_terms = np.logical_and.reduce([has(t) for t in ph[1]])
            no_phrase = w.base.clause(ph[1], ph[2], st)[0] < 0
            in_group = np.logical_or.reduce([has(t) for t in grp[1]])
            d = w.ref.hits(q)[0]
            assert (all_terms & no_phrase & in_group)[d].any(), (kind, q)


def test_must_kinds_nest_their_sums(gen):
    """some shared doc's nested-sum bits differ from those of the same clauses with the groups flattened"""
    w, qs = gen
    for kind in gp.MUST_KINDS:
        differ = 0
        for q in qs[kind]:
            d, s = w.ref.hits(q)
            fd, fs = w.ref.hits(gp.flatten_groups(q))
            _, i, j = np.intersect1d(d, fd, return_indices=True)
            differ += bool((s[i].view(np.uint32) != fs[j].view(np.uint32)).any())
        assert differ >= 1, kind


def as_count_clause(oc, body):
    t = lambda x: None if x >= 64 else int(x)  # noqa: E731 (a term the dictionary lacks)
    if gp.is_phrase(body):
        return ccr.P(oc, [t(x) for x in body[1]], body[2])
    if gp.is_group(body):
        return (ccr.ANY if body[0] == ANY else ccr.ALL)(oc, [t(x) for x in body[1]])
    return ccr.T(oc, t(body))


def test_match_sets_equal_the_count_reference(gen):
    """an independent statement of the match rule: count_clause_ref.match_mask over the same clauses"""
    w, qs = gen
    ints = lambda rows: [[int(x) for x in r] for r in rows]  # noqa: E731
    c = ccr.Corpus(ints(w.text), [r or None for r in ints(w.namef)], [[] for _ in range(w.n)], w.deleted.astype(np.uint8),
                   w.V, w.text_gaps, w.name_gaps)
    for kind, v in qs.items():
        for q in v:
            m = ccr.match_mask(c, [as_count_clause(oc, b) for oc, b in q], [])
            assert np.array_equal(np.flatnonzero(m), np.sort(w.ref.hits(q)[0])), (kind, q)


def test_ties_and_missing_terms(gen):
    w, qs = gen
    for q in qs["tie"]:
        assert gp.ties(w.ref, q), q
    gone = lambda q: [t for _, b in q for t in gp.terms_of(b) if t in gp.GONE[w.name]]  # noqa: E731
    assert all(gone(q) for q in qs["miss"])
    under = {(oc, gp.is_phrase(b)) for q in qs["miss"] for oc, b in q if set(gp.terms_of(b)) & set(gp.GONE[w.name])}
    assert {(M, True), (S, True), (M, False), (S, False)} <= under  # in the phrase and in the group, Must and Should
    for q in qs["miss"]:  # an absent Must empties the query
        must_gone = any(oc == M and set(gp.terms_of(b)) & set(gp.GONE[w.name]) and not (gp.is_group(b) and b[0] == ANY)
                        for oc, b in q)
        assert (len(w.ref.hits(q)[0]) == 0) == must_gone, q


def test_segments_lack_terms():
    """corpus A's first segment is short enough to lack terms the queries use"""
    w = gp.world("A")
    assert gp.SEG_CUTS_A[0] == 0 and gp.SEG_CUTS_A[-1] == w.n and len(set(np.diff(gp.SEG_CUTS_A))) == 3
    first = {int(t) for d in range(gp.SEG_CUTS_A[1]) for f in (w.text, w.namef) for t in f[d]}
    used = {t for v in gp.queries("A").values() for q in v for _, b in q for t in gp.terms_of(b) if t < w.V}
    assert used - first, "every term of the queries occurs in the first segment"
    qs = [q for v in gp.queries("A").values() for q in v]
    differ = sum(not np.array_equal(w.ref.hits(q)[1].view(np.uint32), w.ref.hits(q, seg_bounds=gp.SEG_CUTS_A)[1].view(np.uint32))
                 for q in qs)
    print("queries whose score bits differ once the corpus is cut:", differ)


def test_position_edges():
    """pos_edge on A: a hit whose only match starts at position >= 64; a match that ends on the doc's last token; a doc
    that would match only by running into the next doc's tokens, and does not hit"""
    w = gp.world("A")
    forms = [gp.pos_edge_form(w, q) for q in gp.queries("A")["pos_edge"]]
    for i, f in enumerate(forms):
        assert gp.POS_EDGE_FORMS[i % 3] in f, (i, f)
    assert set().union(*forms) >= set(gp.POS_EDGE_FORMS)


def test_lead_edges_and_the_chunk_bound():
    """lead_edge on B: +"t t" +(a b) for t on each edge list, a group member on each edge list beside "u u"; and, in
    the reference's numbers, k_group's chunk bound fires on the 8193-posting list at k = 1 and 10"""
    w = gp.world("B")
    qs = gp.queries("B")["lead_edge"]
    syn = gr.synth()
    assert [syn.merged_len(t) for t in gp.EDGE_TERMS] == [2047, 2048, 2049, 8193]
    for i, t in enumerate(gp.EDGE_TERMS):
        assert qs[i][0] == gp.P(M, [t, t]) and gp.is_group(qs[i][1][1])
        member_q = qs[4 + i]
        assert any(gp.is_group(b) and t in b[1] for _, b in member_q)
        ph = next(b for _, b in member_q if gp.is_phrase(b))
        assert ph[1][0] == ph[1][1] and ph[1][0] not in gp.EDGE_TERMS
    # "t t" matches exactly the docs with tf(t) >= 2, with count tf - 1: the escaped-tf doc among T_2047's
    t = gr.T_2047
    tf = np.array([int((np.asarray(d) == t).sum()) for d in w.text])
    ct = w.base.text.counts([t, t], [0, 1])
    assert np.array_equal(ct, np.maximum(tf - 1, 0)) and ct.max() == 299
    q = qs[gp.LONG_LEAD]
    assert q[0][0] == X and q[1] == gp.G(M, ANY, [gr.T_LONG, q[1][1][1][1]])
    for k in (1, 10):
        fires, bounds, kth = gp.long_lead_bound(w, q, k)
        print(f"k={k}: chunk bounds {[float(b) for b in bounds]}, k-th score {float(kth)}")
        assert fires and len(bounds) == 5 and bounds[0] >= kth


# ------------------------------------------------------------------ a hand case
def test_four_docs_by_hand():
    """a b c / b a c / a b / c d with "a b" (c OR d): every doc hits; d1, which holds a and b but not the phrase,
    scores exactly what (c OR d) alone gives it"""
    import bool_phrase_ref as bp
    a, b, c, d = 0, 1, 2, 3
    docs = [[a, b, c], [b, a, c], [a, b], [c, d]]
    ref = gp.Ref(bp.Ref(4, docs))
    q = [gp.P(S, [a, b]), gp.G(S, ANY, [c, d])]
    hd, hs = ref.hits(q)
    assert hd.tolist() == [0, 1, 2, 3]
    gd, gs = ref.hits([gp.G(S, ANY, [c, d])])
    assert gd.tolist() == [0, 1, 3]
    assert hs[1].view(np.uint32) == gs[1].view(np.uint32) and hs[3].view(np.uint32) == gs[2].view(np.uint32)
    pd, ps = ref.hits([gp.P(S, [a, b])])
    assert pd.tolist() == [0, 2] and hs[2].view(np.uint32) == ps[1].view(np.uint32)
    assert hs[0] == F(F(F(0.0) + ps[0]) + gs[0])  # Shoulds from 0.0 in clause order
    assert gp.hit_set(ref, gp.phrases_as_groups(q)) == {0, 1, 2, 3} and gp.hit_set(ref, [gp.P(M, [a, b]), gp.G(M, ANY, [c, d])]) == {0}
    qo, terms, occur, plen, ppos = gp.batch([q])
    assert (qo.tolist(), terms.tolist(), occur.tolist()) == ([0, 4], [a, b, c, d], [S] * 4)
    assert plen.tolist() == [2, 0, 2 | gr.FLAG[ANY], 0] and ppos.tolist() == [0, 1, 0, 0]
