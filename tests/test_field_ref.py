"""Field-qualified term clauses without a GPU: the reference's
identities and the conditions of the generator whose queries test_gpu_field.py
runs -- that every kind is there, that the fields decide which docs hit and what
they score, that `name:a text:a` IS the unqualified `a` bit for bit, that the
queries have hits, that the tie queries tie and that the escaped tfs reach a top
10.  The reference alone must stay within these before the GPU test relies on it."""
import numpy as np
import pytest

import bool_ref as br
import field_ref as fr

M, S, X = fr.MUST, fr.SHOULD, fr.MUST_NOT
TEXT, NAME = fr.TEXT, fr.NAME
F = np.float32


@pytest.fixture(scope="module")
def world():
    c = fr.synth()
    ref = fr.Ref(c.corpus)
    kinds = fr.queries()
    want = {k: [ref.search(q, 1000) for q in qs] for k, qs in kinds.items()}  # computed once, shared, never changed
    return c, ref, kinds, want


def bits(s):
    return np.asarray(s, F).view(np.uint32).tolist()


# ------------------------------------------------------------------ the corpus
def test_corpus_has_the_edges(world):
    c, ref, _, _ = world
    for t, n in fr.EDGE_LEN.items():
        assert c.merged_len(t) == n
        dt, dn = c.corpus.docs(t, 0), c.corpus.docs(t, 1)
        both = len(np.intersect1d(dt, dn))
        assert 0 < both < min(len(dt), len(dn))  # text only, both, name only
    for t in fr.TEXT_ONLY:
        assert len(c.corpus.docs(t, 0)) and not len(c.corpus.docs(t, 1))
    for t in fr.NAME_ONLY:
        assert len(c.corpus.docs(t, 1)) and not len(c.corpus.docs(t, 0))
    for t in fr.BOTH_OVER:
        assert len(np.intersect1d(c.corpus.docs(t, 0), c.corpus.docs(t, 1)))
    for t in fr.BOTH_DISJ:
        assert len(c.corpus.docs(t, 1)) and not len(np.intersect1d(c.corpus.docs(t, 0), c.corpus.docs(t, 1)))
    assert not len(c.corpus.docs(fr.T_ABSENT, 0)) and not len(c.corpus.docs(fr.T_ABSENT, 1))
    # the escaped tfs: >= 255 in one field, 1 in the other, in the same docs
    for t, big, small in ((fr.T_ESC_TEXT, 0, 1), (fr.T_ESC_NAME, 1, 0)):
        for d in fr.ESC_DOCS[t]:
            tf = []
            for f in (big, small):
                docs, tfs = c.corpus._list(c.corpus.fld[f], t)
                tf.append(int(tfs[np.searchsorted(docs, d)]))
                assert docs[np.searchsorted(docs, d)] == d
            assert tf[0] >= 255 and tf[1] == 1 and not c.deleted[d]
    # the segments: T_FEW only in the last, T_LOW only in the first, no name postings at all in the second
    lo, hi = fr.SEG_CUTS[1], fr.SEG_CUTS[2]
    assert c.name_off[hi] == c.name_off[lo] and c.name_off[lo] > 0 and c.name_off[-1] > c.name_off[hi]
    assert c.merged_len(fr.T_FEW) == 40 and c.corpus.docs(fr.T_FEW, 0).min() >= hi
    assert c.corpus.docs(fr.T_LOW, 0).max() < lo
    assert c.deleted.sum() > 100


# ------------------------------------------------------------------ the reference's identities
def test_field_clause_is_the_fields_part(world):
    c, ref, _, _ = world
    st = c.corpus.own
    for t in (fr.T_2047, 6, 12, 20, 50, fr.T_ESC_NAME):
        whole, _ = ref._clause(t, None, st)
        parts = [ref._clause(t, f, st)[0] for f in (TEXT, NAME)]
        on = [p >= 0 for p in parts]
        assert np.array_equal(on[0] | on[1], whole >= 0)
        for f in (0, 1):  # a doc that holds the term in one field only: the unqualified clause's bits
            only = on[f] & ~on[1 - f]
            assert np.array_equal(parts[f][only].view(np.uint32), whole[only].view(np.uint32))
            assert np.array_equal(np.flatnonzero(on[f]), c.corpus.docs(t, f))
        b = on[0] & on[1]  # in both: 0.0 + text + name
        assert np.array_equal((F(0.0) + parts[0][b] + parts[1][b]).view(np.uint32), whole[b].view(np.uint32))
        # the cost prefix is the field's list alone
        for f in (0, 1):
            assert ref._clause(t, f, st)[1][-1] == len(c.corpus.docs(t, f))


def test_unqualified_queries_are_bool_ref(world):
    c, ref, kinds, _ = world
    for k, qs in kinds.items():
        for q in qs[:4]:
            q0 = fr.strip(q)
            s, d = ref.search(q0, 100)
            rs, rd = c.corpus.search([t for _, t, _ in q0], [oc for oc, _, _ in q0], 100)
            assert fr.hits_of(s, d) == br.hits_of(rs, rd), (k, q)


def test_absent_clauses(world):
    c, ref, _, _ = world
    t = 20  # text only
    assert len(ref.search([fr.C(M, t, NAME)], 10)[1]) == 0                       # a Must empties the query
    assert len(ref.search([fr.C(M, 21), fr.C(M, t, NAME)], 10)[1]) == 0
    a = ref.search([fr.C(S, 21), fr.C(S, t, NAME)], 1000)                           # a Should drops out
    b = ref.search([fr.C(S, 21)], 1000)
    assert fr.hits_of(*a) == fr.hits_of(*b)
    a = ref.search([fr.C(M, 21), fr.C(X, t, NAME)], 1000)                           # a MustNot drops out
    b = ref.search([fr.C(M, 21)], 1000)
    assert fr.hits_of(*a) == fr.hits_of(*b)
    # per segment: no name postings in the second one, so `+name:t` has no hit there
    d, _ = ref.hits([fr.C(M, fr.T_LONG, NAME)], seg_bounds=fr.SEG_CUTS)
    assert len(d) and not ((d >= fr.SEG_CUTS[1]) & (d < fr.SEG_CUTS[2])).any()
    nameless = br.Corpus(fr.V, c.text_off, c.text_tok)
    assert len(fr.Ref(nameless).search([fr.C(S, fr.T_EVERY), fr.C(M, 6, NAME)], 10)[1]) == 0


def test_must_order_uses_the_fields_cost(world):
    """three Musts: (s0 + s1) + (0.0 + s2) depends on which clause is last; the field's own doc count decides"""
    c, ref, _, _ = world
    st = c.corpus.own
    found = False
    for a in fr.BOTH_OVER:
        for b in range(16, 40):
            q = [fr.C(M, a, TEXT), fr.C(M, b), fr.C(M, fr.T_EVERY)]
            na, nb = len(c.corpus.docs(a, 0)), len(c.corpus.docs(b, 0))
            if not na < nb < na + len(c.corpus.docs(a, 1)):
                continue  # (b sorts between text:a and the unqualified a)
            s, d = ref.search(q, 1000)
            sa, sb, se = (ref._clause(t, f, st)[0] for _, t, f in q)
            assert np.array_equal(s, (F(0.0) + ((sa[d] + sb[d]) + (F(0.0) + se[d]))))
            found = True
    assert found


# ------------------------------------------------------------------ the generator's conditions
def test_every_kind_is_there(world):
    _, _, kinds, _ = world
    assert set(kinds) == set(fr.KINDS) and len(fr.KINDS) >= 9
    for k, qs in kinds.items():
        assert len(qs) == fr.PER_KIND >= 12, k
        assert all(any(f is not None for _, _, f in q) for q in qs), k  # every query holds a field clause
        assert all(len(q) <= 16 for q in qs)
    assert all(len(q) == 1 for q in kinds["lone"])
    assert {f for q in kinds["lone"] for _, _, f in q} == {TEXT, NAME}
    assert all([oc for oc, _, _ in q] == [M, M] and [f for _, _, f in q] == [NAME, TEXT] for q in kinds["must_nt"])
    assert all([oc for oc, _, _ in q] == [M, M] and [f for _, _, f in q] == [NAME, None] for q in kinds["must_nu"])
    assert all(q[0][1] == q[1][1] and {q[0][2], q[1][2]} == {TEXT, NAME} and q[0][0] == q[1][0] == S
               for q in kinds[fr.EQUAL])
    assert {len(q) for q in kinds["shoulds"]} == {3, 4, 5, 6}
    assert all(all(oc == S for oc, _, _ in q) for q in kinds["shoulds"])
    assert all([(oc, f) for oc, _, f in q] == [(M, None), (X, NAME)] for q in kinds["not_name"])
    assert all([(oc, f) for oc, _, f in q[:2]] == [(M, TEXT), (S, NAME)] for q in kinds["must_should"])
    lead = {q[0][1] for qs in kinds.values() for q in qs}
    assert {fr.T_2047, fr.T_2048, fr.T_2049, fr.T_LONG, fr.T_FEW} <= lead
    used = {t for qs in kinds.values() for q in qs for _, t, _ in q}
    assert fr.T_ABSENT in used and fr.MISSING in used and fr.GONE[1] in used


def test_the_fields_decide(world):
    c, ref, kinds, want = world
    for k in fr.KINDS:
        differ = 0
        for q, w in zip(kinds[k], want[k]):
            # (the equality kind: the two clauses against the ONE unqualified clause)
            flat = ref.search(fr.strip(q)[:1] if k == fr.EQUAL else fr.strip(q), 1000)
            differ += fr.hits_of(*flat) != fr.hits_of(*w)
        print(k, "differ from the stripped query:", differ, "of", len(kinds[k]))
        if k == fr.EQUAL:  # `name:a text:a` is the unqualified `a`: docs and score bits
            assert differ == 0
            assert sum(len(w[1]) > 0 for w in want[k]) == len(want[k])
        else:
            assert 2 * differ >= len(kinds[k]), k


def test_most_queries_have_hits(world):
    _, _, kinds, want = world
    n = [len(w[1]) > 0 for k in fr.KINDS for w in want[k]]
    assert len(n) == fr.PER_KIND * len(fr.KINDS) >= 108 and np.mean(n) >= 0.9
    empty = [q for q, w in zip(kinds["lacking"], want["lacking"]) if len(w[1]) == 0]
    assert empty and all(q[0][0] == M for q in empty)  # a Must on a field the term lacks


def test_tie_queries_tie(world):
    _, _, kinds, want = world
    for k in (10, 100):
        assert any(len(rs) > k and rs[k - 1] == rs[k] for rs, _ in want["tie"]), k
        assert any(len(rs) > k and rs[k - 1] == rs[k] for kind in fr.KINDS for rs, _ in want[kind])


def test_escaped_docs_reach_a_top_10(world):
    c, ref, kinds, want = world
    esc = {d for docs in fr.ESC_DOCS.values() for d in docs}
    top = {int(d) for k in fr.KINDS for _, rd in want[k] for d in rd[:10]}
    assert esc & top
    # and the field decides their score: the big tf's field scores above the small one's
    for t, big in ((fr.T_ESC_TEXT, TEXT), (fr.T_ESC_NAME, NAME)):
        sb = ref._clause(t, big, c.corpus.own)[0]
        ss = ref._clause(t, 1 - big, c.corpus.own)[0]
        for d in fr.ESC_DOCS[t]:
            assert sb[d] > 0 and ss[d] > 0 and sb[d] != ss[d]


def test_batch_arrays():
    q_off, terms, occur, plen, ppos = fr.batch([[fr.C(M, 3, NAME), fr.C(S, 4)], [fr.C(X, 5, TEXT)]])
    assert q_off.tolist() == [0, 2, 3] and terms.tolist() == [3, 4, 5] and occur.tolist() == [M, S, X]
    assert plen.tolist() == [1 | 0x10000000, 1, 1 | 0x20000000] and ppos.tolist() == [0, 0, 0]
