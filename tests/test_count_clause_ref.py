"""tests/count_clause_ref.py (the reference of fg_count_batch with phrase and group
clauses) pinned without a GPU against the references the project
already trusts -- bool_phrase_ref for queries with a phrase, group_ref for queries
with a group, phrase_ref for a lone phrase, count_ref.count_brute for term-only
queries -- and proof that the cases of tests/test_gpu_count_clauses.py bite."""
import numpy as np
import pytest

import bool_phrase_ref as bpr
import bool_ref as br
import count_clause_ref as ccr
import count_ref as cr
import group_ref as gr
import phrase_ref as pr


@pytest.fixture(scope="module")
def main():
    c = ccr.main_corpus()
    return c, ccr.query_batch(c)


def ids(t):
    return ccr.MISSING if t is None else t


def kinds(clauses):
    return {k for k, *_ in clauses}


def csr(docs):
    return (np.cumsum([0] + [len(d) for d in docs]).astype(np.int64),
            np.array([x for d in docs for x in d], np.int64))


def test_phrase_queries_equal_bool_phrase_ref(main):
    c, qs = main
    ref = bpr.Ref(c.n_terms, c.text, c.text_gaps, [nm or [] for nm in c.name], c.name_gaps, c.deleted)
    n = 0
    for lab, clauses, flt in qs:
        if flt or "p" not in kinds(clauses) or kinds(clauses) & {"any", "all"}:
            continue
        docs, _ = ref.hits([([ids(t) for t in ts], offs, oc) for _, oc, ts, offs in clauses])
        assert np.array_equal(np.sort(docs), np.flatnonzero(ccr.match_mask(c, clauses, None))), lab
        n += 1
    assert n >= 20


def test_group_queries_equal_group_ref(main):
    c, qs = main
    to, tt = csr(c.text)
    no, nt = csr([nm or [] for nm in c.name])
    ref = gr.Ref(br.Corpus(c.n_terms, to, tt, no, nt, deleted=c.deleted))
    n = 0
    for lab, clauses, flt in qs:
        if flt or "p" in kinds(clauses) or not kinds(clauses) & {"any", "all"}:
            continue
        q = [(oc, ids(ts[0])) if k == "t" else (oc, (k, [ids(t) for t in ts])) for k, oc, ts, _ in clauses]
        docs, _ = ref.hits(q)
        assert np.array_equal(np.sort(docs), np.flatnonzero(ccr.match_mask(c, clauses, None))), lab
        n += 1
    assert n >= 15


def test_lone_phrases_equal_phrase_ref(main):
    c, qs = main
    st = pr.Stats.of(c.ftext, c.fname, c.n_terms)
    phrases = ccr.phrases_of(qs)
    assert len(phrases) >= 12
    for terms, offs in phrases:
        _, docs, _ = pr.search(c.ftext, c.fname, st, [ids(t) for t in terms], offs, c.n, deleted=c.deleted)
        assert np.array_equal(np.sort(docs), np.flatnonzero(ccr.match_mask(c, [ccr.P(ccr.SHOULD, terms, offs)], None))), terms


def test_term_queries_and_filters_equal_count_brute(main):
    c, qs = main
    cts = list(range(len(c.fdict))) + [None]
    plain = [(cl, fl) for _, cl, fl in qs if kinds(cl) <= {"t"}]
    assert len(plain) >= 6
    as_cr = [([(oc, ts[0]) for _, oc, ts, _ in cl], fl) for cl, fl in plain]
    got, want = ccr.count_batch(c, plain, cts), cr.count_brute(c, as_cr, cts)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # a filter intersects any text match with the facet union, from the docs' own facet tokens
    for lab, cl, fl in qs:
        if fl and cl:
            union = np.array([any(t in c.ftok[d] for t in fl if t is not None) for d in range(c.n)])
            assert np.array_equal(ccr.match_mask(c, cl, fl), ccr.match_mask(c, cl, None) & union), lab


def test_snapshots_sum(main):
    c, qs = main
    plain = [(cl, fl) for _, cl, fl in qs]
    cts = list(range(len(c.fdict)))[:5]
    whole, parts = ccr.count_batch(c, plain, cts), ccr.count_segments(c, [0, 4001, 7010, c.n], plain, cts)
    assert np.array_equal(whole[0], parts[0]) and np.array_equal(whole[1], parts[1])


# ---------------------------------------------------------------- the cases bite
def test_non_empty_queries_match(main):
    c, qs = main
    for lab, cl, fl in qs:
        total = int(ccr.match_mask(c, cl, fl).sum())
        assert (total == 0) == ccr.empty_by_design(lab), (lab, total)
    small = ccr.corpus(65, 7)
    assert int(ccr.match_mask(small, [ccr.P(ccr.MUST, [4, 5])], None)[small.n - 1]) == 1


def test_every_phrase_has_a_decoy(main):
    """a doc that holds all the phrase's terms but not the phrase: the verification decides"""
    c, qs = main
    for terms, offs in ccr.phrases_of(qs):
        if not all(c.present(t) for t in terms):
            continue  # (a term no doc holds: the clause is absent)
        conj = ccr.clause_set(c, ccr.ALL(ccr.MUST, terms))
        phrase = ccr.clause_set(c, ccr.P(ccr.MUST, terms, offs))
        assert (conj & ~phrase & c.alive_mask).any(), terms
        assert not (phrase & ~conj).any()


def test_fields_ends_and_spans(main):
    c, qs = main
    in_text = lambda t, o: c.ftext.counts(t, o) > 0  # noqa: E731
    in_name = lambda t, o: c.fname.counts(t, o) > 0  # noqa: E731
    # a phrase that matches only in `name`, one only in `text`
    assert in_name([ccr.N1, ccr.N2], [0, 1]).any() and not in_text([ccr.N1, ccr.N2], [0, 1]).any()
    assert in_text([ccr.DA, ccr.DB], [0, 1]).any() and not in_name([ccr.DA, ccr.DB], [0, 1]).any()
    # a matching phrase that ends at the last position of its doc: the last doc's, and `3 51`
    last = c.n - 1
    assert c.text[last][-2:] == [4, 5] and in_text([4, 5], [0, 1])[last] and not c.deleted[last]
    d = int(np.flatnonzero(in_text([3, ccr.T2049], [0, 1]))[-1])  # (past the docs that `52 53` ends)
    assert d >= ccr.DENSE_DOCS and c.text[d][-2:] == [3, ccr.T2049] and c.text_gaps[d] is None
    # a phrase match that is a deleted doc
    assert c.deleted[c.n - 2] and in_text([4, 5], [0, 1])[c.n - 2]
    # field length == span (no start fits), == span + 1 (one start), and a hole honoured through phrase_pos
    s = ccr.SPAN0
    hole = in_text([ccr.H1, ccr.H2], [0, 2])
    assert [len(c.text[s + i]) for i in range(3)] == [2, 3, 2] and c.text_gaps[s + 2] == [1]
    assert hole[s:s + 4].tolist() == [False, True, True, False]
    assert in_text([ccr.H1, ccr.H2], [0, 1])[s:s + 4].tolist() == [True, False, False, False]
    # a doc shorter than the span of the phrase tested on it: every doc under [0, 500]
    assert max(len(t) for t in c.text) < 500 and not in_text([0, 1], [0, 500]).any()
    # the driver lists on k_crow's chunk edge, and a chunk whose 2048 candidates all survive the probes
    assert len(c.post[ccr.T2048]) == 2048 and len(c.post[ccr.T2049]) == 2049
    assert c.post[ccr.DA] == c.post[ccr.DB] == set(range(ccr.DENSE_DOCS)) and ccr.DENSE_DOCS > 2 * 2048
