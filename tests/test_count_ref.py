"""CPU checks of the count reference (tests/count_ref.py) and of the corpora the
GPU tests of fg_count_batch run on: a hand case with literal expectations, the
set-based reference against a doc-by-doc evaluation, the properties the main
corpus is meant to have, and the host's refusal of a phrase in a count query."""
import numpy as np
import pytest

import count_ref as cr
from count_ref import MUST as M, MUST_NOT as X, SHOULD as S


def hand_corpus():
    text = [[1, 2], [1], [2, 3], [3], [1, 3], [2], [1, 2], [4]]
    name = [None, None, [1], None, None, None, None, [2]]
    facets = [["/a/x"], ["/a/y", "/b/p"], ["/a/x/deep"], ["/b/q"], ["/a"], [], ["/a/x", "/a/x/deep"], ["/b/p", "/b/q"]]
    deleted = [0, 0, 0, 0, 0, 0, 1, 0]
    return cr.Corpus(text, name, facets, deleted, 16)


def test_hand_case():
    c = hand_corpus()
    f = c.fid
    cts = [f("/a"), f("/a/x"), f("/a/y"), f("/a/x/deep"), f("/b"), f("/b/p"), f("/b/q"), f("/"), None]
    assert None not in cts[:-1] and f("/") == c.fdict[""]
    qs = [([], None),                                  # AllQuery
          ([(M, 1), (M, 2)], None),                    # +1 +2 (doc 2 holds 1 in `name` only; doc 6 is deleted)
          ([(S, 1), (S, 3)], None),                    # 1 3
          ([(S, 2), (X, 1)], None),                    # 2 -1
          ([], [f("/b/p"), f("/a/y")]),                # facet union alone
          ([(S, 1)], [f("/a/x")]),                     # 1, filtered
          ([(M, 9)], None)]                            # a Must the corpus lacks
    want_total = [7, 2, 5, 2, 2, 2, 0]
    want_count = [[4, 2, 1, 1, 3, 2, 2, 6, 0],
                  [2, 2, 0, 1, 0, 0, 0, 2, 0],
                  [4, 2, 1, 1, 2, 1, 1, 5, 0],
                  [0, 0, 0, 0, 1, 1, 1, 1, 0],
                  [1, 0, 1, 0, 2, 2, 1, 2, 0],
                  [2, 2, 0, 1, 0, 0, 0, 2, 0],
                  [0, 0, 0, 0, 0, 0, 0, 0, 0]]
    for fn in (cr.count_batch, cr.count_brute):
        total, count = fn(c, qs, cts)
        assert total.tolist() == want_total, fn.__name__
        assert count.tolist() == want_count, fn.__name__
    # FacetCounts::get: direct children, nonzero, encoded order; doc 4's facet IS /a: under no child
    assert cr.children(c, "/a", c.alive) == [("/a/x", 2), ("/a/y", 1)]
    assert cr.children(c, "/", c.alive) == [("/a", 4), ("/b", 3)]
    assert cr.children(c, "/a/x", c.alive) == [("/a/x/deep", 1)]
    assert cr.tree(c) == [("/a", 4), ("/a/x", 2), ("/a/x/deep", 1), ("/a/y", 1), ("/b", 3), ("/b/p", 2), ("/b/q", 2)]
    assert cr.tree(c, 1) == [("/a", 4), ("/b", 3)]
    assert cr.tree(c, 0) == []


def test_reference_equals_brute_force():
    c = cr.small_corpus()
    qs = [(cl, fl) for _, cl, fl in cr.query_batch(c)]
    cts = list(range(len(c.fdict))) + [None]
    total, count = cr.count_batch(c, qs, cts)
    btotal, bcount = cr.count_brute(c, qs, cts)
    assert np.array_equal(total, btotal)
    assert np.array_equal(count, bcount)
    assert total.max() > 0 and count.max() > 0


@pytest.fixture(scope="module")
def main():
    return cr.main_corpus()


def test_main_corpus_exercises_what_it_is_meant_to(main):
    c = main
    assert c.n == 40037 and c.n % 32 != 0
    flen = sorted(len(v) for v in c.fpost.values())
    assert flen[-1] > 16384 and any(8192 < n for n in flen[:-1])  # several k_cfacet chunks per list
    assert len(c.post[cr.DENSE]) > 4096 and len(c.post[cr.RARE]) < 64
    # two facets under one child of /org; a facet equal to a root; no facet at all
    two = [fl for fl in c.facets if sum(p.startswith("/org/") and "/team/" in p for p in fl) == 2]
    assert two and all(two[0][0].split("/")[2] == p.split("/")[2] for p in two[0][:2])
    assert any("/org" in fl for fl in c.facets) and any(fl == ["/org/3"] or "/org/3" in fl for fl in c.facets)
    assert any(not fl for fl in c.facets)
    # a term in `name` only
    assert cr.NAME_ONLY in c.post and not any(cr.NAME_ONLY in t for t in c.text)
    assert 0.03 < c.deleted.mean() < 0.07
    # the facet dictionary: the root, /org, /org/{0..6}, /org/i/team, /org/i/team/{0..4}, /kind, /kind/{a,b,c}
    assert len(c.fdict) == 1 + 1 + 7 + 7 + 35 + 1 + 3
    qs = cr.query_batch(c)
    assert 60 <= len(qs) <= 72
    total, _ = cr.count_batch(c, [(cl, fl) for _, cl, fl in qs], [])
    for (lab, _, _), t in zip(qs, total):
        if lab.split("|")[0] in cr.EMPTY_BY_DESIGN or lab in cr.EMPTY_BY_DESIGN:
            assert t == 0, lab
        else:
            assert t > 0, lab


def test_facet_counts_refuses_a_phrase():
    """parser level (no device): a phrase clause in a count query is outside the subset"""
    from fugu_amd import db, native
    d = db.Database()
    for q in ('"new york"', "e-mail", 'alpha "new york"'):
        with pytest.raises(native.Unsupported) as e:
            d.facet_counts(None, "/", q)
        assert "phrase clause in a count query" in str(e.value)
    # nothing committed: no facets, no matches
    assert d.facet_counts(None, "/", "alpha") == ([], 0)
    assert d.facet_tree() == []
    with pytest.raises(db.NotFound):
        d.facet_counts("nope", "/")
    with pytest.raises(native.FuguError):
        d.facet_counts(None, "no-leading-slash")
    d.close()
