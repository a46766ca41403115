"""The reference of field-qualified phrase clauses (tests/field_phrase_ref.py, DESIGN.md
§21) on a small known corpus, and the conditions its generated queries must meet so
that the GPU test (test_gpu_field_phrase.py) compares something: no GPU, nothing of
libfugu.  These are conditions on the generator, not measurements: a seed that
misses one is fixed in the generator."""
import numpy as np
import pytest

import field_phrase_ref as fp

M, S, X = fp.MUST, fp.SHOULD, fp.MUST_NOT
TEXT, NAME = fp.TEXT, fp.NAME
bits = lambda x: np.asarray(x, np.float32).view(np.uint32).tolist()  # noqa: E731


# ------------------------------------------------------------------ a known corpus
# a=0 b=1 c=2 d=3
KAT_TEXT = [[0, 1, 2], [2, 3], [0, 1], [1, 0, 2], [0, 0, 0, 1], [3]]
KAT_NAME = [[], [0, 1], [0, 1], [0, 2, 1], [0, 0, 0], [0, 1]]
KAT_NAME_GAPS = [None, None, None, None, None, [1]]  # doc 5's name: a, a dropped token, b


@pytest.fixture(scope="module")
def kat():
    return fp.Ref(4, KAT_TEXT, None, KAT_NAME, KAT_NAME_GAPS)


def test_presence_is_per_field(kat):
    docs = lambda q: sorted(kat.hits(q)[0].tolist())  # noqa: E731
    assert docs([fp.P([0, 1], S)]) == [0, 1, 2, 4]
    assert docs([fp.P([0, 1], S, NAME)]) == [1, 2]            # doc 0, 4: in the text only; 3: not adjacent; 5: a gap
    assert docs([fp.P([0, 1], S, TEXT)]) == [0, 2, 4]
    assert docs([fp.P([0, 1], S, NAME, [0, 2])]) == [3, 5]    # the offset 2 spans the other word and the gap
    assert docs([fp.P([0, 0], S, NAME)]) == [4] and docs([fp.P([0, 0], S, TEXT)]) == [4]
    assert docs([fp.T(2, M), fp.P([0, 1], X, NAME)]) == [0, 3]
    assert docs([fp.T(0, M, NAME), fp.P([0, 1], M)]) == [1, 2, 4]  # a field term beside a plain phrase
    assert docs([fp.P([0, 1], M, NAME), fp.T(3, M, TEXT)]) == [1]
    assert docs([fp.P([0, fp.MISSING], M, NAME), fp.T(0, S)]) == []
    assert docs([fp.P([0, 9], S, TEXT), fp.T(3, S)]) == [1, 5]     # an absent Should drops out


def test_scores_are_the_fields_part(kat):
    whole = dict(zip(*kat.hits([fp.P([0, 1], S)])))
    nm = dict(zip(*kat.hits([fp.P([0, 1], S, NAME)])))
    tx = dict(zip(*kat.hits([fp.P([0, 1], S, TEXT)])))
    # in one field only: the unqualified clause's bits; in both: the two parts sum to it, text then name
    assert bits(nm[1]) == bits(whole[1]) and bits(tx[0]) == bits(whole[0]) and bits(tx[4]) == bits(whole[4])
    assert bits(np.float32(np.float32(0.0) + tx[2]) + nm[2]) == bits(whole[2])
    # the repeated term: count 2 of `a a` in `a a a`, the idf summed twice
    st = kat.pstats
    w = fp.pr.weight(st.df_name, st.n, [0, 0])
    c = np.float32(2.0)
    want = w * (c / (c + fp.pr.tf_cache(st.tot[1], st.n)[fp.pr.fieldnorm_id(3)]))
    assert bits(dict(zip(*kat.hits([fp.P([0, 0], S, NAME)])))[4]) == bits(want)
    # name:"a b" text:"a b" is "a b"
    both = kat.search([fp.P([0, 1], S, NAME), fp.P([0, 1], S, TEXT)], 10)
    plain = kat.search([fp.P([0, 1], S)], 10)
    assert fp.hits_of(*both) == fp.hits_of(*plain)


def test_cost_orders_the_musts(kat):
    # three Musts: the sum's bits depend on the (cost, position) order; the field phrase's cost is its field's
    # smallest doc count (name: a 5, b 4 -> 4), the term c's 3 + 1, the text phrase's min(4, 4) = 4
    q = [fp.T(2, M), fp.P([0, 1], M, NAME), fp.P([0, 1], M, TEXT)]
    cl = [kat.clause(t, o, f, kat.pstats) for t, o, _, f in q]
    assert [c[1](0, 6) for c in cl] == [4, 4, 4]
    assert [kat.clause([0, 1], [0, 1], NAME, kat.pstats)[1](0, 2), kat.clause([0, 1], [0, 1], None, kat.pstats)[1](0, 6)] \
        == [1, 8]


# ------------------------------------------------------------------ the generated corpus and queries
@pytest.fixture(scope="module")
def world():
    c = fp.synth()
    ref = c.ref()
    kinds = fp.queries()
    want = {k: [ref.search(q, 1000) for q in qs] for k, qs in kinds.items()}
    return c, ref, kinds, want


def test_corpus_shape(world):
    c, ref, kinds, want = world
    assert c.n == fp.N and 0.03 < c.deleted.mean() < 0.07
    assert all(len(c.name[i]) == 0 for i in range(fp.SEG_CUTS[1], fp.SEG_CUTS[2]))  # the nameless segment
    for e, n in fp.EDGES.items():
        assert c.merged_len(e) == n
        inname = sum(1 for x in c.name if e in x)
        assert 0 < inname < sum(1 for x in c.name if fp.E_B in x)  # the lead of name:"E E_B" is E's list
    lens = [c.merged_len(t) for t in range(fp.V)]
    assert sum(1 for x in lens if x > 8192) >= 3            # more than one work item
    assert sum(1 for x in lens if 2048 < x < 8192) >= 3
    assert all(min(d) >= fp.SEG_CUTS[2] for d in (fp.ESC_NAME_DOCS, fp.ESC_TEXT_DOCS))
    assert any(g for g in c.name_gaps if g)


def test_queries_decide_something(world):
    c, ref, kinds, want = world
    assert set(kinds) == set(fp.KINDS) and all(len(v) == fp.PER_KIND == 12 for v in kinds.values())
    for kind in fp.KINDS:
        nhit = sum(len(d) > 0 for _, d in want[kind])
        if kind == fp.LACKING:
            assert nhit == 0
            continue
        assert nhit >= 11, (kind, nhit)
    for kind in fp.DECIDING:  # the field decides: the top 100 differ from the same query with the fields stripped
        diff = 0
        for q, (s, d) in zip(kinds[kind], want[kind]):
            ss, sd = ref.search(fp.strip(q), 100)
            diff += fp.hits_of(s[:100], d[:100]) != fp.hits_of(ss, sd)
        print(kind, "differ from the stripped query:", diff, "of", len(kinds[kind]))
        assert diff >= 6, (kind, diff)


def test_both_fields_equal_the_unqualified_phrase(world):
    c, ref, kinds, want = world
    for q, (s, d) in zip(kinds[fp.EQUAL], want[fp.EQUAL]):
        ps, pd = ref.search([fp.P(q[0][0], S)], 1000)
        assert len(d) > 0 and fp.hits_of(s, d) == fp.hits_of(ps, pd)


def test_ties_cross_the_cut(world):
    c, ref, kinds, want = world
    for i, (s, _) in enumerate(want["tie"]):  # every one of them, at either cut
        for k in (10, 100):
            assert len(s) > k and bits(s[k - 1]) == bits(s[k]), (i, k, len(s))


def test_hand_placed_docs_reach_a_top_10(world):
    c, ref, kinds, want = world
    top = lambda kind, i: set(want[kind][i][1][:10].tolist())  # noqa: E731
    assert set(fp.ESC_NAME_DOCS) <= top("lone_name2", 3)       # tf >= 255 in the name
    assert set(fp.ESC_TEXT_DOCS) <= top("lone_text3", 0)       # tf >= 255 in the text
    assert want["lone_name2"][4][1][0] == fp.REP_DOC           # `a a` in the name `a a a`
    gap = want["lone_name2"][5][1]
    assert any(c.name_gaps[int(d)] for d in gap[:10])          # a dropped token between the two
    for i in range(3):  # the edge lists: docs that hold the phrase in the name only, and in both fields
        d = want["lone_name2"][i][1]
        e = kinds["lone_name2"][i][0][0][0]
        assert any(e not in c.text[int(x)] for x in d[:10])
        assert any(e in c.text[int(x)] for x in d[:10])
